// Mesh ingest for gfx950: the Gaussians of the 4-D stage's mesh-animation branch from a triangle mesh, and the rigid transform of a
// Gaussian PLY (contract in animate3d_amd/mesh.py and include/animate3d_hip.h), fp32 at the interface.
//   mesh_vertex_kernel    what tools/mesh_animation/mesh2gaussian.py computes with Python loops over faces and vertices
//                         (compute_edge_distances, convert_to_textureVertex_with_average, the distances of
//                         find_and_save_connected_vertices, convert_point_cloud_to_gaussian) followed by Gaussian4DModel.load_ply's
//                         transform: one thread per vertex walks its CSR adjacency row (edge lengths, the per-axis mean |x_u - x_v|)
//                         and its corner list (the mean corner colour, sampled bilinearly from the texture where there is one).
//                         No atomics, no LDS, no per-thread array: every sum runs in list order, so the result does not depend on the
//                         launch geometry.  Sums and the bilinear blend are fp32; the rotation of the position and the SH offset are
//                         fp64 with one rounding (nine multiplications per vertex)
//   rigid_kernel          load_ply's transform of N Gaussians (gaussian_4d.py:196-260): position, log-scale, orientation
#include "f32_common.h"

#include <math.h>

namespace {

constexpr double SH_C0 = 0.28209479177387814;

struct Frame {           // R row-major, the scale factor, and for rigid_kernel R's quaternion (w, x, y, z) and log(scale)
  double R[9], scale, q[4], log_scale;
};

struct MeshArgs {
  int Nv, E, C, Ht, Wt, Nt;
  const float* verts;
  const int *row_start, *col, *corner_order, *corner_start;
  const float *vertex_colors, *corner_colors, *texture, *uvs;
  const int* corner_uv;
  double shrink;
  float *xyz, *scaling, *shs, *colors, *mean_edge, *edge_length;
};

A3D_DEV int clampi(int i, int n) { return max(0, min(i, n - 1)); }

A3D_DEV void rotate_scale(const Frame& f, float x, float y, float z, float* out) {
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = (float)(f.scale * (f.R[3 * i] * (double)x + f.R[3 * i + 1] * (double)y + f.R[3 * i + 2] * (double)z));
}

// F.grid_sample(flip(texture, rows), uv * 2 - 1, bilinear, border, align_corners=True) at one (u, v): pixel coordinates u (Wt - 1) and
// v (Ht - 1), clamped to the image (a NaN goes to 0), row y of the flipped image being row Ht - 1 - y of the texture as stored
A3D_DEV void sample_texture(const float* __restrict__ tex, int Ht, int Wt, float u, float v, float* rgb) {
  const float x = fminf(fmaxf(u * (float)(Wt - 1), 0.f), (float)(Wt - 1)), y = fminf(fmaxf(v * (float)(Ht - 1), 0.f), (float)(Ht - 1));
  const float xf = floorf(x), yf = floorf(y);
  const float wx = x - xf, wy = y - yf;
  const int x0 = clampi((int)xf, Wt), x1 = min(x0 + 1, Wt - 1), y0 = clampi((int)yf, Ht), y1 = min(y0 + 1, Ht - 1);
  const float* r0 = tex + (int64_t)(Ht - 1 - y0) * Wt * 3;
  const float* r1 = tex + (int64_t)(Ht - 1 - y1) * Wt * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = r0[x0 * 3 + c] * (1.f - wx) + r0[x1 * 3 + c] * wx, bottom = r1[x0 * 3 + c] * (1.f - wx) + r1[x1 * 3 + c] * wx;
    rgb[c] = top * (1.f - wy) + bottom * wy;
  }
}

// Indices read from memory (col, corner_order, corner_uv) and the row bounds are clamped to their arrays: a bad one gives a wrong
// value, never an access out of bounds.
__global__ __launch_bounds__(256) void mesh_vertex_kernel(MeshArgs a, Frame f) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= a.Nv) return;
  const float x = a.verts[3 * (int64_t)v], y = a.verts[3 * (int64_t)v + 1], z = a.verts[3 * (int64_t)v + 2];
  const int b = max(0, min(a.row_start[v], a.E)), e = max(b, min(a.row_start[v + 1], a.E));
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int p = b; p < e; ++p) {
    const int64_t n = clampi(a.col[p], a.Nv);
    const float dx = a.verts[3 * n] - x, dy = a.verts[3 * n + 1] - y, dz = a.verts[3 * n + 2] - z;
    sx += fabsf(dx);
    sy += fabsf(dy);
    sz += fabsf(dz);
    a.edge_length[p] = sqrtf(dx * dx + dy * dy + dz * dz);
  }
  const float d = (float)(e - b);
  const float mean[3] = {e > b ? sx / d : 0.f, e > b ? sy / d : 0.f, e > b ? sz / d : 0.f};     // no neighbour: the reference's zero

  float rgb[3];
  if (a.vertex_colors) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = a.vertex_colors[3 * (int64_t)v + c];
  } else {
    const int cb = max(0, min(a.corner_start[v], a.C)), ce = max(cb, min(a.corner_start[v + 1], a.C));
    float s[3] = {0.f, 0.f, 0.f};
    for (int p = cb; p < ce; ++p) {
      const int64_t k = clampi(a.corner_order[p], a.C);
      float t[3];
      if (a.texture) {
        const int64_t i = clampi(a.corner_uv[k], a.Nt);
        sample_texture(a.texture, a.Ht, a.Wt, a.uvs[2 * i], a.uvs[2 * i + 1], t);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = a.corner_colors[3 * k + c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += t[c];
    }
    const float n = (float)max(ce - cb, 1);                                                      // verts_count.clamp(min=1)
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = s[c] / n;
  }

  float pos[3];
  rotate_scale(f, x, y, z, pos);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t o = 3 * (int64_t)v + c;
    a.xyz[o] = pos[c];
    a.mean_edge[o] = mean[c];
    a.scaling[o] = logf((float)((double)mean[c] / a.shrink * f.scale));                          // log(0) = -inf, as the reference's
    a.colors[o] = rgb[c];
    a.shs[o] = (float)(((double)rgb[c] - 0.5) / SH_C0);
  }
}

__global__ __launch_bounds__(256) void rigid_kernel(int N, const float* __restrict__ xyz_in, const float* __restrict__ scaling_in,
                                                    const float* __restrict__ rotation_in, Frame f, float* __restrict__ xyz,
                                                    float* __restrict__ scaling, float* __restrict__ rotation) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  float pos[3];
  rotate_scale(f, xyz_in[3 * i], xyz_in[3 * i + 1], xyz_in[3 * i + 2], pos);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    xyz[3 * i + c] = pos[c];
    scaling[3 * i + c] = (float)((double)scaling_in[3 * i + c] + f.log_scale);
  }
  const double w = rotation_in[4 * i], qx = rotation_in[4 * i + 1], qy = rotation_in[4 * i + 2], qz = rotation_in[4 * i + 3];
  const double inv = 1.0 / sqrt(w * w + qx * qx + qy * qy + qz * qz);
  const double* r = f.q;                                                                         // q' = q_R (x) q / |q|, Hamilton product
  rotation[4 * i] = (float)((r[0] * w - r[1] * qx - r[2] * qy - r[3] * qz) * inv);
  rotation[4 * i + 1] = (float)((r[0] * qx + r[1] * w + r[2] * qz - r[3] * qy) * inv);
  rotation[4 * i + 2] = (float)((r[0] * qy - r[1] * qz + r[2] * w + r[3] * qx) * inv);
  rotation[4 * i + 3] = (float)((r[0] * qz + r[1] * qy - r[2] * qx + r[3] * w) * inv);
}

bool frame_of(Frame& f, const double* rot9, const double* quat4, double scale_factor) {
  if (!rot9 || !(scale_factor > 0.0) || !isfinite(scale_factor)) return false;
  for (int i = 0; i < 9; ++i) f.R[i] = rot9[i];
  for (int i = 0; i < 4; ++i) f.q[i] = quat4 ? quat4[i] : (i == 0 ? 1.0 : 0.0);
  f.scale = scale_factor;
  f.log_scale = log(scale_factor);
  return true;
}

}  // namespace

extern "C" int a3d_mesh_vertex_gaussians_f32(a3d_stream_t stream, int Nv, int E, int C, const float* verts, const int* row_start, const int* col,
                                             const int* corner_order, const int* corner_start, const float* vertex_colors,
                                             const float* corner_colors, const float* texture, int Ht, int Wt, const float* uvs, int Nt,
                                             const int* corner_uv, const double* rot9, double scale_factor, double shrink, float* xyz,
                                             float* scaling, float* shs, float* colors, float* mean_edge, float* edge_length) {
  Frame f;
  if (Nv <= 0 || E < 0 || C < 0 || !verts || !row_start || (!col && E > 0) || (!edge_length && E > 0)) return A3D_EINVAL;
  if (!xyz || !scaling || !shs || !colors || !mean_edge) return A3D_EINVAL;
  if ((vertex_colors != nullptr) + (corner_colors != nullptr) + (texture != nullptr) != 1) return A3D_EINVAL;
  if (!vertex_colors && (!corner_order || !corner_start || C < 1)) return A3D_EINVAL;
  if (texture && (Ht < 1 || Wt < 1 || Nt < 1 || !uvs || !corner_uv || (int64_t)Ht * Wt > (int64_t)1 << 28)) return A3D_EINVAL;
  if (!(shrink > 0.0) || !isfinite(shrink) || !frame_of(f, rot9, nullptr, scale_factor)) return A3D_EINVAL;
  if (!a3d_aligned(4, verts, vertex_colors, corner_colors, texture, uvs) || !a3d_aligned(4, xyz, scaling, shs, colors, mean_edge, edge_length) ||
      !a3d_aligned(4, row_start, col, corner_order, corner_start, corner_uv))
    return A3D_EINVAL;
  const MeshArgs a{Nv, E, C, Ht, Wt, Nt, verts, row_start, col, corner_order, corner_start, vertex_colors, corner_colors, texture, uvs, corner_uv,
                   shrink, xyz, scaling, shs, colors, mean_edge, edge_length};
  mesh_vertex_kernel<<<blocks_for(Nv), 256, 0, (hipStream_t)stream>>>(a, f);
  return a3d_launch_status();
}

extern "C" int a3d_gaussians_rigid_f32(a3d_stream_t stream, int N, const float* xyz_in, const float* scaling_in, const float* rotation_in,
                                       const double* rot9, const double* quat4, double scale_factor, float* xyz, float* scaling,
                                       float* rotation) {
  Frame f;
  if (N <= 0 || !xyz_in || !scaling_in || !rotation_in || !quat4 || !xyz || !scaling || !rotation) return A3D_EINVAL;
  if (!frame_of(f, rot9, quat4, scale_factor)) return A3D_EINVAL;
  if (!a3d_aligned(4, xyz_in, scaling_in, rotation_in, xyz, scaling, rotation)) return A3D_EINVAL;
  rigid_kernel<<<blocks_for(N), 256, 0, (hipStream_t)stream>>>(N, xyz_in, scaling_in, rotation_in, f, xyz, scaling, rotation);
  return a3d_launch_status();
}
