// Mesh export for gfx950: the per-frame vertex normals of a deforming triangle mesh (contract in animate3d_amd/mesh_export.py and
// include/animate3d_hip.h), fp32 at the interface.
//   vertex_normals_kernel  what a DCC tool recomputes for every shape key of tools/mesh_animation/export_animated_mesh.py: one thread per
//                          (frame, vertex) walks the vertex's corner list (the plan mesh_vertex_kernel reads) in ascending corner order
//                          and adds the cross product of the two edges that leave the corner, i.e. twice the face's area times its
//                          normal.  Gather form: no atomics, no LDS, no per-thread array, so the sum does not depend on the launch
//                          geometry.  Differences, products and the sum are fp64 without contraction (a face with two equal corners,
//                          or with parallel edges that are exact multiples, adds exactly 0); the normalisation is fp64 and the result
//                          is rounded to fp32 once
#include "f32_common.h"

#include <math.h>

namespace {

A3D_DEV int clampi(int i, int n) { return max(0, min(i, n - 1)); }

// Indices read from memory (starts, order, faces) are clamped to their arrays: a bad one gives a wrong value, never an access out of
// bounds.  T Nv 3 < 2^31 (checked by the entry point), so every offset fits in 32 bits; they are computed in 64 all the same.
__global__ __launch_bounds__(256) void vertex_normals_kernel(int total, int Nv, int C, const float* __restrict__ pos,
                                                             const int* __restrict__ faces, const int* __restrict__ order,
                                                             const int* __restrict__ starts, float* __restrict__ nrm) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int t = i / Nv, v = i - t * Nv;
  const float* __restrict__ P = pos + 3 * (int64_t)t * Nv;
  const int cb = max(0, min(starts[v], C)), ce = max(cb, min(starts[v + 1], C));
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int p = cb; p < ce; ++p) {
    const int c = clampi(order[p], C);
    const int f3 = c / 3 * 3, k = c - f3;
    const int64_t a = clampi(faces[c], Nv), b = clampi(faces[f3 + (k + 1) % 3], Nv), d = clampi(faces[f3 + (k + 2) % 3], Nv);
    const double ax = P[3 * a], ay = P[3 * a + 1], az = P[3 * a + 2];
    const double ux = (double)P[3 * b] - ax, uy = (double)P[3 * b + 1] - ay, uz = (double)P[3 * b + 2] - az;
    const double wx = (double)P[3 * d] - ax, wy = (double)P[3 * d + 1] - ay, wz = (double)P[3 * d + 2] - az;
    sx += uy * wz - uz * wy;
    sy += uz * wx - ux * wz;
    sz += ux * wy - uy * wx;
  }
  const double len2 = sx * sx + sy * sy + sz * sz;
  float n[3] = {0.f, 0.f, 1.f};                           // no area at this vertex, or a non-finite position: glTF wants a unit normal
  if (len2 > 0.0 && isfinite(len2)) {
    const double len = sqrt(len2);
    n[0] = (float)(sx / len);
    n[1] = (float)(sy / len);
    n[2] = (float)(sz / len);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) nrm[3 * (int64_t)i + c] = n[c];
}

}  // namespace

extern "C" int a3d_mesh_vertex_normals_f32(a3d_stream_t stream, int T, int Nv, int C, const float* pos, const int* faces, const int* order,
                                           const int* starts, float* nrm) {
  if (T < 1 || Nv < 1 || C < 3 || C % 3 != 0 || !pos || !faces || !order || !starts || !nrm) return A3D_EINVAL;
  if ((int64_t)T * Nv * 3 >= (int64_t)1 << 31) return A3D_EINVAL;
  if (!a3d_aligned(4, pos, nrm) || !a3d_aligned(4, faces, order, starts)) return A3D_EINVAL;
  const int total = T * Nv;
  vertex_normals_kernel<<<blocks_for(total), 256, 0, (hipStream_t)stream>>>(total, Nv, C, pos, faces, order, starts, nrm);
  return a3d_launch_status();
}
