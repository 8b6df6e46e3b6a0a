// Camera batches of the 4-D stage for gfx950 (contract in animate3d_amd/cameras.py and include/animate3d_hip.h), fp32 at the interface.
// What the reference's data modules compute per step on the CPU (custom/threestudio-animate3d/data/uncond_hybrid.py,
// data/simple_multi_image.py) and what splat.get_cam_info_gaussian recovers from it with two solver calls:
//   spherical_kernel   per-camera (elevation, azimuth, distance, fovy) and an optional perturbation -> the look-at camera
//   random_kernel      HybridRandomCameraIterableDataset.collate (uncond_hybrid.py:195-304, 367-377) on explicit draws
//   from_c2w_kernel    any c2w [B, 4, 4] + fovy -> the rasterizer's inputs, by the adjugate
// One thread per camera.  All arithmetic is fp64 and every output is rounded to fp32 once: B is a few hundred at the most, and the result
// then does not depend on the device's fp32 sinf / asinf.  Plain stores, no atomics, no LDS: a camera's outputs do not depend on the block
// it lands in.  All three end in emit(): c2w -> w2c (row-vector world_view_transform after the OpenGL -> COLMAP flip), full_proj =
// w2c projT, campos, tanfov, in the layout rasterize_gaussians takes.
#include "f32_common.h"

#include <math.h>

namespace {

constexpr double DEG = 0.017453292519943295;      // pi / 180

struct CamOut {            // every pointer [B, ...]; c2w may be NULL (from_c2w_kernel: it is the input)
  float *c2w, *w2c, *full_proj, *campos, *tanfov;
};

struct RandomArgs {
  int B, n_view, total_frame, elev_mode, relative_radius;
  double elev[2], azim[2], fovy[2], dist[2], zoom[2];      // elevation, azimuth and fovy in degrees
  double camera_perturb, center_perturb, up_perturb, znear, zfar;
  const float *obj, *pert_u, *pert_n;
  float *elevation_deg, *azimuth_deg, *fovy_out, *distances;
};

A3D_DEV void normalize3(double* v) {              // F.normalize: v / max(|v|, 1e-12)
  const double n = fmax(sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-12);
  v[0] /= n;
  v[1] /= n;
  v[2] /= n;
}

A3D_DEV void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// w2c [4, 4] row-major fp64 (row-vector form) -> the four rasterizer inputs of camera b.  projT is get_projection_matrix_gaussian's
// matrix transposed, fovx = fovy: its non-zeros are [0][0] = [1][1] = 1 / tan(fovy / 2), [2][2] = zfar / (zfar - znear), [2][3] = 1,
// [3][2] = -zfar znear / (zfar - znear)
A3D_DEV void store_views(const CamOut& o, int64_t b, const double* w2c, const double* pos, double fovy, double znear, double zfar) {
  const double t = tan(0.5 * fovy), a = 1.0 / t, c = zfar / (zfar - znear), d = -(zfar * znear) / (zfar - znear);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o.w2c[16 * b + 4 * i + j] = (float)w2c[4 * i + j];
    o.full_proj[16 * b + 4 * i] = (float)(w2c[4 * i] * a);
    o.full_proj[16 * b + 4 * i + 1] = (float)(w2c[4 * i + 1] * a);
    o.full_proj[16 * b + 4 * i + 2] = (float)(w2c[4 * i + 2] * c + w2c[4 * i + 3] * d);
    o.full_proj[16 * b + 4 * i + 3] = (float)w2c[4 * i + 2];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) o.campos[3 * b + i] = (float)pos[i];
  o.tanfov[b] = (float)t;
}

// The one camera function: (position, centre, up, fovy) -> c2w = [right, up, -lookat | pos] (uncond_hybrid.py:367-377) and, in closed
// form for this rigid matrix, w2c: the flip negates the up and -lookat columns, R' = [right, -up, lookat], w2c = [[R', 0], [-pos R', 1]]
A3D_DEV void emit(const CamOut& o, int64_t b, const double* pos, const double* center, const double* up_in, double fovy, double znear,
                  double zfar) {
  double look[3] = {center[0] - pos[0], center[1] - pos[1], center[2] - pos[2]}, right[3], up[3];
  normalize3(look);
  cross3(look, up_in, right);
  normalize3(right);
  cross3(right, look, up);
  normalize3(up);
  double w2c[16];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float* row = o.c2w + 16 * b + 4 * i;
    row[0] = (float)right[i];
    row[1] = (float)up[i];
    row[2] = (float)-look[i];
    row[3] = (float)pos[i];
    w2c[4 * i] = right[i];
    w2c[4 * i + 1] = -up[i];
    w2c[4 * i + 2] = look[i];
    w2c[4 * i + 3] = 0.0;
  }
  o.c2w[16 * b + 12] = o.c2w[16 * b + 13] = o.c2w[16 * b + 14] = 0.f;
  o.c2w[16 * b + 15] = 1.f;
  w2c[12] = -(pos[0] * right[0] + pos[1] * right[1] + pos[2] * right[2]);
  w2c[13] = pos[0] * up[0] + pos[1] * up[1] + pos[2] * up[2];
  w2c[14] = -(pos[0] * look[0] + pos[1] * look[1] + pos[2] * look[2]);
  w2c[15] = 1.0;
  store_views(o, b, w2c, pos, fovy, znear, zfar);
}

A3D_DEV void on_sphere(double elevation, double azimuth, double distance, double* pos) {      // uncond_hybrid.py:273-280
  pos[0] = distance * cos(elevation) * cos(azimuth);
  pos[1] = distance * cos(elevation) * sin(azimuth);
  pos[2] = distance * sin(elevation);
}

__global__ __launch_bounds__(64) void spherical_kernel(int B, const float* __restrict__ elevation, const float* __restrict__ azimuth,
                                                       const float* __restrict__ distance, const float* __restrict__ fovy,
                                                       const float* __restrict__ perturb, double angle_unit, double znear, double zfar,
                                                       CamOut o) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double pos[3], center[3] = {0.0, 0.0, 0.0}, up[3] = {0.0, 0.0, 1.0};
  on_sphere((double)elevation[b] * angle_unit, (double)azimuth[b] * angle_unit, (double)distance[b], pos);
  if (perturb) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      pos[i] += (double)perturb[9 * b + i];
      center[i] = (double)perturb[9 * b + 3 + i];
      up[i] += (double)perturb[9 * b + 6 + i];
    }
  }
  emit(o, b, pos, center, up, (double)fovy[b] * angle_unit, znear, zfar);
}

__global__ __launch_bounds__(64) void random_kernel(RandomArgs a, CamOut o) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int64_t r = b / ((int64_t)a.n_view * a.total_frame), v = (b / a.total_frame) % a.n_view;   // per object; per (object, view)
  const float* u = a.obj + 5 * r;
  double elev, elev_deg;
  if (a.elev_mode == 0) {                                          // uniform in degrees (:199-205)
    elev_deg = (double)u[0] * (a.elev[1] - a.elev[0]) + a.elev[0];
    elev = elev_deg * DEG;
  } else {                                                         // uniform on the sphere: inverse transform (:207-223)
    const double s0 = sin(a.elev[0] * DEG), s1 = sin(a.elev[1] * DEG);
    elev = asin((double)u[0] * (s1 - s0) + s0);
    elev_deg = elev / DEG;
  }
  const double azim_deg = ((double)u[1] + (double)v) / (double)a.n_view * (a.azim[1] - a.azim[0]) + a.azim[0];    // :232-240
  double fovy_deg = (double)u[2] * (a.fovy[1] - a.fovy[0]) + a.fovy[0];
  double fovy = fovy_deg * DEG;
  double dist = (double)u[3] * (a.dist[1] - a.dist[0]) + a.dist[0];
  if (a.relative_radius) dist *= 1.0 / tan(0.5 * fovy);            // before the zoom multiplies fovy (:257-267)
  const double zoom = (double)u[4] * (a.zoom[1] - a.zoom[0]) + a.zoom[0];
  fovy *= zoom;
  fovy_deg *= zoom;
  double pos[3], center[3], up[3] = {0.0, 0.0, 1.0};
  on_sphere(elev, azim_deg * DEG, dist, pos);
#pragma unroll
  for (int i = 0; i < 3; ++i) {                                    // :289-304
    pos[i] += (double)a.pert_u[3 * b + i] * 2.0 * a.camera_perturb - a.camera_perturb;
    center[i] = (double)a.pert_n[6 * b + i] * a.center_perturb;
    up[i] += (double)a.pert_n[6 * b + 3 + i] * a.up_perturb;
  }
  a.elevation_deg[b] = (float)elev_deg;
  a.azimuth_deg[b] = (float)azim_deg;
  a.fovy_out[b] = (float)fovy;
  a.distances[b] = (float)dist;
  emit(o, b, pos, center, up, fovy, a.znear, a.zfar);
}

A3D_DEV double det3(double a, double b, double c, double d, double e, double f, double g, double h, double i) {
  return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
}

// w2c = inverse(c2w diag(1, -1, -1, 1)) transposed, by the adjugate; campos = inverse(w2c)[3, :3], which is c2w[:3, 3] exactly
__global__ __launch_bounds__(64) void from_c2w_kernel(int B, const float* __restrict__ c2w, const float* __restrict__ fovy, double znear,
                                                      double zfar, CamOut o) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double m[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) m[4 * i + j] = (double)c2w[16 * b + 4 * i + j] * ((j == 1 || j == 2) ? -1.0 : 1.0);
  double cof[16];                                                  // cof[i][j]: the signed minor of m[i][j]; inverse[j][i] = cof[i][j] / det
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r0 = i == 0 ? 1 : 0, r1 = i <= 1 ? 2 : 1, r2 = i <= 2 ? 3 : 2, c0 = j == 0 ? 1 : 0, c1 = j <= 1 ? 2 : 1, c2 = j <= 2 ? 3 : 2;
      const double minor = det3(m[4 * r0 + c0], m[4 * r0 + c1], m[4 * r0 + c2], m[4 * r1 + c0], m[4 * r1 + c1], m[4 * r1 + c2],
                                m[4 * r2 + c0], m[4 * r2 + c1], m[4 * r2 + c2]);
      cof[4 * i + j] = ((i + j) & 1) ? -minor : minor;
    }
  }
  const double det = m[0] * cof[0] + m[1] * cof[1] + m[2] * cof[2] + m[3] * cof[3];
  double w2c[16];                                                  // inverse transposed: w2c[i][j] = inverse[j][i] = cof[i][j] / det
#pragma unroll
  for (int k = 0; k < 16; ++k) w2c[k] = cof[k] / det;
  const double pos[3] = {(double)c2w[16 * b + 3], (double)c2w[16 * b + 7], (double)c2w[16 * b + 11]};
  store_views(o, b, w2c, pos, (double)fovy[b], znear, zfar);
}

bool planes_ok(double znear, double zfar) { return isfinite(znear) && isfinite(zfar) && znear > 0.0 && zfar > znear; }

bool out_ok(const CamOut& o, bool need_c2w) {
  return (o.c2w || !need_c2w) && o.w2c && o.full_proj && o.campos && o.tanfov && a3d_aligned(4, o.c2w, o.w2c, o.full_proj, o.campos, o.tanfov);
}

}  // namespace

extern "C" int a3d_cameras_spherical_f32(a3d_stream_t stream, int B, const float* elevation, const float* azimuth, const float* distance,
                                         const float* fovy, const float* perturb, double angle_unit, double znear, double zfar, float* c2w,
                                         float* w2c, float* full_proj, float* campos, float* tanfov) {
  const CamOut o{c2w, w2c, full_proj, campos, tanfov};
  if (B <= 0 || !elevation || !azimuth || !distance || !fovy || !out_ok(o, true) || !planes_ok(znear, zfar)) return A3D_EINVAL;
  if (!(angle_unit > 0.0) || !isfinite(angle_unit) || !a3d_aligned(4, elevation, azimuth, distance, fovy, perturb)) return A3D_EINVAL;
  spherical_kernel<<<blocks_for(B, 64), 64, 0, (hipStream_t)stream>>>(B, elevation, azimuth, distance, fovy, perturb, angle_unit, znear, zfar, o);
  return a3d_launch_status();
}

extern "C" int a3d_cameras_random_f32(a3d_stream_t stream, int R, int n_view, int total_frame, const float* obj, const float* pert_u,
                                      const float* pert_n, const double* ranges10, int elev_mode, int relative_radius, double camera_perturb,
                                      double center_perturb, double up_perturb, double znear, double zfar, float* c2w, float* w2c,
                                      float* full_proj, float* campos, float* tanfov, float* elevation_deg, float* azimuth_deg, float* fovy,
                                      float* camera_distances) {
  const CamOut o{c2w, w2c, full_proj, campos, tanfov};
  if (R <= 0 || n_view <= 0 || total_frame <= 0 || (int64_t)R * n_view * total_frame > (int64_t)1 << 24) return A3D_EINVAL;
  if (!obj || !pert_u || !pert_n || !ranges10 || !out_ok(o, true) || !planes_ok(znear, zfar)) return A3D_EINVAL;
  if (!elevation_deg || !azimuth_deg || !fovy || !camera_distances || (elev_mode != 0 && elev_mode != 1)) return A3D_EINVAL;
  if (!a3d_aligned(4, obj, pert_u, pert_n, elevation_deg, azimuth_deg, fovy, camera_distances)) return A3D_EINVAL;
  for (int i = 0; i < 10; ++i)
    if (!isfinite(ranges10[i])) return A3D_EINVAL;
  if (!isfinite(camera_perturb) || !isfinite(center_perturb) || !isfinite(up_perturb)) return A3D_EINVAL;
  RandomArgs a{};
  a.B = R * n_view * total_frame;
  a.n_view = n_view;
  a.total_frame = total_frame;
  a.elev_mode = elev_mode;
  a.relative_radius = relative_radius != 0;
  for (int i = 0; i < 2; ++i) {
    a.elev[i] = ranges10[i];
    a.azim[i] = ranges10[2 + i];
    a.fovy[i] = ranges10[4 + i];
    a.dist[i] = ranges10[6 + i];
    a.zoom[i] = ranges10[8 + i];
  }
  a.camera_perturb = camera_perturb;
  a.center_perturb = center_perturb;
  a.up_perturb = up_perturb;
  a.znear = znear;
  a.zfar = zfar;
  a.obj = obj;
  a.pert_u = pert_u;
  a.pert_n = pert_n;
  a.elevation_deg = elevation_deg;
  a.azimuth_deg = azimuth_deg;
  a.fovy_out = fovy;
  a.distances = camera_distances;
  random_kernel<<<blocks_for(a.B, 64), 64, 0, (hipStream_t)stream>>>(a, o);
  return a3d_launch_status();
}

extern "C" int a3d_cameras_from_c2w_f32(a3d_stream_t stream, int B, const float* c2w, const float* fovy, double znear, double zfar, float* w2c,
                                        float* full_proj, float* campos, float* tanfov) {
  const CamOut o{nullptr, w2c, full_proj, campos, tanfov};
  if (B <= 0 || !c2w || !fovy || !out_ok(o, false) || !planes_ok(znear, zfar) || !a3d_aligned(4, c2w, fovy)) return A3D_EINVAL;
  from_c2w_kernel<<<blocks_for(B, 64), 64, 0, (hipStream_t)stream>>>(B, c2w, fovy, znear, zfar, o);
  return a3d_launch_status();
}
