// 4-D Gaussian deformation field (two-scale HexPlane / K-Planes grid + five 32-wide MLPs), forward and backward, fp32, every frame of a
// step in one call.  The contract is written out in animate3d_amd/deform4d.py.
//
// Planes arrive repacked texel-major ([H][W][16] per plane, one 64-byte line per texel) in one buffer; plane k = 6 s + p with p over the
// coordinate pairs (x,y) (x,z) (x,t) (y,z) (y,t) (z,t).  MLP weights arrive as [5][1152]: per network layers.0.weight [32][32] then
// layers.2.weight padded to [4][32], networks in the order delta_xyz, delta_rot, delta_scaling, global_rot, global_trans.
//
// Forward stages
//   spatial          one thread per Gaussian: product of the three spatial planes per scale, sp [N, 32] (xyz is fixed: once per call)
//   mean_partial     per (frame, 256 Gaussians): hidden = sp * time planes, summed over the block in index order        (use_global_trans)
//   frame            per frame (32 threads): partials in order -> mean; global_rot / global_trans MLPs; R = Rz Ry Rx, trans
//   deform           per (frame, Gaussian): hidden, three MLPs on the VALU (weights wave-uniform), activations, global transform; the result
//                    is written to every image of the frame
// Backward stages
//   bwd_global_partial  per (frame, 256 Gaussians): the cotangents of R (9) and trans (3), block sums in index order    (use_global_trans)
//   bwd_frame           per frame: partials in order; Euler / sigmoid / global MLPs backward; d mean / N; global weight gradients per frame
//   bwd                 per (frame, 512 Gaussians), 128 threads: recompute, three MLPs backward; d hidden [T, N, 32]; per-frame d scaling /
//                       d rotation; weight gradients as outer products summed over the block through LDS in row order, one slab per block
//   wreduce             slabs of a frame in block order -> per-frame weight gradients; sum_leading (f32_common.h) adds frames in order
//   bwd_spatial         per Gaussian: d sp = sum over frames (in order) of d hidden * time product; per spatial plane sample gradient [N, 3, 32]
//   sgather / tgather   gather-form plane gradients: per texel (per frame row for the time planes), the Gaussians of the adjacent cells in
//                       the cached stable-sorted order, split over a fixed number of slices that are added in slice order
//   tcombine            time-plane texel = sum over frames (in order) of the frame's row times its t weight
// No atomics anywhere: gradients are bitwise reproducible and independent of how images map to frames.
//
// Only fp32 entry points: compiled out of the fp16-storage pass of build.py so they are exported once.
#include "f32_common.h"

namespace {

constexpr int DG_C = 16;            // channels per scale
constexpr int DG_F = 32;            // hidden features = 2 scales x 16
constexpr int DG_P = 12;            // planes
constexpr int DG_NETW = 1152;       // floats per network: 32 x 32 + 4 x 32
constexpr int DG_BLOCK = 256;
constexpr int DG_BWD_BLOCK = 128;   // rows per outer-product tile of the backward
constexpr int DG_BWD_SUB = 4;       // tiles per block: one weight-gradient slab per 512 (frame, Gaussian) rows
constexpr int DG_LD = 33;           // LDS row stride of the 32-wide tiles (odd: conflict-free)
constexpr int DG_SLICES_S = 4, DG_SLICES_T = 16;

struct DgPlanes {
  int64_t off[DG_P];                // float offset of plane k in the packed buffer
  int W[DG_P], H[DG_P];             // W: resolution of the pair's first coordinate, H: of its second
};

struct DgArgs {
  int T, N, B, flags;               // flags: 1 use_global_trans, 2 deform_scales, 4 first_frame_trainable
  const float* xyz;                 // [N, 3]
  const float* scaling;             // [N, 3]
  const float* rotation;            // [N, 4]
  const float* ts;                  // [T]
  const float* grid;                // packed planes
  const float* w;                   // [5, 1152]
  const int* img_start;             // [T + 1]
  const int* img_list;              // [B] images of each frame, ascending
  DgPlanes P;
};

struct DgLerp { int i0; float w1; };

// grid_sample's align_corners=True unnormalisation with padding_mode="border": the cell and the weight of its upper texel
A3D_DEV DgLerp dg_lerp(float u, int R) {
  float x = ((u + 1.f) * 0.5f) * (float)(R - 1);
  x = fminf((float)(R - 1), fmaxf(x, 0.f));
  const int i0 = min((int)x, R - 2);
  DgLerp l; l.i0 = i0; l.w1 = x - (float)i0;
  return l;
}

A3D_DEV bool dg_bypass(const DgArgs& a, float t) { return !(a.flags & 4) && t == -1.f; }

// v[c] *= bilinear sample of plane k, 16 channels
A3D_DEV void dg_sample_mul(const float* __restrict__ grid, const DgPlanes& P, int k, DgLerp lx, DgLerp ly, float (&v)[DG_C]) {
  const float4* r0 = reinterpret_cast<const float4*>(grid + P.off[k] + ((int64_t)ly.i0 * P.W[k] + lx.i0) * DG_C);
  const float4* r1 = r0 + (int64_t)P.W[k] * (DG_C / 4);
  const float wx0 = 1.f - lx.w1, wy0 = 1.f - ly.w1;
  const float w00 = wx0 * wy0, w01 = lx.w1 * wy0, w10 = wx0 * ly.w1, w11 = lx.w1 * ly.w1;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 a = r0[q], b = r0[4 + q], c = r1[q], d = r1[4 + q];
    v[4 * q + 0] *= a.x * w00 + b.x * w01 + c.x * w10 + d.x * w11;
    v[4 * q + 1] *= a.y * w00 + b.y * w01 + c.y * w10 + d.y * w11;
    v[4 * q + 2] *= a.z * w00 + b.z * w01 + c.z * w10 + d.z * w11;
    v[4 * q + 3] *= a.w * w00 + b.w * w01 + c.w * w10 + d.w * w11;
  }
}

// the same sample, one channel (the gather kernels run one thread per channel)
A3D_DEV float dg_sample1(const float* __restrict__ grid, const DgPlanes& P, int k, DgLerp lx, DgLerp ly, int c) {
  const float* r0 = grid + P.off[k] + ((int64_t)ly.i0 * P.W[k] + lx.i0) * DG_C + c;
  const float* r1 = r0 + (int64_t)P.W[k] * DG_C;
  const float wx0 = 1.f - lx.w1, wy0 = 1.f - ly.w1;
  return r0[0] * (wx0 * wy0) + r0[DG_C] * (lx.w1 * wy0) + r1[0] * (wx0 * ly.w1) + r1[DG_C] * (lx.w1 * ly.w1);
}

// product of the three spatial planes of scale s: (x,y) (x,z) (y,z)
A3D_DEV void dg_spatial_prod(const float* __restrict__ grid, const DgPlanes& P, int s, float x, float y, float z, float (&v)[DG_C]) {
#pragma unroll
  for (int c = 0; c < DG_C; ++c) v[c] = 1.f;
  const int k = 6 * s;
  dg_sample_mul(grid, P, k + 0, dg_lerp(x, P.W[k + 0]), dg_lerp(y, P.H[k + 0]), v);
  dg_sample_mul(grid, P, k + 1, dg_lerp(x, P.W[k + 1]), dg_lerp(z, P.H[k + 1]), v);
  dg_sample_mul(grid, P, k + 3, dg_lerp(y, P.W[k + 3]), dg_lerp(z, P.H[k + 3]), v);
}

// product of the three time planes of scale s: (x,t) (y,t) (z,t)
A3D_DEV void dg_time_prod(const float* __restrict__ grid, const DgPlanes& P, int s, float x, float y, float z, float t, float (&v)[DG_C]) {
#pragma unroll
  for (int c = 0; c < DG_C; ++c) v[c] = 1.f;
  const int k = 6 * s;
  dg_sample_mul(grid, P, k + 2, dg_lerp(x, P.W[k + 2]), dg_lerp(t, P.H[k + 2]), v);
  dg_sample_mul(grid, P, k + 4, dg_lerp(y, P.W[k + 4]), dg_lerp(t, P.H[k + 4]), v);
  dg_sample_mul(grid, P, k + 5, dg_lerp(z, P.W[k + 5]), dg_lerp(t, P.H[k + 5]), v);
}

A3D_DEV void dg_hidden(const DgArgs& a, const float* __restrict__ sp, int n, float x, float y, float z, float t, float (&h)[DG_F]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float v[DG_C];
    dg_time_prod(a.grid, a.P, s, x, y, z, t, v);
    const float4* src = reinterpret_cast<const float4*>(sp + (int64_t)n * DG_F + s * DG_C);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 p = src[q];
      h[s * DG_C + 4 * q + 0] = p.x * v[4 * q + 0]; h[s * DG_C + 4 * q + 1] = p.y * v[4 * q + 1];
      h[s * DG_C + 4 * q + 2] = p.z * v[4 * q + 2]; h[s * DG_C + 4 * q + 3] = p.w * v[4 * q + 3];
    }
  }
}

// out = layers.2.weight relu(layers.0.weight h); the weight addresses are wave-uniform
template <int K>
A3D_DEV void dg_mlp(const float* __restrict__ w, const float (&h)[DG_F], float (&out)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.f;
#pragma unroll 2
  for (int j = 0; j < DG_F; ++j) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < DG_F; ++i) a = fmaf(w[j * DG_F + i], h[i], a);
    a = fmaxf(a, 0.f);
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = fmaf(w[1024 + k * DG_F + j], a, out[k]);
  }
}

// ---- rotation chain: rot' = extract_rotation_torch(R build_rotation(q)), with what its derivative needs
struct DgRot {
  float qn[4], qinv, M[9], u[4], uinv, e[4], it;
  int branch;
};

A3D_DEV void dg_rot_fwd(const float (&q)[4], const float* __restrict__ R, DgRot& o) {
  o.qinv = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) o.qn[i] = q[i] * o.qinv;
  const float r = o.qn[0], x = o.qn[1], y = o.qn[2], z = o.qn[3];
  o.M[0] = 1.f - 2.f * (y * y + z * z); o.M[1] = 2.f * (x * y - r * z); o.M[2] = 2.f * (x * z + r * y);
  o.M[3] = 2.f * (x * y + r * z); o.M[4] = 1.f - 2.f * (x * x + z * z); o.M[5] = 2.f * (y * z - r * x);
  o.M[6] = 2.f * (x * z - r * y); o.M[7] = 2.f * (y * z + r * x); o.M[8] = 1.f - 2.f * (x * x + y * y);
  float A[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = R[i * 3 + 0] * o.M[j] + R[i * 3 + 1] * o.M[3 + j] + R[i * 3 + 2] * o.M[6 + j];
  const float tr = A[0] + A[4] + A[8];
  float tt;
  if (tr > 0.f) {
    o.branch = 0; tt = sqrtf(tr + 1.f) * 2.f; o.it = 1.f / tt;
    o.u[0] = 0.25f * tt; o.u[1] = (A[7] - A[5]) * o.it; o.u[2] = (A[2] - A[6]) * o.it; o.u[3] = (A[3] - A[1]) * o.it;
  } else if (A[0] > A[4] && A[0] > A[8]) {
    o.branch = 1; tt = sqrtf(1.f + A[0] - A[4] - A[8]) * 2.f; o.it = 1.f / tt;
    o.u[0] = (A[7] - A[5]) * o.it; o.u[1] = 0.25f * tt; o.u[2] = (A[1] + A[3]) * o.it; o.u[3] = (A[2] + A[6]) * o.it;
  } else if (A[4] > A[8]) {
    o.branch = 2; tt = sqrtf(1.f + A[4] - A[0] - A[8]) * 2.f; o.it = 1.f / tt;
    o.u[0] = (A[2] - A[6]) * o.it; o.u[1] = (A[1] + A[3]) * o.it; o.u[2] = 0.25f * tt; o.u[3] = (A[5] + A[7]) * o.it;
  } else {
    o.branch = 3; tt = sqrtf(1.f + A[8] - A[0] - A[4]) * 2.f; o.it = 1.f / tt;
    o.u[0] = (A[3] - A[1]) * o.it; o.u[1] = (A[2] + A[6]) * o.it; o.u[2] = (A[5] + A[7]) * o.it; o.u[3] = 0.25f * tt;
  }
  o.uinv = 1.f / sqrtf(o.u[0] * o.u[0] + o.u[1] * o.u[1] + o.u[2] * o.u[2] + o.u[3] * o.u[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) o.e[i] = o.u[i] * o.uinv;
}

// de: cotangent of rot'.  dq: cotangent of the raw quaternion; dR += cotangent of the global rotation
A3D_DEV void dg_rot_bwd(const DgRot& o, const float* __restrict__ R, const float (&de)[4], float (&dq)[4], float (&dR)[9]) {
  const float ed = o.e[0] * de[0] + o.e[1] * de[1] + o.e[2] * de[2] + o.e[3] * de[3];
  float du[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) du[i] = (de[i] - o.e[i] * ed) * o.uinv;
  float dA[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float it = o.it;
  float dtt, darg;
#define DG_OFF(c, ia, ib, sg) { const float g = du[c] * it; dA[ia] += g; dA[ib] += (sg) * g; dtt -= o.u[c] * g; }
  if (o.branch == 0) {
    dtt = 0.25f * du[0];
    DG_OFF(1, 7, 5, -1.f) DG_OFF(2, 2, 6, -1.f) DG_OFF(3, 3, 1, -1.f)
    darg = dtt * 2.f * it; dA[0] += darg; dA[4] += darg; dA[8] += darg;
  } else if (o.branch == 1) {
    dtt = 0.25f * du[1];
    DG_OFF(0, 7, 5, -1.f) DG_OFF(2, 1, 3, 1.f) DG_OFF(3, 2, 6, 1.f)
    darg = dtt * 2.f * it; dA[0] += darg; dA[4] -= darg; dA[8] -= darg;
  } else if (o.branch == 2) {
    dtt = 0.25f * du[2];
    DG_OFF(0, 2, 6, -1.f) DG_OFF(1, 1, 3, 1.f) DG_OFF(3, 5, 7, 1.f)
    darg = dtt * 2.f * it; dA[0] -= darg; dA[4] += darg; dA[8] -= darg;
  } else {
    dtt = 0.25f * du[3];
    DG_OFF(0, 3, 1, -1.f) DG_OFF(1, 2, 6, 1.f) DG_OFF(2, 5, 7, 1.f)
    darg = dtt * 2.f * it; dA[0] -= darg; dA[4] -= darg; dA[8] += darg;
  }
#undef DG_OFF
  float dM[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      dM[i * 3 + j] = R[0 + i] * dA[j] + R[3 + i] * dA[3 + j] + R[6 + i] * dA[6 + j];                       // R^T dA
      dR[i * 3 + j] += dA[i * 3 + 0] * o.M[j * 3 + 0] + dA[i * 3 + 1] * o.M[j * 3 + 1] + dA[i * 3 + 2] * o.M[j * 3 + 2];   // dA M^T
    }
  const float r = o.qn[0], x = o.qn[1], y = o.qn[2], z = o.qn[3];
  float dn[4];
  dn[0] = 2.f * (-z * dM[1] + y * dM[2] + z * dM[3] - x * dM[5] - y * dM[6] + x * dM[7]);
  dn[1] = 2.f * (y * dM[1] + z * dM[2] + y * dM[3] - r * dM[5] + z * dM[6] + r * dM[7]) - 4.f * x * (dM[4] + dM[8]);
  dn[2] = 2.f * (x * dM[1] + r * dM[2] + x * dM[3] + z * dM[5] - r * dM[6] + z * dM[7]) - 4.f * y * (dM[0] + dM[8]);
  dn[3] = 2.f * (-r * dM[1] + x * dM[2] + r * dM[3] + y * dM[5] + x * dM[6] + y * dM[7]) - 4.f * z * (dM[0] + dM[4]);
  const float nd = o.qn[0] * dn[0] + o.qn[1] * dn[1] + o.qn[2] * dn[2] + o.qn[3] * dn[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) dq[i] = (dn[i] - o.qn[i] * nd) * o.qinv;
}

// rotations = normalize(base + delta) (F.normalize, eps 1e-12); returns 1 / norm
A3D_DEV float dg_normalize(const float (&base)[4], const float (&delta)[4], float (&out)[4]) {
  float p[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = base[i] + delta[i];
  const float inv = 1.f / fmaxf(sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]), 1e-12f);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = p[i] * inv;
  return inv;
}

A3D_DEV void dg_normalize_bwd(const float (&out)[4], float inv, const float (&d)[4], float (&dp)[4]) {
  const float od = out[0] * d[0] + out[1] * d[1] + out[2] * d[2] + out[3] * d[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) dp[i] = (d[i] - out[i] * od) * inv;
}

// cotangent of one output of frame f at Gaussian n: the sum over the frame's images in ascending image order
template <int K>
A3D_DEV void dg_sum_images(const DgArgs& a, const float* __restrict__ g, int f, int n, float (&out)[K]) {
  const int e0 = a.img_start[f], e1 = a.img_start[f + 1];
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.f;
  for (int e = e0; e < e1; ++e) {
    const float* src = g + ((int64_t)a.img_list[e] * a.N + n) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = (e == e0) ? src[k] : out[k] + src[k];
  }
}

// ---------------------------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(DG_BLOCK) void dg_cells_kernel(int N, const float* __restrict__ xyz, DgPlanes P, int* __restrict__ cells) {
  const int n = blockIdx.x * DG_BLOCK + threadIdx.x;
  if (n >= N) return;
  const float p[3] = {xyz[n * 3 + 0], xyz[n * 3 + 1], xyz[n * 3 + 2]};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int k = 6 * s;
    cells[(int64_t)(k + 0) * N + n] = dg_lerp(p[1], P.H[k + 0]).i0 * (P.W[k + 0] - 1) + dg_lerp(p[0], P.W[k + 0]).i0;
    cells[(int64_t)(k + 1) * N + n] = dg_lerp(p[2], P.H[k + 1]).i0 * (P.W[k + 1] - 1) + dg_lerp(p[0], P.W[k + 1]).i0;
    cells[(int64_t)(k + 3) * N + n] = dg_lerp(p[2], P.H[k + 3]).i0 * (P.W[k + 3] - 1) + dg_lerp(p[1], P.W[k + 3]).i0;
    cells[(int64_t)(k + 2) * N + n] = dg_lerp(p[0], P.W[k + 2]).i0;
    cells[(int64_t)(k + 4) * N + n] = dg_lerp(p[1], P.W[k + 4]).i0;
    cells[(int64_t)(k + 5) * N + n] = dg_lerp(p[2], P.W[k + 5]).i0;
  }
}

__global__ __launch_bounds__(DG_BLOCK) void dg_spatial_kernel(int N, const float* __restrict__ xyz, const float* __restrict__ grid, DgPlanes P,
                                                              float* __restrict__ sp) {
  const int n = blockIdx.x * DG_BLOCK + threadIdx.x;
  if (n >= N) return;
  const float x = xyz[n * 3 + 0], y = xyz[n * 3 + 1], z = xyz[n * 3 + 2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float v[DG_C];
    dg_spatial_prod(grid, P, s, x, y, z, v);
    float4* dst = reinterpret_cast<float4*>(sp + (int64_t)n * DG_F + s * DG_C);
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  }
}

// mpart [T, chunks, 32]: sum of hidden over the block's Gaussians in index order
__global__ __launch_bounds__(DG_BLOCK) void dg_mean_partial_kernel(DgArgs a, const float* __restrict__ sp, float* __restrict__ mpart) {
  __shared__ float tile[DG_BLOCK * DG_LD];
  const int f = blockIdx.y, n = blockIdx.x * DG_BLOCK + threadIdx.x;
  const float t = a.ts[f];
  if (dg_bypass(a, t)) return;
  float h[DG_F];
  if (n < a.N) {
    dg_hidden(a, sp, n, a.xyz[n * 3 + 0], a.xyz[n * 3 + 1], a.xyz[n * 3 + 2], t, h);
  } else {
#pragma unroll
    for (int i = 0; i < DG_F; ++i) h[i] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < DG_F; ++i) tile[threadIdx.x * DG_LD + i] = h[i];
  __syncthreads();
  if (threadIdx.x < DG_F) {
    float s = 0.f;
    for (int r = 0; r < DG_BLOCK; ++r) s += tile[r * DG_LD + threadIdx.x];
    mpart[((int64_t)f * gridDim.x + blockIdx.x) * DG_F + threadIdx.x] = s;
  }
}

A3D_DEV void dg_mat3(const float* A, const float* B, float* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// 32 threads per frame; thread j owns neuron j of both global networks.  sig[0..2]: rotation sigmoids, sig[3..5]: translation sigmoids
A3D_DEV void dg_global_nets(const float* __restrict__ w, const float* g_lds, float* act_lds /*[2][32]*/, float (&pre)[2], float (&sig)[6]) {
  const int j = threadIdx.x;
#pragma unroll
  for (int net = 0; net < 2; ++net) {
    const float* w0 = w + (3 + net) * DG_NETW;
    float a = 0.f;
    for (int i = 0; i < DG_F; ++i) a = fmaf(w0[j * DG_F + i], g_lds[i], a);
    pre[net] = a;
    act_lds[net * DG_F + j] = fmaxf(a, 0.f);
  }
  __syncthreads();
#pragma unroll
  for (int net = 0; net < 2; ++net) {
    const float* w2 = w + (3 + net) * DG_NETW + 1024;
    for (int k = 0; k < 3; ++k) {
      float o = 0.f;
      for (int jj = 0; jj < DG_F; ++jj) o = fmaf(w2[k * DG_F + jj], act_lds[net * DG_F + jj], o);
      sig[net * 3 + k] = 1.f / (1.f + expf(-o));
    }
  }
}

struct DgEuler { float Rx[9], Ry[9], Rz[9]; };
A3D_DEV void dg_euler(const float (&sig)[6], DgEuler& E) {
  const float PI = 3.14159265358979323846f;
  const float roll = sig[0] * 2.f * PI - PI, pitch = sig[1] * 2.f * PI - PI, yaw = sig[2] * 2.f * PI - PI;
  const float cr = cosf(roll), sr = sinf(roll), cp = cosf(pitch), sp = sinf(pitch), cy = cosf(yaw), sy = sinf(yaw);
  const float rx[9] = {1.f, 0.f, 0.f, 0.f, cr, -sr, 0.f, sr, cr};
  const float ry[9] = {cp, 0.f, sp, 0.f, 1.f, 0.f, -sp, 0.f, cp};
  const float rz[9] = {cy, -sy, 0.f, sy, cy, 0.f, 0.f, 0.f, 1.f};
  for (int i = 0; i < 9; ++i) { E.Rx[i] = rx[i]; E.Ry[i] = ry[i]; E.Rz[i] = rz[i]; }
}

// gmean [T, 32], glob [T, 12] = R (row-major) | trans
__global__ __launch_bounds__(DG_F) void dg_frame_kernel(DgArgs a, const float* __restrict__ mpart, int chunks, float* __restrict__ gmean,
                                                        float* __restrict__ glob) {
  __shared__ float g[DG_F], act[2 * DG_F];
  const int f = blockIdx.x, j = threadIdx.x;
  if (dg_bypass(a, a.ts[f])) return;
  float s = 0.f;
  for (int b = 0; b < chunks; ++b) s += mpart[((int64_t)f * chunks + b) * DG_F + j];
  s = s / (float)a.N;
  g[j] = s;
  gmean[f * DG_F + j] = s;
  __syncthreads();
  float pre[2], sig[6];
  dg_global_nets(a.w, g, act, pre, sig);
  if (j == 0) {
    DgEuler E;
    dg_euler(sig, E);
    float yx[9], R[9];
    dg_mat3(E.Ry, E.Rx, yx);
    dg_mat3(E.Rz, yx, R);
    for (int i = 0; i < 9; ++i) glob[f * 12 + i] = R[i];
    for (int k = 0; k < 3; ++k) glob[f * 12 + 9 + k] = sig[3 + k] * 2.f - 1.f;
  }
}

__global__ __launch_bounds__(DG_BLOCK) void dg_deform_kernel(DgArgs a, const float* __restrict__ sp, const float* __restrict__ glob,
                                                             float* __restrict__ means, float* __restrict__ scales, float* __restrict__ rots) {
  const int f = blockIdx.y, n = blockIdx.x * DG_BLOCK + threadIdx.x;
  if (n >= a.N) return;
  const float t = a.ts[f];
  const float x = a.xyz[n * 3 + 0], y = a.xyz[n * 3 + 1], z = a.xyz[n * 3 + 2];
  const float sc[3] = {a.scaling[n * 3 + 0], a.scaling[n * 3 + 1], a.scaling[n * 3 + 2]};
  const float q[4] = {a.rotation[n * 4 + 0], a.rotation[n * 4 + 1], a.rotation[n * 4 + 2], a.rotation[n * 4 + 3]};
  float m[3] = {x, y, z}, so[3], ro[4];
  const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
  if (dg_bypass(a, t)) {
#pragma unroll
    for (int k = 0; k < 3; ++k) so[k] = expf(sc[k]);
    dg_normalize(q, zero4, ro);
  } else {
    float h[DG_F];
    dg_hidden(a, sp, n, x, y, z, t, h);
    float dx[3], dr[4], ds[3] = {0.f, 0.f, 0.f};
    dg_mlp<3>(a.w, h, dx);
    dg_mlp<4>(a.w + DG_NETW, h, dr);
    if (a.flags & 2) dg_mlp<3>(a.w + 2 * DG_NETW, h, ds);
    if (a.flags & 1) {
      const float* R = glob + f * 12;
      m[0] = R[0] * x + R[1] * y + R[2] * z + R[9];
      m[1] = R[3] * x + R[4] * y + R[5] * z + R[10];
      m[2] = R[6] * x + R[7] * y + R[8] * z + R[11];
      DgRot rc;
      dg_rot_fwd(q, R, rc);
      dg_normalize(rc.e, dr, ro);
    } else {
      dg_normalize(q, dr, ro);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { m[k] += dx[k]; so[k] = expf(sc[k] + ds[k]); }
  }
  for (int e = a.img_start[f]; e < a.img_start[f + 1]; ++e) {
    const int64_t row = (int64_t)a.img_list[e] * a.N + n;
#pragma unroll
    for (int k = 0; k < 3; ++k) { means[row * 3 + k] = m[k]; scales[row * 3 + k] = so[k]; }
    *reinterpret_cast<float4*>(rots + row * 4) = make_float4(ro[0], ro[1], ro[2], ro[3]);
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// gpart [T, chunks, 12]: block sums, in index order, of the cotangents of R (9) and trans (3)
__global__ __launch_bounds__(DG_BLOCK) void dg_bwd_global_partial_kernel(DgArgs a, const float* __restrict__ sp, const float* __restrict__ glob,
                                                                         const float* __restrict__ d_means, const float* __restrict__ d_rots,
                                                                         float* __restrict__ gpart) {
  __shared__ float tile[DG_BLOCK * 13];
  const int f = blockIdx.y, n = blockIdx.x * DG_BLOCK + threadIdx.x;
  const float t = a.ts[f];
  if (dg_bypass(a, t)) return;
  float dR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dt[3] = {0.f, 0.f, 0.f};
  if (n < a.N) {
    const float x = a.xyz[n * 3 + 0], y = a.xyz[n * 3 + 1], z = a.xyz[n * 3 + 2];
    const float q[4] = {a.rotation[n * 4 + 0], a.rotation[n * 4 + 1], a.rotation[n * 4 + 2], a.rotation[n * 4 + 3]};
    const float* R = glob + f * 12;
    float h[DG_F], dr[4], ro[4], dm[3], dro[4], dp[4], dq[4];
    dg_hidden(a, sp, n, x, y, z, t, h);
    dg_mlp<4>(a.w + DG_NETW, h, dr);
    DgRot rc;
    dg_rot_fwd(q, R, rc);
    const float inv = dg_normalize(rc.e, dr, ro);
    dg_sum_images<3>(a, d_means, f, n, dm);
    dg_sum_images<4>(a, d_rots, f, n, dro);
    dg_normalize_bwd(ro, inv, dro, dp);
    dg_rot_bwd(rc, R, dp, dq, dR);
    const float p[3] = {x, y, z};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      dt[i] = dm[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) dR[i * 3 + k] += dm[i] * p[k];
    }
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) tile[threadIdx.x * 13 + i] = dR[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) tile[threadIdx.x * 13 + 9 + i] = dt[i];
  __syncthreads();
  if (threadIdx.x < 12) {
    float s = 0.f;
    for (int r = 0; r < DG_BLOCK; ++r) s += tile[r * 13 + threadIdx.x];
    gpart[((int64_t)f * gridDim.x + blockIdx.x) * 12 + threadIdx.x] = s;
  }
}

// per frame: dgm [T, 32] = cotangent of the mean feature / N; wf [T, 5 * 1152] slots 3, 4 = the frame's global weight gradients
__global__ __launch_bounds__(DG_F) void dg_bwd_frame_kernel(DgArgs a, const float* __restrict__ gpart, int chunks, const float* __restrict__ gmean,
                                                            float* __restrict__ dgm, float* __restrict__ wf) {
  __shared__ float g[DG_F], act[2 * DG_F], red[12], dpre_l[2 * DG_F];
  const int f = blockIdx.x, j = threadIdx.x;
  float* wout = wf + (int64_t)f * 5 * DG_NETW + 3 * DG_NETW;
  if (dg_bypass(a, a.ts[f])) {
    for (int i = j; i < 2 * DG_NETW; i += DG_F) wout[i] = 0.f;
    dgm[f * DG_F + j] = 0.f;
    return;
  }
  if (j < 12) {
    float s = 0.f;
    for (int b = 0; b < chunks; ++b) s += gpart[((int64_t)f * chunks + b) * 12 + j];
    red[j] = s;
  }
  g[j] = gmean[f * DG_F + j];
  __syncthreads();
  float pre[2], sig[6];
  dg_global_nets(a.w, g, act, pre, sig);
  // cotangents of the six pre-sigmoid outputs
  DgEuler E;
  dg_euler(sig, E);
  const float PI = 3.14159265358979323846f;
  const float cr = E.Rx[4], sr = E.Rx[7], cp = E.Ry[0], sp = E.Ry[2], cy = E.Rz[0], sy = E.Rz[3];
  const float dRx[9] = {0.f, 0.f, 0.f, 0.f, -sr, -cr, 0.f, cr, -sr};
  const float dRy[9] = {-sp, 0.f, cp, 0.f, 0.f, 0.f, -cp, 0.f, -sp};
  const float dRz[9] = {-sy, -cy, 0.f, cy, -sy, 0.f, 0.f, 0.f, 0.f};
  float tmp[9], D[9], dout[6];
  dg_mat3(E.Ry, dRx, tmp); dg_mat3(E.Rz, tmp, D);
  dout[0] = 0.f; for (int i = 0; i < 9; ++i) dout[0] += red[i] * D[i];
  dg_mat3(dRy, E.Rx, tmp); dg_mat3(E.Rz, tmp, D);
  dout[1] = 0.f; for (int i = 0; i < 9; ++i) dout[1] += red[i] * D[i];
  dg_mat3(E.Ry, E.Rx, tmp); dg_mat3(dRz, tmp, D);
  dout[2] = 0.f; for (int i = 0; i < 9; ++i) dout[2] += red[i] * D[i];
  for (int k = 0; k < 3; ++k) {
    dout[k] *= 2.f * PI * sig[k] * (1.f - sig[k]);
    dout[3 + k] = red[9 + k] * 2.f * sig[3 + k] * (1.f - sig[3 + k]);
  }
  for (int net = 0; net < 2; ++net) {
    const float* w2 = a.w + (3 + net) * DG_NETW + 1024;
    float* wo = wout + net * DG_NETW;
    float da = 0.f;
    for (int k = 0; k < 3; ++k) {
      da = fmaf(w2[k * DG_F + j], dout[net * 3 + k], da);
      wo[1024 + k * DG_F + j] = dout[net * 3 + k] * act[net * DG_F + j];
    }
    wo[1024 + 3 * DG_F + j] = 0.f;
    const float dp = pre[net] > 0.f ? da : 0.f;
    dpre_l[net * DG_F + j] = dp;
    for (int i = 0; i < DG_F; ++i) wo[j * DG_F + i] = dp * g[i];
  }
  __syncthreads();
  float dg = 0.f;
  for (int net = 0; net < 2; ++net) {
    const float* w0 = a.w + (3 + net) * DG_NETW;
    for (int jj = 0; jj < DG_F; ++jj) dg = fmaf(w0[jj * DG_F + j], dpre_l[net * DG_F + jj], dg);
  }
  dgm[f * DG_F + j] = dg / (float)a.N;
}

// One network of the main backward for a tile of 128 rows.  Forward half: activations of the thread's row into its LDS row, outputs returned.
template <int K>
A3D_DEV void dg_net_fwd_tile(const float* __restrict__ w, const float (&h)[DG_F], bool valid, float* row, float (&out)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.f;
#pragma unroll 2
  for (int j = 0; j < DG_F; ++j) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < DG_F; ++i) a = fmaf(w[j * DG_F + i], h[i], a);
    a = valid ? fmaxf(a, 0.f) : 0.f;
    row[j] = a;
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = fmaf(w[1024 + k * DG_F + j], a, out[k]);
  }
}

// Backward half (dpre of the row into a second LDS tile): dh += W0^T dpre; acc2 (thread = entry k * 32 + j of layers.2.weight) and acc0 (thread = row tid >> 2, columns (tid & 3) * 8 ..
// + 7 of layers.0.weight) accumulate the tile's outer products over its rows in row order.
template <int K>
A3D_DEV void dg_net_bwd_tile(const float* __restrict__ w, const float (&dout)[K], bool valid, float (&dh)[DG_F], const float* buf, float* dbuf,
                             const float* hb, float* dob, float (&acc0)[8], float& acc2) {
  const int tid = threadIdx.x;
  const float* row = buf + tid * DG_LD;
  float* drow = dbuf + tid * DG_LD;
#pragma unroll
  for (int k = 0; k < 4; ++k) dob[tid * 4 + k] = (k < K && valid) ? dout[k < K ? k : 0] : 0.f;
#pragma unroll 2
  for (int j = 0; j < DG_F; ++j) {
    float da = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) da = fmaf(w[1024 + k * DG_F + j], dout[k], da);
    const float dp = row[j] > 0.f ? da : 0.f;          // the row holds relu(pre), zero for a row past N
    drow[j] = dp;
#pragma unroll
    for (int i = 0; i < DG_F; ++i) dh[i] = fmaf(w[j * DG_F + i], dp, dh[i]);
  }
  __syncthreads();
  {
    const int k = tid >> 5, j = tid & 31;
    float s = acc2;
    for (int r = 0; r < DG_BWD_BLOCK; ++r) s = fmaf(dob[r * 4 + k], buf[r * DG_LD + j], s);
    acc2 = s;
  }
  {
    const int j = tid >> 2, i0 = (tid & 3) * 8;
    for (int r = 0; r < DG_BWD_BLOCK; ++r) {
      const float d = dbuf[r * DG_LD + j];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc0[q] = fmaf(d, hb[r * DG_LD + i0 + q], acc0[q]);
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(DG_BWD_BLOCK) void dg_bwd_kernel(DgArgs a, const float* __restrict__ sp, const float* __restrict__ glob,
                                                              const float* __restrict__ dgm, const float* __restrict__ d_means,
                                                              const float* __restrict__ d_scales, const float* __restrict__ d_rots,
                                                              float* __restrict__ dh_out, float* __restrict__ dsc_f, float* __restrict__ drot_f,
                                                              float* __restrict__ wpart) {
  __shared__ float hb[DG_BWD_BLOCK * DG_LD], buf[DG_BWD_BLOCK * DG_LD], dbuf[DG_BWD_BLOCK * DG_LD], dob[DG_BWD_BLOCK * 4];
  const int f = blockIdx.y, tid = threadIdx.x;
  const float t = a.ts[f];
  const bool bypass = dg_bypass(a, t);
  const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
  float acc0[3][8], acc2[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc0[i][q] = 0.f;
#pragma unroll 1
  for (int sub = 0; sub < DG_BWD_SUB; ++sub) {
    const int n = (blockIdx.x * DG_BWD_SUB + sub) * DG_BWD_BLOCK + tid;
    const bool valid = n < a.N;
    float x = 0.f, y = 0.f, z = 0.f, sc[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f};
    float dm[3] = {0.f, 0.f, 0.f}, dso[3] = {0.f, 0.f, 0.f}, dro[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
      x = a.xyz[n * 3 + 0]; y = a.xyz[n * 3 + 1]; z = a.xyz[n * 3 + 2];
#pragma unroll
      for (int k = 0; k < 3; ++k) sc[k] = a.scaling[n * 3 + k];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = a.rotation[n * 4 + k];
      dg_sum_images<3>(a, d_means, f, n, dm);
      dg_sum_images<3>(a, d_scales, f, n, dso);
      dg_sum_images<4>(a, d_rots, f, n, dro);
    }
    const int64_t row_fn = (int64_t)f * a.N + n;
    if (bypass) {                                                   // first frame: means = xyz, scales = exp(scaling), rotations = normalize(rotation)
      if (valid) {
        float ro[4], dq[4];
        const float inv = dg_normalize(q, zero4, ro);
        dg_normalize_bwd(ro, inv, dro, dq);
#pragma unroll
        for (int k = 0; k < 3; ++k) dsc_f[row_fn * 3 + k] = dso[k] * expf(sc[k]);
        *reinterpret_cast<float4*>(drot_f + row_fn * 4) = make_float4(dq[0], dq[1], dq[2], dq[3]);
      }
      continue;
    }
    float h[DG_F], dh[DG_F];
#pragma unroll
    for (int i = 0; i < DG_F; ++i) { h[i] = 0.f; dh[i] = 0.f; }
    if (valid) dg_hidden(a, sp, n, x, y, z, t, h);
#pragma unroll
    for (int i = 0; i < DG_F; ++i) hb[tid * DG_LD + i] = h[i];
    float* row = buf + tid * DG_LD;
    // delta_xyz: means = xyz' + out
    {
      float out[3];
      dg_net_fwd_tile<3>(a.w, h, valid, row, out);
      dg_net_bwd_tile<3>(a.w, dm, valid, dh, buf, dbuf, hb, dob, acc0[0], acc2[0]);
    }
    // delta_rot: rotations = normalize(rot' + out)
    {
      float out[4], ro[4], dp[4], dq[4], dR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      dg_net_fwd_tile<4>(a.w + DG_NETW, h, valid, row, out);
      if (a.flags & 1) {
        const float* R = glob + f * 12;
        DgRot rc;
        dg_rot_fwd(q, R, rc);
        const float inv = dg_normalize(rc.e, out, ro);
        dg_normalize_bwd(ro, inv, dro, dp);
        dg_rot_bwd(rc, R, dp, dq, dR);
      } else {
        const float inv = dg_normalize(q, out, ro);
        dg_normalize_bwd(ro, inv, dro, dp);
#pragma unroll
        for (int k = 0; k < 4; ++k) dq[k] = dp[k];
      }
      if (valid) *reinterpret_cast<float4*>(drot_f + row_fn * 4) = make_float4(dq[0], dq[1], dq[2], dq[3]);
      dg_net_bwd_tile<4>(a.w + DG_NETW, dp, valid, dh, buf, dbuf, hb, dob, acc0[1], acc2[1]);
    }
    // delta_scaling: scales = exp(scaling + out)
    if (a.flags & 2) {
      float out[3], dp[3];
      dg_net_fwd_tile<3>(a.w + 2 * DG_NETW, h, valid, row, out);
#pragma unroll
      for (int k = 0; k < 3; ++k) dp[k] = dso[k] * expf(sc[k] + out[k]);
      if (valid) {
#pragma unroll
        for (int k = 0; k < 3; ++k) dsc_f[row_fn * 3 + k] = dp[k];
      }
      dg_net_bwd_tile<3>(a.w + 2 * DG_NETW, dp, valid, dh, buf, dbuf, hb, dob, acc0[2], acc2[2]);
    } else if (valid) {
#pragma unroll
      for (int k = 0; k < 3; ++k) dsc_f[row_fn * 3 + k] = dso[k] * expf(sc[k]);
    }
    if (valid) {
      if (a.flags & 1) {
#pragma unroll
        for (int i = 0; i < DG_F; ++i) dh[i] += dgm[f * DG_F + i];
      }
      float4* dst = reinterpret_cast<float4*>(dh_out + row_fn * DG_F);
#pragma unroll
      for (int v = 0; v < 8; ++v) dst[v] = make_float4(dh[4 * v], dh[4 * v + 1], dh[4 * v + 2], dh[4 * v + 3]);
    }
  }
  if (bypass) return;
  float* slab = wpart + ((int64_t)f * gridDim.x + blockIdx.x) * 3 * DG_NETW;
#pragma unroll
  for (int net = 0; net < 3; ++net) {
    const int j = tid >> 2, i0 = (tid & 3) * 8;
#pragma unroll
    for (int v = 0; v < 8; ++v) slab[net * DG_NETW + j * DG_F + i0 + v] = acc0[net][v];
    slab[net * DG_NETW + 1024 + tid] = acc2[net];
  }
}

// wf [T, 5 * 1152] slots 0 .. 2: the frame's slabs in block order
__global__ __launch_bounds__(DG_BLOCK) void dg_wreduce_kernel(DgArgs a, const float* __restrict__ wpart, int nblk, float* __restrict__ wf) {
  const int e = blockIdx.x * DG_BLOCK + threadIdx.x, f = blockIdx.y;
  if (e >= 3 * DG_NETW) return;
  float s = 0.f;
  if (!dg_bypass(a, a.ts[f]))
    for (int b = 0; b < nblk; ++b) s += wpart[((int64_t)f * nblk + b) * 3 * DG_NETW + e];
  wf[(int64_t)f * 5 * DG_NETW + e] = s;
}

// dspat [N, 3, 32]: cotangent of the sample of spatial plane (x,y) / (x,z) / (y,z), both scales
__global__ __launch_bounds__(DG_BLOCK) void dg_bwd_spatial_kernel(DgArgs a, const float* __restrict__ dh, float* __restrict__ dspat) {
  const int n = blockIdx.x * DG_BLOCK + threadIdx.x;
  if (n >= a.N) return;
  const float x = a.xyz[n * 3 + 0], y = a.xyz[n * 3 + 1], z = a.xyz[n * 3 + 2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float d[DG_C];
#pragma unroll
    for (int c = 0; c < DG_C; ++c) d[c] = 0.f;
    for (int f = 0; f < a.T; ++f) {
      const float t = a.ts[f];
      if (dg_bypass(a, t)) continue;
      float v[DG_C];
      dg_time_prod(a.grid, a.P, s, x, y, z, t, v);
      const float4* src = reinterpret_cast<const float4*>(dh + ((int64_t)f * a.N + n) * DG_F + s * DG_C);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 g = src[q];
        d[4 * q + 0] = fmaf(g.x, v[4 * q + 0], d[4 * q + 0]); d[4 * q + 1] = fmaf(g.y, v[4 * q + 1], d[4 * q + 1]);
        d[4 * q + 2] = fmaf(g.z, v[4 * q + 2], d[4 * q + 2]); d[4 * q + 3] = fmaf(g.w, v[4 * q + 3], d[4 * q + 3]);
      }
    }
    const int k = 6 * s;
    float pa[DG_C], pb[DG_C], pc[DG_C];
#pragma unroll
    for (int c = 0; c < DG_C; ++c) pa[c] = pb[c] = pc[c] = 1.f;
    dg_sample_mul(a.grid, a.P, k + 0, dg_lerp(x, a.P.W[k + 0]), dg_lerp(y, a.P.H[k + 0]), pa);
    dg_sample_mul(a.grid, a.P, k + 1, dg_lerp(x, a.P.W[k + 1]), dg_lerp(z, a.P.H[k + 1]), pb);
    dg_sample_mul(a.grid, a.P, k + 3, dg_lerp(y, a.P.W[k + 3]), dg_lerp(z, a.P.H[k + 3]), pc);
    float* dst = dspat + (int64_t)n * 3 * DG_F + s * DG_C;
#pragma unroll
    for (int c = 0; c < DG_C; ++c) {
      dst[c] = d[c] * pb[c] * pc[c];
      dst[DG_F + c] = d[c] * pa[c] * pc[c];
      dst[2 * DG_F + c] = d[c] * pa[c] * pb[c];
    }
  }
}

// the slices' partial sums, added in slice order by slice 0
template <int SLICES>
A3D_DEV float dg_slice_sum(float acc, float* red, int c, int slice, bool& owner) {
  red[slice * DG_C + c] = acc;
  __syncthreads();
  owner = slice == 0;
  float s = 0.f;
  if (owner)
    for (int i = 0; i < SLICES; ++i) s += red[i * DG_C + c];
  return s;
}

// spatial plane k (pair slot pi of 0 .. 2 over coordinates ca, cb): one block per texel
__global__ __launch_bounds__(DG_SLICES_S * DG_C) void dg_sgather_kernel(DgArgs a, int k, int pi, int ca, int cb, const float* __restrict__ dspat,
                                                                       const int* __restrict__ order, const int* __restrict__ starts,
                                                                       float* __restrict__ dgrid) {
  __shared__ float red[DG_SLICES_S * DG_C];
  const int W = a.P.W[k], H = a.P.H[k];
  const int ix = blockIdx.x % W, iy = blockIdx.x / W;
  const int c = threadIdx.x & 15, slice = threadIdx.x >> 4, s = k / 6;
  float acc = 0.f;
  for (int cy = max(iy - 1, 0); cy <= min(iy, H - 2); ++cy)
    for (int cx = max(ix - 1, 0); cx <= min(ix, W - 2); ++cx) {
      const int cell = cy * (W - 1) + cx;
      for (int e = starts[cell] + slice; e < starts[cell + 1]; e += DG_SLICES_S) {
        const int n = order[e];
        const DgLerp lx = dg_lerp(a.xyz[n * 3 + ca], W), ly = dg_lerp(a.xyz[n * 3 + cb], H);
        const float wgt = (cx == ix ? 1.f - lx.w1 : lx.w1) * (cy == iy ? 1.f - ly.w1 : ly.w1);
        acc = fmaf(wgt, dspat[((int64_t)n * 3 + pi) * DG_F + s * DG_C + c], acc);
      }
    }
  bool owner;
  const float sum = dg_slice_sum<DG_SLICES_S>(acc, red, c, slice, owner);
  if (owner) dgrid[a.P.off[k] + ((int64_t)iy * W + ix) * DG_C + c] = sum;
}

struct DgTime {
  int woff[7];                      // prefix sums of W over the six time planes (s = 0: x y z, s = 1: x y z)
  int64_t soff[DG_P];               // where plane k's segment starts begin in the plan
};

// rows [T, sumW, 16]: per frame and x-texel of every time plane, the cotangent before the t weight
__global__ __launch_bounds__(DG_SLICES_T * DG_C) void dg_tgather_kernel(DgArgs a, DgTime tw, const float* __restrict__ sp, const float* __restrict__ dh,
                                                                       const int* __restrict__ order, const int* __restrict__ starts_all,
                                                                       float* __restrict__ rows) {
  __shared__ float red[DG_SLICES_T * DG_C];
  const int f = blockIdx.y;
  const float t = a.ts[f];
  if (dg_bypass(a, t)) return;
  int pl = 0;
  while (pl < 5 && (int)blockIdx.x >= tw.woff[pl + 1]) ++pl;
  const int ix = blockIdx.x - tw.woff[pl], s = pl / 3, ax = pl % 3;
  const int k = 6 * s + (ax == 0 ? 2 : ax == 1 ? 4 : 5);
  const int W = a.P.W[k];
  const int* starts = starts_all + tw.soff[k];
  const int* ord = order + (int64_t)k * a.N;
  const int c = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int ka = 6 * s + 2, kb = 6 * s + 4, kc = 6 * s + 5;
  const DgLerp lta = dg_lerp(t, a.P.H[ka]), ltb = dg_lerp(t, a.P.H[kb]), ltc = dg_lerp(t, a.P.H[kc]);
  float acc = 0.f;
  for (int cx = max(ix - 1, 0); cx <= min(ix, W - 2); ++cx)
    for (int e = starts[cx] + slice; e < starts[cx + 1]; e += DG_SLICES_T) {
      const int n = ord[e];
      const float x = a.xyz[n * 3 + 0], y = a.xyz[n * 3 + 1], z = a.xyz[n * 3 + 2];
      const DgLerp lx = dg_lerp(ax == 0 ? x : ax == 1 ? y : z, W);
      float v = dh[((int64_t)f * a.N + n) * DG_F + s * DG_C + c] * sp[(int64_t)n * DG_F + s * DG_C + c];
      if (ax != 0) v *= dg_sample1(a.grid, a.P, ka, dg_lerp(x, a.P.W[ka]), lta, c);
      if (ax != 1) v *= dg_sample1(a.grid, a.P, kb, dg_lerp(y, a.P.W[kb]), ltb, c);
      if (ax != 2) v *= dg_sample1(a.grid, a.P, kc, dg_lerp(z, a.P.W[kc]), ltc, c);
      acc = fmaf(cx == ix ? 1.f - lx.w1 : lx.w1, v, acc);
    }
  bool owner;
  const float sum = dg_slice_sum<DG_SLICES_T>(acc, red, c, slice, owner);
  if (owner) rows[((int64_t)f * tw.woff[6] + blockIdx.x) * DG_C + c] = sum;
}

// time plane k: texel (it, ix) = sum over frames, in order, of the frame's row times its t weight
__global__ __launch_bounds__(DG_BLOCK) void dg_tcombine_kernel(DgArgs a, int k, int woff, int sumW, const float* __restrict__ rows,
                                                               float* __restrict__ dgrid) {
  const int W = a.P.W[k], H = a.P.H[k];
  const int idx = blockIdx.x * DG_BLOCK + threadIdx.x;
  if (idx >= W * H * DG_C) return;
  const int c = idx % DG_C, ix = (idx / DG_C) % W, it = idx / (DG_C * W);
  float s = 0.f;
  for (int f = 0; f < a.T; ++f) {
    const float t = a.ts[f];
    if (dg_bypass(a, t)) continue;
    const DgLerp lt = dg_lerp(t, H);
    if (it != lt.i0 && it != lt.i0 + 1) continue;
    s = fmaf(it == lt.i0 ? 1.f - lt.w1 : lt.w1, rows[((int64_t)f * sumW + woff + ix) * DG_C + c], s);
  }
  dgrid[a.P.off[k] + idx] = s;
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline int64_t dg_up4(int64_t v) { return (v + 3) & ~int64_t(3); }

bool dg_planes(const int64_t* desc, DgPlanes& P) {        // desc: host [36] = off[12] | W[12] | H[12]
  if (!desc) return false;
  for (int k = 0; k < DG_P; ++k) {
    P.off[k] = desc[k]; P.W[k] = (int)desc[12 + k]; P.H[k] = (int)desc[24 + k];
    if (desc[k] < 0 || (desc[k] & 15) || desc[12 + k] < 2 || desc[24 + k] < 2 || desc[12 + k] > 32768 || desc[24 + k] > 32768) return false;
  }
  return true;
}

struct DgWs { int64_t dh, dsc, drot, wpart, wf, gpart, dgm, dspat, rows, total; int chunks, nblk, sumW; };

DgWs dg_workspace(int T, int N, const DgPlanes& P) {
  DgWs w;
  w.chunks = (N + DG_BLOCK - 1) / DG_BLOCK;
  w.nblk = (N + DG_BWD_BLOCK * DG_BWD_SUB - 1) / (DG_BWD_BLOCK * DG_BWD_SUB);
  w.sumW = 0;
  for (int s = 0; s < 2; ++s)
    for (int p : {2, 4, 5}) w.sumW += P.W[6 * s + p];
  int64_t o = 0;
  w.dh = o;    o += dg_up4((int64_t)T * N * DG_F);
  w.dsc = o;   o += dg_up4((int64_t)T * N * 3);
  w.drot = o;  o += dg_up4((int64_t)T * N * 4);
  w.wpart = o; o += dg_up4((int64_t)T * w.nblk * 3 * DG_NETW);
  w.wf = o;    o += dg_up4((int64_t)T * 5 * DG_NETW);
  w.gpart = o; o += dg_up4((int64_t)T * w.chunks * 12);
  w.dgm = o;   o += dg_up4((int64_t)T * DG_F);
  w.dspat = o; o += dg_up4((int64_t)N * 3 * DG_F);
  w.rows = o;  o += dg_up4((int64_t)T * w.sumW * DG_C);
  w.total = o;
  return w;
}

bool dg_args(DgArgs& a, int T, int N, int B, const float* xyz, const float* scaling, const float* rotation, const float* ts, const float* grid,
             const int64_t* desc, const float* w, int flags, const int* img_start, const int* img_list) {
  if (T <= 0 || N <= 0 || B <= 0 || T > 65535 || (int64_t)T * N > 0x7fffffffLL / 4 || (int64_t)B * N > 0x7fffffffLL / 4) return false;
  if (!xyz || !scaling || !rotation || !ts || !grid || !w || !img_start || !img_list) return false;
  if (!a3d_aligned(16, grid, rotation) || !a3d_aligned(4, xyz, scaling, ts, w, img_start, img_list)) return false;
  if (!dg_planes(desc, a.P)) return false;
  a.T = T; a.N = N; a.B = B; a.flags = flags; a.xyz = xyz; a.scaling = scaling; a.rotation = rotation; a.ts = ts; a.grid = grid; a.w = w;
  a.img_start = img_start; a.img_list = img_list;
  return true;
}

}  // namespace

extern "C" int a3d_dg_cells_f32(a3d_stream_t stream, int N, const float* xyz, const int64_t* plane_desc, int* cells) {
  DgPlanes P;
  if (N <= 0 || !xyz || !cells || !a3d_aligned(4, xyz, cells) || !dg_planes(plane_desc, P)) return A3D_EINVAL;
  dg_cells_kernel<<<blocks_for(N, DG_BLOCK), DG_BLOCK, 0, (hipStream_t)stream>>>(N, xyz, P, cells);
  return a3d_launch_status();
}

extern "C" int64_t a3d_dg_mean_partials(int N) { return N <= 0 ? 0 : (N + DG_BLOCK - 1) / DG_BLOCK; }

extern "C" int a3d_dg_forward_f32(a3d_stream_t stream, int T, int N, int B, const float* xyz, const float* scaling, const float* rotation,
                                  const float* timestamps, const float* grid, const int64_t* plane_desc, const float* weights, int flags,
                                  const int* img_start, const int* img_list, float* sp, float* mpart, float* gmean, float* glob, float* means,
                                  float* scales, float* rots) {
  DgArgs a;
  if (!dg_args(a, T, N, B, xyz, scaling, rotation, timestamps, grid, plane_desc, weights, flags, img_start, img_list)) return A3D_EINVAL;
  if (!sp || !means || !scales || !rots || !a3d_aligned(16, sp, rots) || !a3d_aligned(4, means, scales, mpart, gmean, glob)) return A3D_EINVAL;
  if ((flags & 1) && (!mpart || !gmean || !glob)) return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (N + DG_BLOCK - 1) / DG_BLOCK;
  dg_spatial_kernel<<<chunks, DG_BLOCK, 0, st>>>(N, xyz, grid, a.P, sp);
  if (flags & 1) {
    dg_mean_partial_kernel<<<dim3(chunks, T), DG_BLOCK, 0, st>>>(a, sp, mpart);
    dg_frame_kernel<<<T, DG_F, 0, st>>>(a, mpart, chunks, gmean, glob);
  }
  dg_deform_kernel<<<dim3(chunks, T), DG_BLOCK, 0, st>>>(a, sp, glob, means, scales, rots);
  return a3d_launch_status();
}

extern "C" int64_t a3d_dg_backward_ws_floats(int T, int N, const int64_t* plane_desc) {
  DgPlanes P;
  if (T <= 0 || N <= 0 || !dg_planes(plane_desc, P)) return 0;
  return dg_workspace(T, N, P).total;
}

extern "C" int a3d_dg_backward_f32(a3d_stream_t stream, int T, int N, int B, const float* xyz, const float* scaling, const float* rotation,
                                   const float* timestamps, const float* grid, const int64_t* plane_desc, const float* weights, int flags,
                                   const int* img_start, const int* img_list, const float* sp, const float* gmean, const float* glob,
                                   const int* order, const int* starts, const float* d_means, const float* d_scales, const float* d_rots,
                                   float* ws, float* d_grid, float* d_weights, float* d_scaling, float* d_rotation) {
  DgArgs a;
  if (!dg_args(a, T, N, B, xyz, scaling, rotation, timestamps, grid, plane_desc, weights, flags, img_start, img_list)) return A3D_EINVAL;
  if (!sp || !order || !starts || !d_means || !d_scales || !d_rots || !ws || !d_grid || !d_weights || !d_scaling || !d_rotation) return A3D_EINVAL;
  if (!a3d_aligned(16, sp, ws, d_grid, d_rots, d_rotation) || ((flags & 1) && (!gmean || !glob))) return A3D_EINVAL;
  if (!a3d_aligned(4, order, starts, d_means, d_scales, d_weights, d_scaling, gmean, glob)) return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const DgWs w = dg_workspace(T, N, a.P);
  // plan offsets: starts of plane k begin at soff[k]; cells: (W - 1)(H - 1) for a spatial plane, W - 1 for a time plane
  DgTime tw;
  int64_t o = 0;
  for (int k = 0; k < DG_P; ++k) {
    const int p = k % 6;
    const bool time_plane = p == 2 || p == 4 || p == 5;
    tw.soff[k] = o;
    o += (time_plane ? (int64_t)(a.P.W[k] - 1) : (int64_t)(a.P.W[k] - 1) * (a.P.H[k] - 1)) + 1;
  }
  float *dh = ws + w.dh, *dsc = ws + w.dsc, *drot = ws + w.drot, *wpart = ws + w.wpart, *wf = ws + w.wf, *gpart = ws + w.gpart, *dgm = ws + w.dgm,
        *dspat = ws + w.dspat, *rows = ws + w.rows;
  if (flags & 1) {
    dg_bwd_global_partial_kernel<<<dim3(w.chunks, T), DG_BLOCK, 0, st>>>(a, sp, glob, d_means, d_rots, gpart);
    dg_bwd_frame_kernel<<<T, DG_F, 0, st>>>(a, gpart, w.chunks, gmean, dgm, wf);
  } else if (hipError_t e = hipMemsetAsync(wf, 0, (size_t)T * 5 * DG_NETW * sizeof(float), st); e != hipSuccess) {
    return (int)e;
  }
  dg_bwd_kernel<<<dim3(w.nblk, T), DG_BWD_BLOCK, 0, st>>>(a, sp, glob, dgm, d_means, d_scales, d_rots, dh, dsc, drot, wpart);
  dg_wreduce_kernel<<<dim3(blocks_for(3 * DG_NETW, DG_BLOCK), T), DG_BLOCK, 0, st>>>(a, wpart, w.nblk, wf);
  sum_leading(st, wf, d_weights, T, 5 * DG_NETW);
  sum_leading(st, dsc, d_scaling, T, (int64_t)N * 3);
  sum_leading(st, drot, d_rotation, T, (int64_t)N * 4);
  dg_bwd_spatial_kernel<<<w.chunks, DG_BLOCK, 0, st>>>(a, dh, dspat);
  tw.woff[0] = 0;
  for (int s = 0, i = 0; s < 2; ++s)
    for (int p : {2, 4, 5}) { tw.woff[i + 1] = tw.woff[i] + a.P.W[6 * s + p]; ++i; }
  dg_tgather_kernel<<<dim3(w.sumW, T), DG_SLICES_T * DG_C, 0, st>>>(a, tw, sp, dh, order, starts, rows);
  for (int s = 0, i = 0; s < 2; ++s)
    for (int p : {2, 4, 5}) {
      const int k = 6 * s + p;
      dg_tcombine_kernel<<<blocks_for((int64_t)a.P.W[k] * a.P.H[k] * DG_C, DG_BLOCK), DG_BLOCK, 0, st>>>(a, k, tw.woff[i], w.sumW, rows, d_grid);
      ++i;
    }
  for (int s = 0; s < 2; ++s) {
    const int slot[3] = {0, 1, 3}, ca[3] = {0, 0, 1}, cb[3] = {1, 2, 2};
    for (int pi = 0; pi < 3; ++pi) {
      const int k = 6 * s + slot[pi];
      dg_sgather_kernel<<<a.P.W[k] * a.P.H[k], DG_SLICES_S * DG_C, 0, st>>>(a, k, pi, ca[pi], cb[pi], dspat, order + (int64_t)k * N,
                                                                            starts + tw.soff[k], d_grid);
    }
  }
  return a3d_launch_status();
}
