// Differentiable 3-D Gaussian splat rasterizer (Kerbl et al. 2023, the forward of the published 3DGS rasterizer as the ashawkey fork of
// diff_gaussian_rasterization exposes it), fp32, batched over B cameras per launch.  The contract is written out in animate3d_amd/splat.py.
//
// Stages (every one launches once for all B images):
//   preprocess       one thread per (image, Gaussian): cull, 2-D covariance (EWA), conic, radius, pixel centre, depth, colour (SH), tile count
//   duplicate        one (key, value) per touched tile at the Gaussian's exclusive prefix-sum offset; key = (image * tiles + tile) << 32 | depth bits
//   (sort)           stable torch.sort of the keys on the host side (rocPRIM); its permutation maps sorted -> duplicated order
//   tile_ranges      [start, end) of every (image, tile) in the sorted keys
//   render           one 256-thread workgroup per (image, 16 x 16 tile), Gaussians staged through LDS in batches of 256, front to back
//   render_bwd       same tiling, back to front; each Gaussian's gradient is summed over the tile's 256 pixels on chip (DPP within rows of 16
//                    lanes, readlane across rows, LDS across the four waves) and stored as ONE row per instance, in duplicated order
//   preprocess_bwd   one thread per (image, Gaussian): sums its contiguous span of instance rows in a fixed order, chains to the inputs
//   sum_batch        inputs shared by all images ([N, ...]) get their gradient summed over B in a fixed order (f32_common.h: sum_leading)
// No atomics anywhere: gradients are bitwise reproducible.
//
// Only fp32 entry points: compiled out of the fp16-storage pass of build.py so they are exported once.
#include "f32_common.h"

namespace {

constexpr int GS_TILE = 16;
constexpr int GS_BLOCK = GS_TILE * GS_TILE;      // 256 threads, four wave64
constexpr int GS_ROW = 12;                       // floats per instance gradient row: centre(2) conic(3) opacity colour(3) depth, pad(2)

constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
__constant__ float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
__constant__ float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                               -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};

struct GsInputs {
  const float* means;  int64_t means_bs;        // [*, N, 3]; *_bs: elements between images, 0 when shared by all images
  const float* scales; int64_t scales_bs;       // [*, N, 3]
  const float* rots;   int64_t rots_bs;         // [*, N, 4] (r, x, y, z)
  const float* opac;   int64_t opac_bs;         // [*, N]
  const float* shs;    int64_t shs_bs;          // [*, N, M, 3] or NULL
  const float* colors; int64_t colors_bs;       // [*, N, 3] or NULL
  int M, deg;
  const float* view;                            // [B, 4, 4] row-vector convention: p_view = [x, 1] . view
  const float* proj;                            // [B, 4, 4]
  const float* campos;                          // [B, 3]
  const float* tanfovx;                         // [B]
  const float* tanfovy;                         // [B]
  float scale_mod;
  int B, N, H, W;
};

// SH basis values Y_k(d), k < (deg + 1)^2
A3D_DEV void sh_basis(int deg, float x, float y, float z, float* Y) {
  Y[0] = SH_C0;
  if (deg < 1) return;
  Y[1] = -SH_C1 * y; Y[2] = SH_C1 * z; Y[3] = -SH_C1 * x;
  if (deg < 2) return;
  const float xx = x * x, yy = y * y, zz = z * z;
  Y[4] = SH_C2[0] * x * y; Y[5] = SH_C2[1] * y * z; Y[6] = SH_C2[2] * (2.f * zz - xx - yy); Y[7] = SH_C2[3] * x * z;
  Y[8] = SH_C2[4] * (xx - yy);
  if (deg < 3) return;
  Y[9] = SH_C3[0] * y * (3.f * xx - yy); Y[10] = SH_C3[1] * x * y * z; Y[11] = SH_C3[2] * y * (4.f * zz - xx - yy);
  Y[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy); Y[13] = SH_C3[4] * x * (4.f * zz - xx - yy);
  Y[14] = SH_C3[5] * z * (xx - yy); Y[15] = SH_C3[6] * x * (xx - 3.f * yy);
}

// gradients dY_k / d(x, y, z)
A3D_DEV void sh_basis_grad(int deg, float x, float y, float z, float (*g)[3]) {
  g[0][0] = g[0][1] = g[0][2] = 0.f;
  if (deg < 1) return;
  g[1][0] = 0.f;     g[1][1] = -SH_C1; g[1][2] = 0.f;
  g[2][0] = 0.f;     g[2][1] = 0.f;    g[2][2] = SH_C1;
  g[3][0] = -SH_C1;  g[3][1] = 0.f;    g[3][2] = 0.f;
  if (deg < 2) return;
  const float xx = x * x, yy = y * y, zz = z * z;
  g[4][0] = SH_C2[0] * y;         g[4][1] = SH_C2[0] * x;         g[4][2] = 0.f;
  g[5][0] = 0.f;                  g[5][1] = SH_C2[1] * z;         g[5][2] = SH_C2[1] * y;
  g[6][0] = -2.f * SH_C2[2] * x;  g[6][1] = -2.f * SH_C2[2] * y;  g[6][2] = 4.f * SH_C2[2] * z;
  g[7][0] = SH_C2[3] * z;         g[7][1] = 0.f;                  g[7][2] = SH_C2[3] * x;
  g[8][0] = 2.f * SH_C2[4] * x;   g[8][1] = -2.f * SH_C2[4] * y;  g[8][2] = 0.f;
  if (deg < 3) return;
  g[9][0] = 6.f * SH_C3[0] * x * y;                 g[9][1] = SH_C3[0] * (3.f * xx - 3.f * yy);         g[9][2] = 0.f;
  g[10][0] = SH_C3[1] * y * z;                      g[10][1] = SH_C3[1] * x * z;                        g[10][2] = SH_C3[1] * x * y;
  g[11][0] = -2.f * SH_C3[2] * x * y;               g[11][1] = SH_C3[2] * (4.f * zz - xx - 3.f * yy);   g[11][2] = 8.f * SH_C3[2] * y * z;
  g[12][0] = -6.f * SH_C3[3] * x * z;               g[12][1] = -6.f * SH_C3[3] * y * z;                 g[12][2] = SH_C3[3] * (6.f * zz - 3.f * xx - 3.f * yy);
  g[13][0] = SH_C3[4] * (4.f * zz - 3.f * xx - yy); g[13][1] = -2.f * SH_C3[4] * x * y;                 g[13][2] = 8.f * SH_C3[4] * x * z;
  g[14][0] = 2.f * SH_C3[5] * x * z;                g[14][1] = -2.f * SH_C3[5] * y * z;                 g[14][2] = SH_C3[5] * (xx - yy);
  g[15][0] = SH_C3[6] * (3.f * xx - 3.f * yy);      g[15][1] = -6.f * SH_C3[6] * x * y;                 g[15][2] = 0.f;
}

// R(q / |q|) in the standard (column-vector) form; Sigma = R diag(s^2) R^T
A3D_DEV void quat_rot(const float* qin, float* qn, float& qnorm, float R[3][3]) {
  qnorm = sqrtf(qin[0] * qin[0] + qin[1] * qin[1] + qin[2] * qin[2] + qin[3] * qin[3]);
  const float inv = 1.f / qnorm;
  const float r = qin[0] * inv, x = qin[1] * inv, y = qin[2] * inv, z = qin[3] * inv;
  qn[0] = r; qn[1] = x; qn[2] = y; qn[3] = z;
  R[0][0] = 1.f - 2.f * (y * y + z * z); R[0][1] = 2.f * (x * y - r * z);       R[0][2] = 2.f * (x * z + r * y);
  R[1][0] = 2.f * (x * y + r * z);       R[1][1] = 1.f - 2.f * (x * x + z * z); R[1][2] = 2.f * (y * z - r * x);
  R[2][0] = 2.f * (x * z - r * y);       R[2][1] = 2.f * (y * z + r * x);       R[2][2] = 1.f - 2.f * (x * x + y * y);
}

// Everything the forward derives from one (image, Gaussian), recomputed identically by the backward.
struct GsProj {
  float t[3];          // p_view
  float txc, tyc;      // clamped t.x, t.y
  bool clx, cly;       // the clamp is active
  float hom[4];        // [x, 1] . proj
  float fx, fy;
  float Wc[3][3];      // rotation part of the view matrix, column-vector form: t = Wc x + tc
  float R[3][3], qn[4], qnorm, s[3];
  float Sig[3][3];
  float T[2][3];       // J Wc
  float a, b, c;       // 2-D covariance + 0.3 on the diagonal
};

A3D_DEV bool gs_project(const GsInputs& in, int bimg, int i, GsProj& p) {
  const float* m = in.means + bimg * in.means_bs + (int64_t)i * 3;
  const float* V = in.view + bimg * 16;
  const float* P = in.proj + bimg * 16;
  const float x = m[0], y = m[1], z = m[2];
#pragma unroll
  for (int c = 0; c < 3; ++c) p.t[c] = x * V[c] + y * V[4 + c] + z * V[8 + c] + V[12 + c];
  if (p.t[2] <= 0.2f) return false;
#pragma unroll
  for (int c = 0; c < 4; ++c) p.hom[c] = x * P[c] + y * P[4 + c] + z * P[8 + c] + P[12 + c];
  const float* sc = in.scales + bimg * in.scales_bs + (int64_t)i * 3;
  const float* q = in.rots + bimg * in.rots_bs + (int64_t)i * 4;
  quat_rot(q, p.qn, p.qnorm, p.R);
#pragma unroll
  for (int k = 0; k < 3; ++k) p.s[k] = sc[k] * in.scale_mod;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      p.Sig[r][c] = p.R[r][0] * p.s[0] * p.s[0] * p.R[c][0] + p.R[r][1] * p.s[1] * p.s[1] * p.R[c][1] + p.R[r][2] * p.s[2] * p.s[2] * p.R[c][2];
  const float tfx = in.tanfovx[bimg], tfy = in.tanfovy[bimg];
  p.fx = in.W / (2.f * tfx);
  p.fy = in.H / (2.f * tfy);
  const float limx = 1.3f * tfx, limy = 1.3f * tfy, tz = p.t[2];
  const float txtz = p.t[0] / tz, tytz = p.t[1] / tz;
  p.clx = txtz < -limx || txtz > limx;
  p.cly = tytz < -limy || tytz > limy;
  p.txc = fminf(limx, fmaxf(-limx, txtz)) * tz;
  p.tyc = fminf(limy, fmaxf(-limy, tytz)) * tz;
  const float J00 = p.fx / tz, J02 = -p.fx * p.txc / (tz * tz), J11 = p.fy / tz, J12 = -p.fy * p.tyc / (tz * tz);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) p.Wc[r][k] = V[k * 4 + r];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p.T[0][k] = J00 * p.Wc[0][k] + J02 * p.Wc[2][k];
    p.T[1][k] = J11 * p.Wc[1][k] + J12 * p.Wc[2][k];
  }
  float TS[2][3];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) TS[r][c] = p.T[r][0] * p.Sig[0][c] + p.T[r][1] * p.Sig[1][c] + p.T[r][2] * p.Sig[2][c];
  p.a = TS[0][0] * p.T[0][0] + TS[0][1] * p.T[0][1] + TS[0][2] * p.T[0][2] + 0.3f;
  p.b = TS[0][0] * p.T[1][0] + TS[0][1] * p.T[1][1] + TS[0][2] * p.T[1][2];
  p.c = TS[1][0] * p.T[1][0] + TS[1][1] * p.T[1][1] + TS[1][2] * p.T[1][2] + 0.3f;
  return true;
}

__global__ __launch_bounds__(256) void gs_preprocess_kernel(GsInputs in, int* __restrict__ radii, float2* __restrict__ xy,
                                                            float* __restrict__ depth, float4* __restrict__ conic_o, float* __restrict__ rgb,
                                                            int* __restrict__ clamped, int* __restrict__ tiles_touched) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)in.B * in.N) return;
  const int bimg = (int)(idx / in.N), i = (int)(idx % in.N);
  radii[idx] = 0;
  tiles_touched[idx] = 0;
  clamped[idx] = 0;
  GsProj p;
  if (!gs_project(in, bimg, i, p)) return;
  const float det = p.a * p.c - p.b * p.b;
  if (det == 0.f) return;
  const float det_inv = 1.f / det;
  const float mid = 0.5f * (p.a + p.c);
  const float l1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
  const int radius = (int)ceilf(3.f * sqrtf(l1));
  const float pw = 1.f / (p.hom[3] + 1e-7f);
  const float px = ((p.hom[0] * pw + 1.f) * in.W - 1.f) * 0.5f, py = ((p.hom[1] * pw + 1.f) * in.H - 1.f) * 0.5f;
  const int gx = (in.W + GS_TILE - 1) / GS_TILE, gy = (in.H + GS_TILE - 1) / GS_TILE;
  const int x0 = min(gx, max(0, (int)((px - radius) / GS_TILE))), x1 = min(gx, max(0, (int)((px + radius + GS_TILE - 1) / GS_TILE)));
  const int y0 = min(gy, max(0, (int)((py - radius) / GS_TILE))), y1 = min(gy, max(0, (int)((py + radius + GS_TILE - 1) / GS_TILE)));
  const int area = (x1 - x0) * (y1 - y0);
  if (area == 0) return;
  float col[3];
  int cl = 0;
  if (in.colors) {
    const float* cp = in.colors + bimg * in.colors_bs + (int64_t)i * 3;
    col[0] = cp[0]; col[1] = cp[1]; col[2] = cp[2];
  } else {
    const float* m = in.means + bimg * in.means_bs + (int64_t)i * 3;
    const float* cam = in.campos + bimg * 3;
    float d[3] = {m[0] - cam[0], m[1] - cam[1], m[2] - cam[2]};
    const float inv = 1.f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    float Y[16];
    sh_basis(in.deg, d[0] * inv, d[1] * inv, d[2] * inv, Y);
    const float* sh = in.shs + bimg * in.shs_bs + (int64_t)i * in.M * 3;
    const int K = (in.deg + 1) * (in.deg + 1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v = 0.f;
      for (int k = 0; k < K; ++k) v += Y[k] * sh[k * 3 + ch];
      v += 0.5f;
      if (v < 0.f) { cl |= 1 << ch; v = 0.f; }
      col[ch] = v;
    }
  }
  radii[idx] = radius;
  xy[idx] = make_float2(px, py);
  depth[idx] = p.t[2];
  conic_o[idx] = make_float4(p.c * det_inv, -p.b * det_inv, p.a * det_inv, in.opac[bimg * in.opac_bs + i]);
  rgb[idx * 3 + 0] = col[0]; rgb[idx * 3 + 1] = col[1]; rgb[idx * 3 + 2] = col[2];
  clamped[idx] = cl;
  tiles_touched[idx] = area;
}

__global__ __launch_bounds__(256) void gs_duplicate_kernel(int B, int N, int H, int W, const float2* __restrict__ xy,
                                                           const float* __restrict__ depth, const int* __restrict__ radii,
                                                           const int64_t* __restrict__ offsets, uint64_t* __restrict__ keys,
                                                           int* __restrict__ vals) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)B * N) return;
  const int r = radii[idx];
  if (r <= 0) return;
  const int bimg = (int)(idx / N);
  const int gx = (W + GS_TILE - 1) / GS_TILE, gy = (H + GS_TILE - 1) / GS_TILE;
  const float2 p = xy[idx];
  const int x0 = min(gx, max(0, (int)((p.x - r) / GS_TILE))), x1 = min(gx, max(0, (int)((p.x + r + GS_TILE - 1) / GS_TILE)));
  const int y0 = min(gy, max(0, (int)((p.y - r) / GS_TILE))), y1 = min(gy, max(0, (int)((p.y + r + GS_TILE - 1) / GS_TILE)));
  int64_t off = idx == 0 ? 0 : offsets[idx - 1];
  const uint64_t dbits = (uint64_t)__float_as_uint(depth[idx]);
  const uint64_t base = (uint64_t)bimg * (uint64_t)(gx * gy);
  for (int ty = y0; ty < y1; ++ty)
    for (int tx = x0; tx < x1; ++tx) {
      keys[off] = ((base + (uint64_t)(ty * gx + tx)) << 32) | dbits;
      vals[off] = (int)(idx % N);
      ++off;
    }
}

__global__ __launch_bounds__(256) void gs_tile_ranges_kernel(const uint64_t* __restrict__ keys, int64_t L, int2* __restrict__ ranges) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= L) return;
  const int cur = (int)(keys[s] >> 32);
  if (s == 0) ranges[cur].x = 0;
  else {
    const int prev = (int)(keys[s - 1] >> 32);
    if (prev != cur) { ranges[prev].y = (int)s; ranges[cur].x = (int)s; }
  }
  if (s == L - 1) ranges[cur].y = (int)L;
}

__global__ __launch_bounds__(GS_BLOCK) void gs_render_kernel(int B, int N, int H, int W, const int2* __restrict__ ranges,
                                                             const int64_t* __restrict__ perm, const int* __restrict__ vals,
                                                             const float2* __restrict__ xy, const float4* __restrict__ conic_o,
                                                             const float* __restrict__ rgb, const float* __restrict__ depth,
                                                             const float* __restrict__ bg, float* __restrict__ out_img,
                                                             float* __restrict__ out_depth, float* __restrict__ out_alpha,
                                                             float* __restrict__ T_final, int* __restrict__ n_contrib) {
  __shared__ float2 s_xy[GS_BLOCK];
  __shared__ float4 s_co[GS_BLOCK];
  __shared__ float s_rgbd[GS_BLOCK][4];
  const int gx = gridDim.x, bimg = blockIdx.z;
  const int px = blockIdx.x * GS_TILE + (threadIdx.x & 15), py = blockIdx.y * GS_TILE + (threadIdx.x >> 4);
  const bool inside = px < W && py < H;
  const int2 range = ranges[(int64_t)bimg * gx * gridDim.y + blockIdx.y * gx + blockIdx.x];
  const int total = range.y - range.x;
  const float pfx = (float)px, pfy = (float)py;
  bool done = !inside;
  float T = 1.f, C[3] = {0.f, 0.f, 0.f}, D = 0.f;
  int contributor = 0, last = 0;
  for (int base = 0; base < total; base += GS_BLOCK) {
    if (__syncthreads_count(done) == GS_BLOCK) break;
    const int k = base + threadIdx.x;
    if (k < total) {
      const int64_t g = (int64_t)bimg * N + vals[perm[range.x + k]];
      s_xy[threadIdx.x] = xy[g];
      s_co[threadIdx.x] = conic_o[g];
      s_rgbd[threadIdx.x][0] = rgb[g * 3 + 0]; s_rgbd[threadIdx.x][1] = rgb[g * 3 + 1]; s_rgbd[threadIdx.x][2] = rgb[g * 3 + 2];
      s_rgbd[threadIdx.x][3] = depth[g];
    }
    __syncthreads();
    const int cnt = min(GS_BLOCK, total - base);
    for (int j = 0; !done && j < cnt; ++j) {
      ++contributor;
      const float2 c = s_xy[j];
      const float4 co = s_co[j];
      const float dx = c.x - pfx, dy = c.y - pfy;
      const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
      if (power > 0.f) continue;
      const float alpha = fminf(0.99f, co.w * __expf(power));
      if (alpha < 1.f / 255.f) continue;
      const float test_T = T * (1.f - alpha);
      if (test_T < 0.0001f) { done = true; continue; }
      const float w = alpha * T;
      C[0] += s_rgbd[j][0] * w; C[1] += s_rgbd[j][1] * w; C[2] += s_rgbd[j][2] * w;
      D += s_rgbd[j][3] * w;
      T = test_T;
      last = contributor;
    }
  }
  if (inside) {
    const int64_t HW = (int64_t)H * W, pix = (int64_t)py * W + px;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out_img[((int64_t)bimg * 3 + ch) * HW + pix] = C[ch] + T * bg[ch];
    out_depth[bimg * HW + pix] = D;
    out_alpha[bimg * HW + pix] = 1.f - T;
    T_final[bimg * HW + pix] = T;
    n_contrib[bimg * HW + pix] = last;
  }
}

// Sum over the 16 lanes of each DPP row: every lane of the row ends up holding the row's sum.
A3D_DEV float row16_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xF, 0xF, false));   // row_ror:4
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, false));   // row_ror:8
  return v;
}

A3D_DEV float wave64_sum(float v) {
  v = row16_sum(v);
  return (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16))) +
         (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48)));
}

__global__ __launch_bounds__(GS_BLOCK) void gs_render_bwd_kernel(int B, int N, int H, int W, const int2* __restrict__ ranges,
                                                                 const int64_t* __restrict__ perm, const int* __restrict__ vals,
                                                                 const float2* __restrict__ xy, const float4* __restrict__ conic_o,
                                                                 const float* __restrict__ rgb, const float* __restrict__ depth,
                                                                 const float* __restrict__ bg, const float* __restrict__ T_final,
                                                                 const int* __restrict__ n_contrib, const float* __restrict__ d_img,
                                                                 const float* __restrict__ d_depth, const float* __restrict__ d_alpha,
                                                                 float* __restrict__ rows) {
  __shared__ float2 s_xy[GS_BLOCK];
  __shared__ float4 s_co[GS_BLOCK];
  __shared__ float s_rgbd[GS_BLOCK][4];
  __shared__ float s_part[4][GS_BLOCK][10];
  __shared__ int s_maxlast;
  const int gx = gridDim.x, bimg = blockIdx.z;
  const int px = blockIdx.x * GS_TILE + (threadIdx.x & 15), py = blockIdx.y * GS_TILE + (threadIdx.x >> 4);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool inside = px < W && py < H;
  const int2 range = ranges[(int64_t)bimg * gx * gridDim.y + blockIdx.y * gx + blockIdx.x];
  const int total = range.y - range.x;
  const int64_t HW = (int64_t)H * W, pix = (int64_t)py * W + px;
  const float pfx = (float)px, pfy = (float)py;
  float T = 1.f, Tf = 1.f, dpix[3] = {0.f, 0.f, 0.f}, dD = 0.f, dA = 0.f;
  int last = 0;
  if (inside) {
    Tf = T = T_final[bimg * HW + pix];
    last = n_contrib[bimg * HW + pix];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dpix[ch] = d_img[((int64_t)bimg * 3 + ch) * HW + pix];
    if (d_depth) dD = d_depth[bimg * HW + pix];
    if (d_alpha) dA = d_alpha[bimg * HW + pix];
  }
  const float bgdot = bg[0] * dpix[0] + bg[1] * dpix[1] + bg[2] * dpix[2];
  if (threadIdx.x == 0) s_maxlast = 0;
  __syncthreads();
  if (last > 0) atomicMax(&s_maxlast, last);          // LDS only: the tile's deepest contributor
  __syncthreads();
  const int maxlast = s_maxlast;
  float acc[3] = {0.f, 0.f, 0.f}, last_col[3] = {0.f, 0.f, 0.f}, accD = 0.f, last_d = 0.f, last_alpha = 0.f;
  // batches from the back: batch k holds range positions total-1-k*256 .. downwards; LDS slot j = position total-1-k*256-j
  for (int top = total - 1; top >= 0; top -= GS_BLOCK) {
    const int cnt = min(GS_BLOCK, top + 1);
    const int lowest = top - cnt + 1;                 // range-relative position of the batch's front-most Gaussian
    const bool live = lowest < maxlast;                // otherwise no pixel of the tile reached this batch: zero rows
    __syncthreads();
    if (live && threadIdx.x < cnt) {
      const int64_t g = (int64_t)bimg * N + vals[perm[range.x + top - threadIdx.x]];
      s_xy[threadIdx.x] = xy[g];
      s_co[threadIdx.x] = conic_o[g];
      s_rgbd[threadIdx.x][0] = rgb[g * 3 + 0]; s_rgbd[threadIdx.x][1] = rgb[g * 3 + 1]; s_rgbd[threadIdx.x][2] = rgb[g * 3 + 2];
      s_rgbd[threadIdx.x][3] = depth[g];
    }
    __syncthreads();
    if (live) {
      for (int j = 0; j < cnt; ++j) {
        const int posn = top - j;                      // contributes iff posn < last (the forward's contributor count)
        float gr[10];
#pragma unroll
        for (int e = 0; e < 10; ++e) gr[e] = 0.f;
        bool contrib = false;
        if (posn < last) {
          const float2 c = s_xy[j];
          const float4 co = s_co[j];
          const float dx = c.x - pfx, dy = c.y - pfy;
          const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
          if (power <= 0.f) {
            const float G = __expf(power);
            const float oG = co.w * G;
            const float alpha = fminf(0.99f, oG);
            if (alpha >= 1.f / 255.f) {
              contrib = true;
              T = T / (1.f - alpha);
              const float w = alpha * T;
              float dLda = 0.f;
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) {
                const float col = s_rgbd[j][ch];
                acc[ch] = last_alpha * last_col[ch] + (1.f - last_alpha) * acc[ch];
                last_col[ch] = col;
                dLda += (col - acc[ch]) * dpix[ch];
                gr[6 + ch] = w * dpix[ch];
              }
              const float z = s_rgbd[j][3];
              accD = last_alpha * last_d + (1.f - last_alpha) * accD;
              last_d = z;
              dLda += (z - accD) * dD;
              gr[9] = w * dD;
              last_alpha = alpha;
              dLda *= T;
              const float tf1 = Tf / (1.f - alpha);
              dLda += tf1 * (dA - bgdot);
              if (oG <= 0.99f) {                        // alpha = min(0.99, o G): no gradient through the clamp
                const float dLdG = co.w * dLda;
                const float gdx = G * dx, gdy = G * dy;
                gr[0] = dLdG * (-gdx * co.x - gdy * co.y);
                gr[1] = dLdG * (-gdy * co.z - gdx * co.y);
                gr[2] = -0.5f * gdx * dx * dLdG;
                gr[3] = -gdx * dy * dLdG;
                gr[4] = -0.5f * gdy * dy * dLdG;
                gr[5] = G * dLda;
              }
            }
          }
        }
        if (__any(contrib)) {
#pragma unroll
          for (int e = 0; e < 10; ++e) {
            const float s = wave64_sum(gr[e]);
            if (lane == 0) s_part[wave][j][e] = s;
          }
        } else if (lane == 0) {
#pragma unroll
          for (int e = 0; e < 10; ++e) s_part[wave][j][e] = 0.f;
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < cnt) {
      float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
      if (live) {
        float v[10];
#pragma unroll
        for (int e = 0; e < 10; ++e)
          v[e] = (s_part[0][threadIdx.x][e] + s_part[1][threadIdx.x][e]) + (s_part[2][threadIdx.x][e] + s_part[3][threadIdx.x][e]);
        r0 = make_float4(v[0], v[1], v[2], v[3]);
        r1 = make_float4(v[4], v[5], v[6], v[7]);
        r2 = make_float4(v[8], v[9], 0.f, 0.f);
      }
      float4* dst = reinterpret_cast<float4*>(rows + perm[range.x + top - threadIdx.x] * GS_ROW);
      dst[0] = r0; dst[1] = r1; dst[2] = r2;
    }
  }
}

__global__ __launch_bounds__(256) void gs_preprocess_bwd_kernel(GsInputs in, const int* __restrict__ radii, const int* __restrict__ clamped,
                                                                const int64_t* __restrict__ offsets, const int* __restrict__ tiles_touched,
                                                                const float* __restrict__ rows, float* __restrict__ d_means2d,
                                                                float* __restrict__ d_means, float* __restrict__ d_scales,
                                                                float* __restrict__ d_rots, float* __restrict__ d_opac,
                                                                float* __restrict__ d_shs, float* __restrict__ d_colors) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)in.B * in.N) return;
  const int bimg = (int)(idx / in.N), i = (int)(idx % in.N);
  float g[10];
#pragma unroll
  for (int e = 0; e < 10; ++e) g[e] = 0.f;
  GsProj p;
  const bool vis = radii[idx] > 0 && gs_project(in, bimg, i, p);
  if (vis) {
    const int64_t end = offsets[idx], start = end - tiles_touched[idx];
    for (int64_t r = start; r < end; ++r) {
      const float4* src = reinterpret_cast<const float4*>(rows + r * GS_ROW);
      const float4 a = src[0], b = src[1], c = src[2];
      g[0] += a.x; g[1] += a.y; g[2] += a.z; g[3] += a.w; g[4] += b.x; g[5] += b.y; g[6] += b.z; g[7] += b.w; g[8] += c.x; g[9] += c.y;
    }
  }
  float dm[3] = {0.f, 0.f, 0.f}, ds[3] = {0.f, 0.f, 0.f}, dq[4] = {0.f, 0.f, 0.f, 0.f}, dcol[3] = {g[6], g[7], g[8]};
  float dndc[2] = {0.f, 0.f};
  if (vis) {
    // centre: pixel = ((ndc + 1) size - 1) / 2
    dndc[0] = g[0] * 0.5f * in.W;
    dndc[1] = g[1] * 0.5f * in.H;
    const float* P = in.proj + bimg * 16;
    const float wi = 1.f / (p.hom[3] + 1e-7f);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      dm[k] += dndc[0] * (P[k * 4 + 0] * wi - p.hom[0] * P[k * 4 + 3] * wi * wi) + dndc[1] * (P[k * 4 + 1] * wi - p.hom[1] * P[k * 4 + 3] * wi * wi);
    // conic -> 2-D covariance: d Sigma' = -Q G Q, Q = Sigma'^-1, G = [[gA, gB/2], [gB/2, gC]]
    const float det = p.a * p.c - p.b * p.b, di = 1.f / det;
    const float Q00 = p.c * di, Q01 = -p.b * di, Q11 = p.a * di;
    const float G00 = g[2], G01 = 0.5f * g[3], G11 = g[4];
    const float QG00 = Q00 * G00 + Q01 * G01, QG01 = Q00 * G01 + Q01 * G11, QG10 = Q01 * G00 + Q11 * G01, QG11 = Q01 * G01 + Q11 * G11;
    float Gc[2][2];
    Gc[0][0] = -(QG00 * Q00 + QG01 * Q01);
    Gc[0][1] = -(QG00 * Q01 + QG01 * Q11);
    Gc[1][0] = -(QG10 * Q00 + QG11 * Q01);
    Gc[1][1] = -(QG10 * Q01 + QG11 * Q11);
    // Sigma' = T Sigma T^T: dSigma = T^T Gc T, dT = 2 Gc T Sigma
    float GT[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) GT[r][k] = Gc[r][0] * p.T[0][k] + Gc[r][1] * p.T[1][k];
    float dSig[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) dSig[r][c] = p.T[0][r] * GT[0][c] + p.T[1][r] * GT[1][c];
    float dT[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) dT[r][c] = 2.f * (GT[r][0] * p.Sig[0][c] + GT[r][1] * p.Sig[1][c] + GT[r][2] * p.Sig[2][c]);
    // T = J Wc: dJ = dT Wc^T (only the four non-constant entries of J matter)
    const float dJ00 = dT[0][0] * p.Wc[0][0] + dT[0][1] * p.Wc[0][1] + dT[0][2] * p.Wc[0][2];
    const float dJ02 = dT[0][0] * p.Wc[2][0] + dT[0][1] * p.Wc[2][1] + dT[0][2] * p.Wc[2][2];
    const float dJ11 = dT[1][0] * p.Wc[1][0] + dT[1][1] * p.Wc[1][1] + dT[1][2] * p.Wc[1][2];
    const float dJ12 = dT[1][0] * p.Wc[2][0] + dT[1][1] * p.Wc[2][1] + dT[1][2] * p.Wc[2][2];
    const float tz = p.t[2], tz2 = tz * tz, tz3 = tz2 * tz;
    const float dtxc = -p.fx / tz2 * dJ02, dtyc = -p.fy / tz2 * dJ12;
    float dt[3];
    dt[2] = -p.fx / tz2 * dJ00 - p.fy / tz2 * dJ11 + 2.f * p.fx * p.txc / tz3 * dJ02 + 2.f * p.fy * p.tyc / tz3 * dJ12 + g[9];
    dt[0] = p.clx ? 0.f : dtxc;
    dt[1] = p.cly ? 0.f : dtyc;
    if (p.clx) dt[2] += dtxc * (p.txc / tz);          // clamped: txc = +-lim tz
    if (p.cly) dt[2] += dtyc * (p.tyc / tz);
#pragma unroll
    for (int k = 0; k < 3; ++k) dm[k] += p.Wc[0][k] * dt[0] + p.Wc[1][k] * dt[1] + p.Wc[2][k] * dt[2];
    // Sigma = R diag(s^2) R^T
    float RtdR[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) v += p.R[r][k] * dSig[r][c] * p.R[c][k];
      RtdR[k] = v;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) ds[k] = RtdR[k] * 2.f * p.s[k] * in.scale_mod;
    float dR[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        dR[r][k] = 2.f * (dSig[r][0] * p.R[0][k] + dSig[r][1] * p.R[1][k] + dSig[r][2] * p.R[2][k]) * p.s[k] * p.s[k];
    const float r = p.qn[0], x = p.qn[1], y = p.qn[2], z = p.qn[3];
    float dqn[4];
    dqn[0] = 2.f * (z * (dR[1][0] - dR[0][1]) + y * (dR[0][2] - dR[2][0]) + x * (dR[2][1] - dR[1][2]));
    dqn[1] = 2.f * (y * (dR[1][0] + dR[0][1]) + z * (dR[2][0] + dR[0][2]) + r * (dR[2][1] - dR[1][2])) - 4.f * x * (dR[2][2] + dR[1][1]);
    dqn[2] = 2.f * (x * (dR[1][0] + dR[0][1]) + r * (dR[0][2] - dR[2][0]) + z * (dR[2][1] + dR[1][2])) - 4.f * y * (dR[2][2] + dR[0][0]);
    dqn[3] = 2.f * (r * (dR[1][0] - dR[0][1]) + x * (dR[2][0] + dR[0][2]) + y * (dR[2][1] + dR[1][2])) - 4.f * z * (dR[1][1] + dR[0][0]);
    const float dot = r * dqn[0] + x * dqn[1] + y * dqn[2] + z * dqn[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) dq[k] = (dqn[k] - p.qn[k] * dot) / p.qnorm;
  }
  // colour
  if (in.colors) {
    float* dc = d_colors + idx * 3;
    dc[0] = dcol[0]; dc[1] = dcol[1]; dc[2] = dcol[2];
  } else {
    float* dsh = d_shs + idx * in.M * 3;
    const int K = (in.deg + 1) * (in.deg + 1);
    if (vis) {
      const int cl = clamped[idx];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        if ((cl >> ch) & 1) dcol[ch] = 0.f;
      const float* m = in.means + bimg * in.means_bs + (int64_t)i * 3;
      const float* cam = in.campos + bimg * 3;
      const float v[3] = {m[0] - cam[0], m[1] - cam[1], m[2] - cam[2]};
      const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), inv = 1.f / len;
      const float d[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
      float Y[16], gY[16][3];
      sh_basis(in.deg, d[0], d[1], d[2], Y);
      sh_basis_grad(in.deg, d[0], d[1], d[2], gY);
      const float* sh = in.shs + bimg * in.shs_bs + (int64_t)i * in.M * 3;
      float dd[3] = {0.f, 0.f, 0.f};
      for (int k = 0; k < K; ++k) {
        const float w = sh[k * 3] * dcol[0] + sh[k * 3 + 1] * dcol[1] + sh[k * 3 + 2] * dcol[2];
        dd[0] += gY[k][0] * w; dd[1] += gY[k][1] * w; dd[2] += gY[k][2] * w;
        dsh[k * 3 + 0] = Y[k] * dcol[0]; dsh[k * 3 + 1] = Y[k] * dcol[1]; dsh[k * 3 + 2] = Y[k] * dcol[2];
      }
      const float ddot = d[0] * dd[0] + d[1] * dd[1] + d[2] * dd[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) dm[k] += (dd[k] - d[k] * ddot) * inv;
    } else {
      for (int k = 0; k < K * 3; ++k) dsh[k] = 0.f;
    }
    for (int k = K * 3; k < in.M * 3; ++k) dsh[k] = 0.f;
  }
  d_means2d[idx * 3 + 0] = dndc[0]; d_means2d[idx * 3 + 1] = dndc[1]; d_means2d[idx * 3 + 2] = 0.f;
  d_means[idx * 3 + 0] = dm[0]; d_means[idx * 3 + 1] = dm[1]; d_means[idx * 3 + 2] = dm[2];
  d_scales[idx * 3 + 0] = ds[0]; d_scales[idx * 3 + 1] = ds[1]; d_scales[idx * 3 + 2] = ds[2];
  d_rots[idx * 4 + 0] = dq[0]; d_rots[idx * 4 + 1] = dq[1]; d_rots[idx * 4 + 2] = dq[2]; d_rots[idx * 4 + 3] = dq[3];
  d_opac[idx] = vis ? g[5] : 0.f;
}

// extents shared by duplicate / render / render_bwd: B N Gaussians and B * tiles ranges are indexed in 32 bits
inline bool gs_extents_ok(int B, int N, int H, int W) {
  if (B <= 0 || N <= 0 || H <= 0 || W <= 0 || (int64_t)B * N > 0x7fffffffLL) return false;
  const int64_t gx = ((int64_t)W + GS_TILE - 1) / GS_TILE, gy = ((int64_t)H + GS_TILE - 1) / GS_TILE;
  return gx * gy <= 0x7fffffffLL / B;
}

inline bool gs_inputs_ok(const GsInputs& in) {
  if (!gs_extents_ok(in.B, in.N, in.H, in.W)) return false;
  if (!in.means || !in.scales || !in.rots || !in.opac || !in.view || !in.proj || !in.campos || !in.tanfovx || !in.tanfovy) return false;
  if ((in.shs == nullptr) == (in.colors == nullptr)) return false;                 // exactly one colour source
  if (in.shs && (in.deg < 0 || in.deg > 3 || in.M < (in.deg + 1) * (in.deg + 1))) return false;
  return a3d_aligned(4, in.means, in.scales, in.rots, in.opac, in.shs, in.colors, in.view, in.proj, in.campos, in.tanfovx, in.tanfovy);
}

GsInputs make_inputs(int B, int N, const float* means, int64_t means_bs, const float* scales, int64_t scales_bs, const float* rots,
                     int64_t rots_bs, const float* opac, int64_t opac_bs, const float* shs, int64_t shs_bs, int M, int deg,
                     const float* colors, int64_t colors_bs, const float* view, const float* proj, const float* campos,
                     const float* tanfovx, const float* tanfovy, int H, int W, float scale_mod) {
  GsInputs in;
  in.means = means; in.means_bs = means_bs; in.scales = scales; in.scales_bs = scales_bs; in.rots = rots; in.rots_bs = rots_bs;
  in.opac = opac; in.opac_bs = opac_bs; in.shs = shs; in.shs_bs = shs_bs; in.colors = colors; in.colors_bs = colors_bs;
  in.M = M; in.deg = deg; in.view = view; in.proj = proj; in.campos = campos; in.tanfovx = tanfovx; in.tanfovy = tanfovy;
  in.scale_mod = scale_mod; in.B = B; in.N = N; in.H = H; in.W = W;
  return in;
}

}  // namespace

#define A3D_GS_INPUT_PARAMS                                                                                                            \
  int B, int N, const float *means, int64_t means_bs, const float *scales, int64_t scales_bs, const float *rots, int64_t rots_bs,   \
      const float *opac, int64_t opac_bs, const float *shs, int64_t shs_bs, int M, int deg, const float *colors, int64_t colors_bs, \
      const float *view, const float *proj, const float *campos, const float *tanfovx, const float *tanfovy, int H, int W, float scale_mod
#define A3D_GS_INPUT_ARGS                                                                                                              \
  B, N, means, means_bs, scales, scales_bs, rots, rots_bs, opac, opac_bs, shs, shs_bs, M, deg, colors, colors_bs, view, proj, campos, \
      tanfovx, tanfovy, H, W, scale_mod

extern "C" int a3d_gs_preprocess_f32(a3d_stream_t stream, A3D_GS_INPUT_PARAMS, int* radii, float* xy, float* depth, float* conic_o,
                                     float* rgb, int* clamped, int* tiles_touched) {
  const GsInputs in = make_inputs(A3D_GS_INPUT_ARGS);
  if (!gs_inputs_ok(in) || !radii || !xy || !depth || !conic_o || !rgb || !clamped || !tiles_touched) return A3D_EINVAL;
  if (!a3d_aligned(16, conic_o) || !a3d_aligned(8, xy) || !a3d_aligned(4, radii, depth, rgb, clamped, tiles_touched)) return A3D_EINVAL;
  gs_preprocess_kernel<<<blocks_for((int64_t)B * N), 256, 0, (hipStream_t)stream>>>(in, radii, reinterpret_cast<float2*>(xy), depth,
                                                                                     reinterpret_cast<float4*>(conic_o), rgb, clamped, tiles_touched);
  return a3d_launch_status();
}

extern "C" int a3d_gs_duplicate_f32(a3d_stream_t stream, int B, int N, int H, int W, const float* xy, const float* depth, const int* radii,
                                    const int64_t* offsets, int64_t* keys, int* vals) {
  if (!gs_extents_ok(B, N, H, W) || !xy || !depth || !radii || !offsets || !keys || !vals || !a3d_aligned(8, xy, offsets, keys) ||
      !a3d_aligned(4, depth, radii, vals))
    return A3D_EINVAL;
  gs_duplicate_kernel<<<blocks_for((int64_t)B * N), 256, 0, (hipStream_t)stream>>>(B, N, H, W, reinterpret_cast<const float2*>(xy), depth, radii,
                                                                                    offsets, reinterpret_cast<uint64_t*>(keys), vals);
  return a3d_launch_status();
}

extern "C" int a3d_gs_tile_ranges_f32(a3d_stream_t stream, const int64_t* keys, int64_t L, int* ranges, int64_t n_tiles) {
  if (!ranges || n_tiles <= 0 || L < 0 || L > 0x7fffffffLL || (L > 0 && !keys) || !a3d_aligned(8, ranges, keys)) return A3D_EINVAL;
  if (hipError_t e = hipMemsetAsync(ranges, 0, n_tiles * 2 * sizeof(int), (hipStream_t)stream); e != hipSuccess) return (int)e;
  if (L == 0) return A3D_OK;
  gs_tile_ranges_kernel<<<blocks_for(L), 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const uint64_t*>(keys), L, reinterpret_cast<int2*>(ranges));
  return a3d_launch_status();
}

extern "C" int a3d_gs_render_f32(a3d_stream_t stream, int B, int N, int H, int W, const int* ranges, const int64_t* perm, const int* vals,
                                 const float* xy, const float* conic_o, const float* rgb, const float* depth, const float* bg,
                                 float* out_img, float* out_depth, float* out_alpha, float* T_final, int* n_contrib) {
  if (!gs_extents_ok(B, N, H, W) || !ranges || !perm || !vals || !xy || !conic_o || !rgb || !depth || !bg || !out_img || !out_depth ||
      !out_alpha || !T_final || !n_contrib || !a3d_aligned(16, conic_o) || !a3d_aligned(8, xy, ranges, perm) ||
      !a3d_aligned(4, vals, rgb, depth, bg, out_img, out_depth, out_alpha, T_final, n_contrib))
    return A3D_EINVAL;
  const dim3 grid((W + GS_TILE - 1) / GS_TILE, (H + GS_TILE - 1) / GS_TILE, B);
  gs_render_kernel<<<grid, GS_BLOCK, 0, (hipStream_t)stream>>>(B, N, H, W, reinterpret_cast<const int2*>(ranges), perm, vals,
                                                               reinterpret_cast<const float2*>(xy), reinterpret_cast<const float4*>(conic_o), rgb,
                                                               depth, bg, out_img, out_depth, out_alpha, T_final, n_contrib);
  return a3d_launch_status();
}

extern "C" int a3d_gs_render_bwd_f32(a3d_stream_t stream, int B, int N, int H, int W, const int* ranges, const int64_t* perm, const int* vals,
                                     const float* xy, const float* conic_o, const float* rgb, const float* depth, const float* bg,
                                     const float* T_final, const int* n_contrib, const float* d_img, const float* d_depth,
                                     const float* d_alpha, float* rows) {
  if (!gs_extents_ok(B, N, H, W) || !ranges || !perm || !vals || !xy || !conic_o || !rgb || !depth || !bg || !T_final || !n_contrib ||
      !d_img || !rows || !a3d_aligned(16, conic_o, rows) || !a3d_aligned(8, xy, ranges, perm) ||
      !a3d_aligned(4, vals, rgb, depth, bg, T_final, n_contrib, d_img, d_depth, d_alpha))
    return A3D_EINVAL;
  const dim3 grid((W + GS_TILE - 1) / GS_TILE, (H + GS_TILE - 1) / GS_TILE, B);
  gs_render_bwd_kernel<<<grid, GS_BLOCK, 0, (hipStream_t)stream>>>(B, N, H, W, reinterpret_cast<const int2*>(ranges), perm, vals,
                                                                   reinterpret_cast<const float2*>(xy), reinterpret_cast<const float4*>(conic_o),
                                                                   rgb, depth, bg, T_final, n_contrib, d_img, d_depth, d_alpha, rows);
  return a3d_launch_status();
}

extern "C" int a3d_gs_preprocess_bwd_f32(a3d_stream_t stream, A3D_GS_INPUT_PARAMS, const int* radii, const int* clamped, const int64_t* offsets,
                                         const int* tiles_touched, const float* rows, float* d_means2d, float* d_means, float* d_scales,
                                         float* d_rots, float* d_opac, float* d_shs, float* d_colors) {
  const GsInputs in = make_inputs(A3D_GS_INPUT_ARGS);
  if (!gs_inputs_ok(in) || !radii || !clamped || !offsets || !tiles_touched || !d_means2d || !d_means || !d_scales || !d_rots || !d_opac ||
      !rows || (shs && !d_shs) || (colors && !d_colors) || !a3d_aligned(16, rows) || !a3d_aligned(8, offsets) ||
      !a3d_aligned(4, radii, clamped, tiles_touched, d_means2d, d_means, d_scales, d_rots, d_opac, d_shs, d_colors))
    return A3D_EINVAL;
  gs_preprocess_bwd_kernel<<<blocks_for((int64_t)B * N), 256, 0, (hipStream_t)stream>>>(in, radii, clamped, offsets, tiles_touched, rows, d_means2d,
                                                                                         d_means, d_scales, d_rots, d_opac, d_shs, d_colors);
  return a3d_launch_status();
}

extern "C" int a3d_gs_sum_batch_f32(a3d_stream_t stream, const float* src, float* dst, int B, int64_t M) {
  if (!src || !dst || B <= 0 || M <= 0 || !a3d_aligned(4, src, dst)) return A3D_EINVAL;
  sum_leading((hipStream_t)stream, src, dst, B, M);
  return a3d_launch_status();
}
