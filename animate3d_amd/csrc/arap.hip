// ARAP (as-rigid-as-possible) rigidity loss of the 4D-SDS stage and its k-NN graph on gfx950; contract in animate3d_amd/arap.py.
// Replaces cal_connectivity_from_points / estimate_rotation / cal_arap_error (custom/threestudio-animate3d/systems/util.py:58-215), whose
// pytorch3d.ops.knn_points has no ROCm build and whose per-frame loop synchronises with the host several times per frame.
//
//   knn_kernel<K>        exact all-pairs search: one query per lane, candidates staged in LDS in tiles of KNN_TILE float4 (every lane reads
//                        the same candidate: an LDS broadcast), the K best as a sorted list in registers (compile-time indices only: no
//                        scratch).  Candidates arrive in ascending index order and a candidate enters only when strictly closer than the
//                        current worst, behind every entry that is not farther: the list is sorted by (distance, index).
//   arap_energy_kernel   one thread per (frame, sample): S = sum_k w_k src_k^T tgt_k, R = W U^T of S = U Sigma W^T made proper, the
//                        energy of the sample.  fp64 inside (there are only F * S problems): the decomposition is a one-sided Jacobi
//                        (Hestenes) SVD, which is accurate in the small singular values too; the proper rotation is assembled from the two
//                        dominant singular pairs, R = w0 u0^T + w1 u1^T + (w0 x w1)(u0 x u1)^T, which equals W U^T where det > 0 and W U^T with
//                        the smallest singular value's column of U flipped where det <= 0.
//   arap_reduce_kernel   the F * S energies summed in a fixed order by one block: thread t adds t, t + 256, ..., then loss_reduce.h's tree
//   arap_bwd_kernel      gather form: one thread per (frame, vertex) walks the vertex's entries of the inverse list (sorted (sample, slot)
//                        pairs: slot 0 the sample's centre, slot k + 1 its k-th neighbour); no atomics, rows without entries are written 0
//   mesh_sample_kernel   the mesh branch's per-step neighbour draw (sample_matrix_vectorized, util.py:320-344: rand + masked add + sort +
//                        gather over [Nv, Dmax]): one thread per vertex walks its CSR row once and keeps K of its d positions by selection
//                        sampling (Knuth's Algorithm S) on Philox4x32-10 words keyed by (seed, vertex, position).  Integers only, no LDS,
//                        no per-thread array, nothing that depends on a maximum degree or on the launch geometry
#include "f32_common.h"
#include "loss_reduce.h"

#include <math.h>

namespace {

constexpr int KNN_BLOCK = 256;
constexpr int KNN_TILE = 1024;        // 16 KiB of LDS per block
constexpr int ARAP_BLOCK = 128;

template <int K>
__global__ __launch_bounds__(KNN_BLOCK) void knn_kernel(int N, const float* __restrict__ pts, int Kout, int least, float r2, int* __restrict__ nn_idx,
                                                        float* __restrict__ nn_dist) {
  __shared__ float4 tile[KNN_TILE];
  const int i = blockIdx.x * KNN_BLOCK + threadIdx.x;
  const int iq = i < N ? i : N - 1;                  // lanes past the end repeat the last query and store nothing
  const float qx = pts[3 * (int64_t)iq], qy = pts[3 * (int64_t)iq + 1], qz = pts[3 * (int64_t)iq + 2];
  float bd[K];
  int bi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    bd[k] = INFINITY;
    bi[k] = -1;
  }
  for (int base = 0; base < N; base += KNN_TILE) {
    const int n = min(KNN_TILE, N - base);
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += KNN_BLOCK) {
      const float* p = pts + 3 * (int64_t)(base + t);
      tile[t] = make_float4(p[0], p[1], p[2], 0.f);
    }
    __syncthreads();
    for (int t = 0; t < n; ++t) {
      const float4 c = tile[t];
      const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
      float d = dx * dx + dy * dy + dz * dz;
      const int j = base + t;
      if (j == iq) d = INFINITY;                     // a point is never its own neighbour
      if (d < bd[K - 1]) {
#pragma unroll
        for (int s = K - 1; s > 0; --s) {
          if (d < bd[s - 1]) {
            bd[s] = bd[s - 1];
            bi[s] = bi[s - 1];
          } else if (d < bd[s]) {
            bd[s] = d;
            bi[s] = j;
          }
        }
        if (d < bd[0]) {
          bd[0] = d;
          bi[0] = j;
        }
      }
    }
  }
  if (i < N) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (k < Kout) {
        const bool cut = k >= least && !(bd[k] < r2);
        nn_idx[(int64_t)i * Kout + k] = cut ? -1 : bi[k];
        nn_dist[(int64_t)i * Kout + k] = cut ? INFINITY : bd[k];
      }
    }
  }
}

struct ArapArgs {
  int F, Nv, K, S;
  const float* src;
  const float* tgt;
  int64_t tgt_bs;
  const int* nn;
  const float* w;
  const int* sidx;
};

#define ARAP_ROT(p, q)                                                                          \
  {                                                                                             \
    double al = 0.0, be = 0.0, ga = 0.0;                                                        \
    _Pragma("unroll") for (int r = 0; r < 3; ++r) {                                             \
      al += G[r][p] * G[r][p];                                                                  \
      be += G[r][q] * G[r][q];                                                                  \
      ga += G[r][p] * G[r][q];                                                                  \
    }                                                                                           \
    if (ga * ga > 1e-33 * al * be) {                                                            \
      const double ze = (be - al) / (2.0 * ga);                                                 \
      const double t = copysign(1.0, ze) / (fabs(ze) + sqrt(1.0 + ze * ze));                    \
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;                                      \
      _Pragma("unroll") for (int r = 0; r < 3; ++r) {                                           \
        const double gp = G[r][p], gq = G[r][q], vp = V[r][p], vq = V[r][q];                    \
        G[r][p] = c * gp - s * gq;                                                              \
        G[r][q] = s * gp + c * gq;                                                              \
        V[r][p] = c * vp - s * vq;                                                              \
        V[r][q] = s * vp + c * vq;                                                              \
      }                                                                                         \
    }                                                                                           \
  }

#define ARAP_SWAP(p, q)                                         \
  {                                                             \
    _Pragma("unroll") for (int r = 0; r < 3; ++r) {             \
      double t = G[r][p];                                       \
      G[r][p] = G[r][q];                                        \
      G[r][q] = t;                                              \
      t = V[r][p];                                              \
      V[r][p] = V[r][q];                                        \
      V[r][q] = t;                                              \
    }                                                           \
    const double t = n[p];                                      \
    n[p] = n[q];                                                \
    n[q] = t;                                                   \
  }

// a unit vector perpendicular to the unit vector a
A3D_DEV void arap_perp(const double a[3], double o[3]) {
  const double ax = fabs(a[0]), ay = fabs(a[1]), az = fabs(a[2]);
  double e[3] = {0.0, 0.0, 0.0};
  if (ax <= ay && ax <= az) e[0] = 1.0; else if (ay <= az) e[1] = 1.0; else e[2] = 1.0;
  o[0] = a[1] * e[2] - a[2] * e[1];
  o[1] = a[2] * e[0] - a[0] * e[2];
  o[2] = a[0] * e[1] - a[1] * e[0];
  const double inv = 1.0 / sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
  o[0] *= inv, o[1] *= inv, o[2] *= inv;
}

// R (row-major) = the proper rotation W U^T of M = U Sigma W^T; the identity for M = 0
A3D_DEV void arap_rotation(const double M[3][3], double R[9]) {
  double G[3][3], V[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      G[r][c] = M[r][c];
      V[r][c] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 12; ++sweep) {       // M V = G with orthogonal columns; quadratic convergence, 12 sweeps are ample for 3 x 3
    ARAP_ROT(0, 1)
    ARAP_ROT(0, 2)
    ARAP_ROT(1, 2)
  }
  double n[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) n[c] = G[0][c] * G[0][c] + G[1][c] * G[1][c] + G[2][c] * G[2][c];
  if (n[0] < n[2]) ARAP_SWAP(0, 2)                 // the smallest singular value to column 2, the largest to column 0
  if (n[1] < n[2]) ARAP_SWAP(1, 2)
  if (n[0] < n[1]) ARAP_SWAP(0, 1)
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
  if (!(n[0] > 0.0)) return;
  double u0[3], u1[3], w0[3], w1[3];
  const double i0 = 1.0 / sqrt(n[0]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    u0[r] = G[r][0] * i0;
    w0[r] = V[r][0];
  }
  if (n[1] > 0.0) {
    const double i1 = 1.0 / sqrt(n[1]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      u1[r] = G[r][1] * i1;
      w1[r] = V[r][1];
    }
  } else {                                         // rank 1: any rotation that maps u0 to w0 is a minimiser
    arap_perp(u0, u1);
    arap_perp(w0, w1);
  }
  const double u2[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
  const double w2[3] = {w0[1] * w1[2] - w0[2] * w1[1], w0[2] * w1[0] - w0[0] * w1[2], w0[0] * w1[1] - w0[1] * w1[0]};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = w0[r] * u0[c] + w1[r] * u1[c] + w2[r] * u2[c];
}

A3D_DEV void arap_load3(const float* p, int64_t v, float o[3]) {
  o[0] = p[3 * v], o[1] = p[3 * v + 1], o[2] = p[3 * v + 2];
}

__global__ __launch_bounds__(ARAP_BLOCK) void arap_energy_kernel(ArapArgs a, double* __restrict__ rot, float* __restrict__ rot_f32,
                                                                 double* __restrict__ energy) {
  const int p = blockIdx.x * ARAP_BLOCK + threadIdx.x;
  if (p >= a.F * a.S) return;
  const int f = p / a.S, s = p % a.S;
  const int v = a.sidx[s];
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double e = 0.0;
  if (v >= 0 && v < a.Nv) {
    const float* tg = a.tgt + (int64_t)f * a.tgt_bs;
    float sv[3], tv[3];
    arap_load3(a.src, v, sv);
    arap_load3(tg, v, tv);
    double M[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    bool same[3] = {true, true, true};
    for (int k = 0; k < a.K; ++k) {
      const int j = a.nn[(int64_t)v * a.K + k];
      const bool valid = j >= 0 && j < a.Nv;
      const double wk = a.w ? (double)a.w[(int64_t)v * a.K + k] : (valid ? 1.0 : 0.0);
      float sj[3] = {sv[0], sv[1], sv[2]}, tj[3] = {tv[0], tv[1], tv[2]};      // an absent edge is the zero vector
      if (valid) {
        arap_load3(a.src, j, sj);
        arap_load3(tg, j, tj);
      }
      double sd[3], td[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        same[c] = same[c] && (sv[c] - sj[c]) == (tv[c] - tj[c]);               // the fp32 edges, as the reference compares them
        sd[c] = (double)sv[c] - (double)sj[c];
        td[c] = (double)tv[c] - (double)tj[c];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r][c] += wk * sd[r] * td[c];
    }
    if (!(same[0] || same[1] || same[2])) arap_rotation(M, R);                 // util.py:156-157: S = 0, hence R = I
    for (int k = 0; k < a.K; ++k) {
      const int j = a.nn[(int64_t)v * a.K + k];
      const bool valid = j >= 0 && j < a.Nv;
      const double wk = a.w ? (double)a.w[(int64_t)v * a.K + k] : (valid ? 1.0 : 0.0);
      float sj[3] = {sv[0], sv[1], sv[2]}, tj[3] = {tv[0], tv[1], tv[2]};
      if (valid) {
        arap_load3(a.src, j, sj);
        arap_load3(tg, j, tj);
      }
      double sd[3], q = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) sd[c] = (double)sv[c] - (double)sj[c];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double d = ((double)tv[r] - (double)tj[r]) - (R[3 * r] * sd[0] + R[3 * r + 1] * sd[1] + R[3 * r + 2] * sd[2]);
        q += d * d;
      }
      e += wk * q;
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    rot[(int64_t)p * 9 + k] = R[k];
    if (rot_f32) rot_f32[(int64_t)p * 9 + k] = (float)R[k];
  }
  energy[p] = e;
}

__global__ __launch_bounds__(LR_BLOCK) void arap_reduce_kernel(const double* __restrict__ energy, int n, float* __restrict__ loss) {
  __shared__ double part[1][LR_BLOCK];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += LR_BLOCK) acc += energy[i];
  part[0][threadIdx.x] = acc;
  lr_tree(part);
  if (threadIdx.x == 0) loss[0] = (float)part[0][0];
}

// adds to acc the derivative of frame f's energy of sample s with respect to the vertex in slot c (0: the centre, k + 1: neighbour k)
template <bool SRC>
A3D_DEV void arap_bwd_entry(const ArapArgs& a, const double* __restrict__ rot, int f, int s, int c, double acc[3]) {
  const int v = a.sidx[s];
  if (v < 0 || v >= a.Nv) return;
  const float* tg = a.tgt + (int64_t)f * a.tgt_bs;
  const double* R = rot + ((int64_t)f * a.S + s) * 9;
  float sv[3], tv[3];
  arap_load3(a.src, v, sv);
  arap_load3(tg, v, tv);
  const int k0 = c == 0 ? 0 : c - 1, k1 = c == 0 ? a.K : c;
  const double sign = c == 0 ? 2.0 : -2.0;
  for (int k = k0; k < k1; ++k) {
    const int j = a.nn[(int64_t)v * a.K + k];
    if (j < 0 || j >= a.Nv) continue;
    const double wk = a.w ? (double)a.w[(int64_t)v * a.K + k] : 1.0;
    float sj[3], tj[3];
    arap_load3(a.src, j, sj);
    arap_load3(tg, j, tj);
    double sd[3], d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) sd[r] = (double)sv[r] - (double)sj[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = ((double)tv[r] - (double)tj[r]) - (R[3 * r] * sd[0] + R[3 * r + 1] * sd[1] + R[3 * r + 2] * sd[2]);
    if (SRC) {
#pragma unroll
      for (int r = 0; r < 3; ++r) acc[r] -= sign * wk * (R[r] * d[0] + R[3 + r] * d[1] + R[6 + r] * d[2]);
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r) acc[r] += sign * wk * d[r];
    }
  }
}

__global__ __launch_bounds__(KNN_BLOCK) void arap_bwd_kernel(ArapArgs a, const double* __restrict__ rot, const int* __restrict__ order,
                                                             const int* __restrict__ starts, const float* __restrict__ grad_out,
                                                             float* __restrict__ d_tgt, float* __restrict__ d_src) {
  const int v = blockIdx.x * KNN_BLOCK + threadIdx.x;
  const int f = blockIdx.y;
  if (v >= a.Nv) return;
  const int n = a.S * (a.K + 1);
  const int b = max(0, min(starts[v], n)), e = max(b, min(starts[v + 1], n));
  const double g = grad_out ? (double)grad_out[0] : 0.0;
  double acc[3] = {0.0, 0.0, 0.0};
  if (f < a.F) {
    for (int i = b; i < e; ++i) {
      const int ent = order[i];
      if (ent >= 0 && ent < n) arap_bwd_entry<false>(a, rot, f, ent / (a.K + 1), ent % (a.K + 1), acc);
    }
    float* o = d_tgt + ((int64_t)f * a.Nv + v) * 3;
    o[0] = (float)(g * acc[0]), o[1] = (float)(g * acc[1]), o[2] = (float)(g * acc[2]);
  } else {
    for (int ff = 0; ff < a.F; ++ff)
      for (int i = b; i < e; ++i) {
        const int ent = order[i];
        if (ent >= 0 && ent < n) arap_bwd_entry<true>(a, rot, ff, ent / (a.K + 1), ent % (a.K + 1), acc);
      }
    float* o = d_src + (int64_t)v * 3;
    o[0] = (float)(g * acc[0]), o[1] = (float)(g * acc[1]), o[2] = (float)(g * acc[2]);
  }
}

// Philox4x32-10 (Salmon et al., SC'11), as Random123 specifies it: ten rounds of
//   (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),
// the key raised by (W0, W1) between rounds.
A3D_DEV void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0], hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += W0;
    k1 += W1;
  }
}

// Row v of nn_idx: min(K, d) of the d entries col[row_start[v] ...] in ascending position, a uniformly random subset, then -1.
// Position p is kept iff mulhi32(r_p, d - p) < K - kept (so always while as many are needed as are left: a row with d <= K is copied);
// r_p is word p % 4 of the Philox block with key (seed lo, seed hi) and counter (v, p / 4, 0, 0).  A row_start outside [0, E] or
// descending is clamped: such a row is short, never out of bounds.
__global__ __launch_bounds__(256) void mesh_sample_kernel(int Nv, int E, const int* __restrict__ row_start, const int* __restrict__ col, int K,
                                                          const int64_t* __restrict__ seed, int* __restrict__ nn_idx) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= Nv) return;
  const int b = max(0, min(row_start[v], E)), e = max(b, min(row_start[v + 1], E));
  const int d = e - b;
  const uint64_t s = (uint64_t)seed[0];
  const uint32_t k0 = (uint32_t)s, k1 = (uint32_t)(s >> 32);
  int* out = nn_idx + (int64_t)v * K;
  int kept = 0;
  for (int q = 0; 4 * q < d && kept < K; ++q) {
    uint32_t r[4] = {(uint32_t)v, (uint32_t)q, 0u, 0u};
    if (d > K) philox4x32_10(k0, k1, r);               // a row that is copied whole draws nothing
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = 4 * q + j;
      if (p < d && kept < K && (d <= K || __umulhi(r[j], (uint32_t)(d - p)) < (uint32_t)(K - kept))) out[kept++] = col[b + p];
    }
  }
  for (; kept < K; ++kept) out[kept] = -1;
}

template <int K>
void knn_launch(hipStream_t st, int N, const float* pts, int Kout, int least, float r2, int* nn_idx, float* nn_dist) {
  knn_kernel<K><<<(N + KNN_BLOCK - 1) / KNN_BLOCK, KNN_BLOCK, 0, st>>>(N, pts, Kout, least, r2, nn_idx, nn_dist);
}

bool arap_args(ArapArgs& a, int F, int Nv, int K, int S, const float* src, const float* tgt, int64_t tgt_bs, const int* nn, const float* w,
               const int* sidx) {
  if (F <= 0 || Nv <= 0 || K <= 0 || S <= 0 || !src || !tgt || !nn || !sidx || tgt_bs < 0) return false;
  if ((int64_t)F * S > (int64_t)1 << 28 || (int64_t)S * (K + 1) > (int64_t)1 << 30 || F >= 65535) return false;
  if (!a3d_aligned(4, src, tgt, w) || !a3d_aligned(4, nn, sidx)) return false;
  a = ArapArgs{F, Nv, K, S, src, tgt, tgt_bs, nn, w, sidx};
  return true;
}

}  // namespace

extern "C" int a3d_knn_f32(a3d_stream_t stream, int N, const float* points, int K, int least_edge_num, float radius2, int* nn_idx,
                           float* nn_dist) {
  if (N <= 0 || !points || !nn_idx || !nn_dist || !a3d_aligned(4, points, nn_dist) || !a3d_aligned(4, nn_idx)) return A3D_EINVAL;
  if (K < 1 || K > 16) return A3D_EUNSUPPORTED;
  if (N <= K || least_edge_num < 0) return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  // the list length is rounded up to an instantiated one: the first K of the K' nearest are the K nearest
  if (K <= 1) knn_launch<1>(st, N, points, K, least_edge_num, radius2, nn_idx, nn_dist);
  else if (K <= 2) knn_launch<2>(st, N, points, K, least_edge_num, radius2, nn_idx, nn_dist);
  else if (K <= 3) knn_launch<3>(st, N, points, K, least_edge_num, radius2, nn_idx, nn_dist);
  else if (K <= 4) knn_launch<4>(st, N, points, K, least_edge_num, radius2, nn_idx, nn_dist);
  else if (K <= 6) knn_launch<6>(st, N, points, K, least_edge_num, radius2, nn_idx, nn_dist);
  else if (K <= 8) knn_launch<8>(st, N, points, K, least_edge_num, radius2, nn_idx, nn_dist);
  else if (K <= 10) knn_launch<10>(st, N, points, K, least_edge_num, radius2, nn_idx, nn_dist);
  else if (K <= 12) knn_launch<12>(st, N, points, K, least_edge_num, radius2, nn_idx, nn_dist);
  else knn_launch<16>(st, N, points, K, least_edge_num, radius2, nn_idx, nn_dist);
  return a3d_launch_status();
}

extern "C" int a3d_arap_energy_f32(a3d_stream_t stream, int F, int Nv, int K, int S, const float* source, const float* targets,
                                   int64_t targets_bs, const int* nn_idx, const float* weight, const int* sample_idx, double* rot,
                                   float* rot_f32, double* energy, float* loss) {
  ArapArgs a;
  if (!arap_args(a, F, Nv, K, S, source, targets, targets_bs, nn_idx, weight, sample_idx)) return A3D_EINVAL;
  if (!rot || !energy || !loss || !a3d_aligned(8, rot, energy) || !a3d_aligned(4, rot_f32, loss)) return A3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int n = F * S;
  arap_energy_kernel<<<(n + ARAP_BLOCK - 1) / ARAP_BLOCK, ARAP_BLOCK, 0, st>>>(a, rot, rot_f32, energy);
  arap_reduce_kernel<<<1, LR_BLOCK, 0, st>>>(energy, n, loss);
  return a3d_launch_status();
}

extern "C" int a3d_arap_backward_f32(a3d_stream_t stream, int F, int Nv, int K, int S, const float* source, const float* targets,
                                     int64_t targets_bs, const int* nn_idx, const float* weight, const int* sample_idx, const double* rot,
                                     const int* order, const int* starts, const float* grad_out, float* d_targets, float* d_source) {
  ArapArgs a;
  if (!arap_args(a, F, Nv, K, S, source, targets, targets_bs, nn_idx, weight, sample_idx)) return A3D_EINVAL;
  if (!rot || !order || !starts || !d_targets || !a3d_aligned(8, rot) || !a3d_aligned(4, grad_out, d_targets, d_source) ||
      !a3d_aligned(4, order, starts))
    return A3D_EINVAL;
  const dim3 grid((Nv + KNN_BLOCK - 1) / KNN_BLOCK, F + (d_source ? 1 : 0));
  arap_bwd_kernel<<<grid, KNN_BLOCK, 0, (hipStream_t)stream>>>(a, rot, order, starts, grad_out, d_targets, d_source);
  return a3d_launch_status();
}

extern "C" int a3d_mesh_sample_neighbours(a3d_stream_t stream, int Nv, int E, const int* row_start, const int* col, int K, const int64_t* seed,
                                          int* nn_idx) {
  if (Nv < 1 || E < 0 || !row_start || (!col && E > 0) || !seed || !nn_idx) return A3D_EINVAL;
  if (!a3d_aligned(4, row_start, col, nn_idx) || !a3d_aligned(8, seed)) return A3D_EINVAL;
  if (K < 1 || K > 16) return A3D_EUNSUPPORTED;
  mesh_sample_kernel<<<blocks_for(Nv), 256, 0, (hipStream_t)stream>>>(Nv, E, row_start, col, K, seed, nn_idx);
  return a3d_launch_status();
}
