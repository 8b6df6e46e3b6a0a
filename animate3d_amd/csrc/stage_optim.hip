// The optimiser step of the 4-D stage for gfx950: Adam over a table of fp32 tensors, each with its own rate and its own step count, that
// leaves everything untouched when a gradient holds an inf or a NaN (contract in animate3d_amd/stage_optim.py and include/animate3d_hip.h).
// The table travels as kernel arguments: the gradients' addresses change every step, and nothing is copied to the device to say so.
//   flag_reset_kernel     one thread: flag = 0
//   grad_finite_kernel    a block per SA_CHUNK elements of one tensor's gradient; a thread that meets an inf or a NaN stores flag = 1.
//                         Every writer stores the same value: which one comes last does not matter, and nobody reads it as a count
//   adam_update_kernel    the same blocks; all of them return at once where flag != 0.  Else the element's p, m, v, g are loaded as fp32
//                         and the step is taken in fp64 without contraction, u from the unrounded m' and v'; p', m', v' are rounded to
//                         fp32 once each.  The tensor's step is only read here: k = step + 1
//   step_advance_kernel   a thread per tensor: step += 1 where flag == 0.  A launch of its own, so that no block of the update reads a
//                         step that another block of its launch has written
// Four launches at most, whatever the number of tensors; 4-byte accesses, consecutive threads on consecutive elements.
#include "f32_common.h"

#include <math.h>

namespace {

constexpr int SA_THREADS = 256;
constexpr int SA_PER_THREAD = 4;
constexpr int SA_CHUNK = SA_THREADS * SA_PER_THREAD;     // elements of one tensor per block

struct SaTable {                                         // by value in the kernel arguments: 32 x 56 + 33 x 4 + 4 bytes of the 4 096 there are
  a3d_stage_adam_entry e[A3D_STAGE_ADAM_MAX_TENSORS];
  unsigned first_block[A3D_STAGE_ADAM_MAX_TENSORS + 1];  // tensor t owns blocks first_block[t] .. first_block[t + 1] - 1
  int count;
};

// The tensor that owns this block, and the block's first element in it.  A walk over at most 32 kernel-argument words, the same for
// every thread of the block.
A3D_DEV int owner_of(const SaTable& tab, unsigned block, int64_t& base) {
  int t = 0;
  while (t + 1 < tab.count && block >= tab.first_block[t + 1]) ++t;
  base = (int64_t)(block - tab.first_block[t]) * SA_CHUNK;
  return t;
}

__global__ void flag_reset_kernel(int* __restrict__ flag) { *flag = 0; }

__global__ __launch_bounds__(SA_THREADS) void grad_finite_kernel(const SaTable tab, int* __restrict__ flag) {
  int64_t base;
  const int t = owner_of(tab, blockIdx.x, base);
  const uint32_t* __restrict__ g = reinterpret_cast<const uint32_t*>(tab.e[t].g);
  const int64_t n = tab.e[t].n;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < SA_PER_THREAD; ++j) {
    const int64_t i = base + j * SA_THREADS + threadIdx.x;
    if (i < n) bad |= (g[i] & 0x7f800000u) == 0x7f800000u;          // every exponent bit set: inf or NaN
  }
  if (bad) *flag = 1;
}

__global__ __launch_bounds__(SA_THREADS) void adam_update_kernel(const SaTable tab, double beta1, double beta2, double eps,
                                                                 const int* __restrict__ flag) {
#pragma clang fp contract(off)
  if (*flag != 0) return;
  int64_t base;
  const int t = owner_of(tab, blockIdx.x, base);
  __shared__ double scale[2];                             // lr / (1 - beta1^k) and sqrt(1 - beta2^k): once per block
  if (threadIdx.x == 0) {
    const double k = (double)*tab.e[t].step + 1.0;
    scale[0] = tab.e[t].lr / (1.0 - pow(beta1, k));
    scale[1] = sqrt(1.0 - pow(beta2, k));
  }
  __syncthreads();
  const double step_size = scale[0], bc2_sqrt = scale[1];
  float* __restrict__ P = tab.e[t].p;
  float* __restrict__ M = tab.e[t].m;
  float* __restrict__ V = tab.e[t].v;
  const float* __restrict__ G = tab.e[t].g;
  const int64_t n = tab.e[t].n;
#pragma unroll
  for (int j = 0; j < SA_PER_THREAD; ++j) {
    const int64_t i = base + j * SA_THREADS + threadIdx.x;
    if (i >= n) continue;
    const double g = G[i], m = M[i], v = V[i], p = P[i];
    const double m1 = beta1 * m + (1.0 - beta1) * g;
    const double v1 = beta2 * v + (1.0 - beta2) * (g * g);
    const double u = step_size * m1 / (sqrt(v1) / bc2_sqrt + eps);
    P[i] = (float)(p - u);
    M[i] = (float)m1;
    V[i] = (float)v1;
  }
}

__global__ void step_advance_kernel(const SaTable tab, const int* __restrict__ flag) {
  const int t = threadIdx.x;
  if (t < tab.count && *flag == 0) *tab.e[t].step += 1.0f;
}

}  // namespace

extern "C" int a3d_stage_adam_f32(a3d_stream_t stream, const a3d_stage_adam_entry* table, int count, double beta1, double beta2, double eps,
                                  int phases, int* flag) {
  if (!table || count < 1 || count > A3D_STAGE_ADAM_MAX_TENSORS || !flag || !a3d_aligned(4, flag)) return A3D_EINVAL;
  if (phases < 1 || phases > (A3D_STAGE_ADAM_BEGIN | A3D_STAGE_ADAM_CHECK | A3D_STAGE_ADAM_UPDATE)) return A3D_EINVAL;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !isfinite(eps)) return A3D_EINVAL;
  SaTable tab;
  uint64_t blocks = 0;
  for (int t = 0; t < count; ++t) {
    const a3d_stage_adam_entry& e = table[t];
    if (!e.p || !e.g || !e.m || !e.v || !e.step || !a3d_aligned(4, e.p, e.g, e.m, e.v, e.step)) return A3D_EINVAL;
    if (e.n < 1 || !(e.lr >= 0.0) || !isfinite(e.lr)) return A3D_EINVAL;
    tab.e[t] = e;
    tab.first_block[t] = (unsigned)blocks;
    blocks += ((uint64_t)e.n + SA_CHUNK - 1) / SA_CHUNK;
    if (blocks > 0x7fffffffull) return A3D_EINVAL;       // a grid's x extent
  }
  for (int t = count; t < A3D_STAGE_ADAM_MAX_TENSORS; ++t) tab.e[t] = a3d_stage_adam_entry{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0.0};
  for (int t = count; t <= A3D_STAGE_ADAM_MAX_TENSORS; ++t) tab.first_block[t] = (unsigned)blocks;
  tab.count = count;
  hipStream_t st = (hipStream_t)stream;
  if (phases & A3D_STAGE_ADAM_BEGIN) flag_reset_kernel<<<1, 1, 0, st>>>(flag);
  if (phases & A3D_STAGE_ADAM_CHECK) grad_finite_kernel<<<(unsigned)blocks, SA_THREADS, 0, st>>>(tab, flag);
  if (phases & A3D_STAGE_ADAM_UPDATE) {
    adam_update_kernel<<<(unsigned)blocks, SA_THREADS, 0, st>>>(tab, beta1, beta2, eps, flag);
    step_advance_kernel<<<1, A3D_STAGE_ADAM_MAX_TENSORS, 0, st>>>(tab, flag);
  }
  return a3d_launch_status();
}
