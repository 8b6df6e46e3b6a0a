// The one reduction of the 4-D stage's scalar losses (recon_loss.hip, stage_reg.hip, arap.hip): their summation order is written down here
// and pinned by tests/test_loss_reduce_gpu.py.  No atomics anywhere, so two calls are bitwise equal.  For K sums at once:
//   1. a thread of a forward kernel adds its run in fp32, in the order its kernel visits it (that part is the kernel's own);
//   2. lr_block_partials: the block's accumulators go through lr_tree in fp32; thread 0 stores sum k of block j at partials[k * n_partials + j];
//   3. lr_final_sums, in one block: thread t adds partials[k * n_partials + i] for i = t, t + LR_BLOCK, ... in fp64, then lr_tree in fp64
//      leaves sum k in red[k][0], for thread 0 to use.
// lr_tree halves: for h = 128, 64, ..., 1, thread t < h does red[k][t] += red[k][t + h].  It stays an LDS tree: a DPP, __shfl or wave-level
// reduction adds in another order and changes result bits.  Nothing here is launched: including this adds no kernel to a code object.
#pragma once
#include "common.h"

namespace {  // one copy per translation unit, like the kernels of the files that include this

constexpr int LR_BLOCK = 256;

// red[k][0] = the sum of red[k][0 .. LR_BLOCK); every thread of the LR_BLOCK-wide block calls it after writing its column
template <int K, typename T>
A3D_DEV void lr_tree(T (&red)[K][LR_BLOCK]) {
  __syncthreads();
  for (int h = LR_BLOCK / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + h];
    }
    __syncthreads();
  }
}

template <int K>
A3D_DEV void lr_block_partials(const float (&acc)[K], float (&red)[K][LR_BLOCK], float* __restrict__ partials, int64_t n_partials) {
#pragma unroll
  for (int k = 0; k < K; ++k) red[k][threadIdx.x] = acc[k];
  lr_tree(red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) partials[k * n_partials + blockIdx.x] = red[k][0];
  }
}

template <int K>
A3D_DEV void lr_final_sums(const float* __restrict__ partials, int64_t n_partials, double (&red)[K][LR_BLOCK]) {
  double s[K] = {};
  for (int64_t i = threadIdx.x; i < n_partials; i += LR_BLOCK) {     // the K loads of a step are independent: all in flight at once
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += (double)partials[k * n_partials + i];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) red[k][threadIdx.x] = s[k];
  lr_tree(red);
}

}  // namespace
