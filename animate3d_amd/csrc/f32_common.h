// Shared by the fp32 4-D stage (splat.hip, deform4d.hip, arap.hip): the grid-size helper and the one reduction their atomic-free backward passes have
// in common.  Math helpers stay in their files: two spellings of one formula round differently.  A file that includes this gets the kernel
// in its code object, so only files that launch it do; arap.hip takes blocks_for from here and carries the kernel unlaunched.
#pragma once
#include "common.h"

namespace {  // one copy per translation unit, like the kernels of the files that include this

inline unsigned blocks_for(int64_t n, int block = 256) { return (unsigned)((n + block - 1) / block); }

// dst[k] = src[0][k] + src[1][k] + ... + src[rows - 1][k] for src [rows, M], in that order: bit-reproducible
__global__ __launch_bounds__(256) void sum_leading_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int64_t M) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= M) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += src[r * M + k];
  dst[k] = s;
}

inline void sum_leading(hipStream_t st, const float* src, float* dst, int rows, int64_t M) {
  sum_leading_kernel<<<blocks_for(M), 256, 0, st>>>(src, dst, rows, M);
}

}  // namespace
