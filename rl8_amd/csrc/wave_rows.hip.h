// One wave per row: the cross-lane reductions and the row walk shared by the masked sequence kernels
// (masked_kernels.hip) and the wide categorical kernels (categorical_wide_kernels.hip).
#pragma once

#include "common.hip.h"

namespace rl8 {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const float o = __shfl_xor(v, off, kWave);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {  // (a xor butterfly: the same tree, hence the same bits, in every lane)
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off, kWave);
  return v;
}

template <class F>
__device__ __forceinline__ void for_each_wave_row(int64_t rows, F &&f) {  // (the row is the same in all 64 lanes)
  const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; r < rows; r += stride)
    f(r, (int)(threadIdx.x & (kWave - 1)));
}

}  // namespace rl8
