// One row of the narrow recurrent models' output heads: out[q] = h[row] . w[q] for h [H], H = 64 or 128, as every
// kernel that evaluates them forms it (linear_heads_narrow_forward_kernel, single and pair form, and
// rollout_step_dummy_heads_narrow_kernel), so that the three agree bit for bit.
//
// Four lanes per row.  Lane q4 takes the 16-byte pieces q4, q4 + 4, .. of the row (the four lanes of a row read 64
// contiguous bytes per load) and runs one fma chain per output over them in piece order; two lane exchanges then add
// the four chains.  The arithmetic and its order for one output depend on H alone: not on the number of outputs, not
// on which array a weight row came from.  The weights are broadcast from LDS, [NOUT][H] as float4.
#pragma once

#include "common.hip.h"

namespace rl8 {
namespace narrow_heads {

constexpr int kMaxOut = 8;

// ws [NOUT][H / 4] <- the first n_a rows from w_a, the rest from w_b (n_a = NOUT: one layer).
template <int H>
__device__ __forceinline__ void stage_weights(float4 *ws, int n_out, const float *__restrict__ w_a, int n_a,
                                              const float *__restrict__ w_b) {
  for (int i = threadIdx.x; i < n_out * (H / 4); i += kBlock)
    ws[i] = i < n_a * (H / 4) ? reinterpret_cast<const float4 *>(w_a)[i]
                              : reinterpret_cast<const float4 *>(w_b)[i - n_a * (H / 4)];
}

// hrow: the row's H floats; every one of the row's four lanes leaves with the whole sums (no bias).
template <int H, int NOUT>
__device__ __forceinline__ void row_dots(const float4 *__restrict__ hrow, const float4 *ws, int q4, float (&o)[NOUT]) {
  static_assert(H == 64 || H == 128, "narrow heads: H = 64 or 128");
#pragma unroll
  for (int q = 0; q < NOUT; ++q) o[q] = 0.0f;
#pragma unroll
  for (int i = 0; i < H / 16; ++i) {
    const float4 v = hrow[q4 + 4 * i];
#pragma unroll
    for (int q = 0; q < NOUT; ++q) {
      const float4 wv = ws[q * (H / 4) + q4 + 4 * i];
      o[q] = __builtin_fmaf(v.x, wv.x, o[q]);
      o[q] = __builtin_fmaf(v.y, wv.y, o[q]);
      o[q] = __builtin_fmaf(v.z, wv.z, o[q]);
      o[q] = __builtin_fmaf(v.w, wv.w, o[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < NOUT; ++q) {
    o[q] += __shfl_xor(o[q], 1, kWave);
    o[q] += __shfl_xor(o[q], 2, kWave);
  }
}

}  // namespace narrow_heads
}  // namespace rl8
