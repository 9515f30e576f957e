// The last launch of both feedforward families' backward (feedforward_kernels.hip, feedforward_wide_kernels.hip): the
// partial rows their kernels left in the workspace, added in fp64 in a fixed order.
#pragma once

#include "common.hip.h"

namespace rl8 {
namespace {

constexpr int kSumSplit = 16;         // row interleaves of the final sum
constexpr int kSumElems = kBlock / kSumSplit;

// The outputs of the final sum: element e of a partial row of `row_floats` belongs to the one whose range holds it.
struct SumTargets {
  float *dw1, *db1, *dw2, *db2;  // each may be NULL: not written
  float *dgamma, *dbeta;
};

// out[e] = sum over partial rows, rows kSumSplit apart in ascending order in fp64, the kSumSplit sums then in order.
__global__ __launch_bounds__(kBlock) void feedforward_sum_kernel(const float *__restrict__ w_partials, int w_rows,
                                                               const float *__restrict__ ln_partials, int ln_rows,
                                                               int f, int hidden, SumTargets to) {
  __shared__ double part[kSumSplit][kSumElems];
  const int w_floats = 2 * f * hidden + hidden + f;
  const int e = blockIdx.x * kSumElems + threadIdx.x % kSumElems, split = threadIdx.x / kSumElems;
  const bool is_w = e < w_floats, is_ln = !is_w && e < w_floats + 2 * f;
  const float *src = is_w ? w_partials : ln_partials;  // (NULL: that half is not wanted)
  const int at = is_w ? e : e - w_floats;
  const int count = !src ? 0 : is_w ? w_rows : is_ln ? ln_rows : 0;
  const int64_t pitch = is_w ? w_floats : 2 * f;
  double s = 0.0;
#pragma unroll 8  // (loads in the air together; the additions stay in row order)
  for (int r = split; r < count; r += kSumSplit) s = s + (double)src[r * pitch + at];
  part[split][threadIdx.x % kSumElems] = s;
  __syncthreads();
  if (split != 0 || !(is_w || is_ln)) return;
#pragma unroll
  for (int q = 1; q < kSumSplit; ++q) s = s + part[q][threadIdx.x];
  float *dst;
  if (e < f * hidden) dst = to.dw1 ? to.dw1 + e : nullptr;
  else if (e < f * hidden + hidden) dst = to.db1 ? to.db1 + (e - f * hidden) : nullptr;
  else if (e < 2 * f * hidden + hidden) dst = to.dw2 ? to.dw2 + (e - f * hidden - hidden) : nullptr;
  else if (e < w_floats) dst = to.db2 ? to.db2 + (e - 2 * f * hidden - hidden) : nullptr;
  else if (e < w_floats + f) dst = to.dgamma ? to.dgamma + (e - w_floats) : nullptr;
  else dst = to.dbeta ? to.dbeta + (e - w_floats - f) : nullptr;
  if (dst) *dst = (float)s;
}

// Floats of one partial row, laid out as the outputs are: dW1 [H][F], db1 [H], dW2 [F][H], db2 [F].
inline int64_t wgrad_row_floats(int f, int hidden) { return 2 * (int64_t)f * hidden + hidden + f; }

}  // namespace
}  // namespace rl8
