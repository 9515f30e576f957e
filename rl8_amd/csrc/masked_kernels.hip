// Masked sequence ops of rl8.nn.functional (src/rl8/nn/functional.py:126-257) over padded sequences: pooling over the
// sequence dimension (masked_avg, masked_max), log-softmax and a categorical draw along the last dimension
// (masked_log_softmax, masked_categorical_sample), forward and backward.  `mask` is torch bool storage, nonzero = VALID,
// NULL = no mask.  Compiled with -ffp-contract=off: every reference operation rounds once.
//
// No kernel here declares LDS or a per-lane array (tests/test_nn_surface_host.py reads that off the metadata): the
// per-row kernels walk their row again instead of keeping it, and a row of K <= 64 floats stays in L1 between walks.
#include <float.h>

#include "common.hip.h"
#include "device_math.hip.h"
#include "wave_rows.hip.h"

namespace rl8 {
namespace {

// z_j = x_j + (valid ? 0 : -FLT_MAX): the float addition of x + clamp(log(mask), FINFO.min, FINFO.max).
struct MaskedRow {
  const float *x;
  const uint8_t *m;  // NULL: no mask
  __device__ __forceinline__ float operator()(int j) const {
    return m ? x[j] + (m[j] ? 0.0f : -FLT_MAX) : x[j];
  }
};

// ---- pooling over T ----------------------------------------------------------------------------------------------
// Lanes run over flattened (row, feature) pairs, the T loop inside the lane: a wave's loads of one t cover 64 / E runs
// of E floats T E apart, and over the loop every byte of the wave's rows is used, so x comes from HBM once.
template <class F>
__device__ __forceinline__ void for_each_pair(int64_t rows, int e, F &&f) {
  const int64_t total = rows * e;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const bool narrow = total <= 0x7fffffff;  // (wave-uniform: a 32-bit division where it is enough)
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
    const int64_t row = narrow ? (int64_t)((uint32_t)i / (uint32_t)e) : i / e;
    f(i, row, (int)(i - row * e));
  }
}

__global__ __launch_bounds__(kBlock) void masked_avg_kernel(const float *__restrict__ x, const uint8_t *__restrict__ mask,
                                                            int64_t rows, int t, int e, float *__restrict__ out) {
  for_each_pair(rows, e, [&](int64_t i, int64_t row, int f) {
    const float *xr = x + row * t * e + f;
    const uint8_t *mr = mask ? mask + row * t : nullptr;
    float sum = 0.0f;
    int count = 0;
    for (int j = 0; j < t; ++j) {
      const float v = xr[(int64_t)j * e];
      if (mr) {
        const int valid = mr[j] != 0;
        count += valid;
        sum = sum + (float)valid * v;  // (the product is formed: 0 * NaN and 0 * inf stay NaN, as mask * x)
      } else {
        sum = sum + v;
      }
    }
    out[i] = sum / (float)(mr ? count : t);
  });
}

__global__ __launch_bounds__(kBlock) void masked_avg_backward_kernel(const float *__restrict__ dout,
                                                                     const uint8_t *__restrict__ mask, int64_t rows, int t,
                                                                     int e, float *__restrict__ dx) {
  for_each_pair(rows, e, [&](int64_t i, int64_t row, int f) {
    float *dr = dx + row * t * e + f;
    const uint8_t *mr = mask ? mask + row * t : nullptr;
    int count = t;
    if (mr) {
      count = 0;
      for (int j = 0; j < t; ++j) count += mr[j] != 0;
    }
    const float g = dout[i] / (float)count;
    for (int j = 0; j < t; ++j) dr[(int64_t)j * e] = mr ? (float)(mr[j] != 0) * g : g;
  });
}

__global__ __launch_bounds__(kBlock) void masked_max_kernel(const float *__restrict__ x, const uint8_t *__restrict__ mask,
                                                            int64_t rows, int t, int e, float *__restrict__ out,
                                                            int64_t *__restrict__ index_out) {
  for_each_pair(rows, e, [&](int64_t i, int64_t row, int f) {
    const float *xr = x + row * t * e + f;
    const uint8_t *mr = mask ? mask + row * t : nullptr;
    float best = 0.0f;
    int at = 0;
    for (int j = 0; j < t; ++j) {
      const float v = (mr && !mr[j]) ? -FLT_MAX : xr[(int64_t)j * e];
      // torch.argmax: the first maximal cell, and a NaN is above everything (the first one stays)
      if (j == 0 || (best == best && (v > best || v != v))) {
        best = v;
        at = j;
      }
    }
    out[i] = best;
    index_out[i] = at;
  });
}

__global__ __launch_bounds__(kBlock) void masked_max_backward_kernel(const float *__restrict__ dout,
                                                                     const uint8_t *__restrict__ mask,
                                                                     const int64_t *__restrict__ index, int64_t rows, int t,
                                                                     int e, float *__restrict__ dx) {
  for_each_pair(rows, e, [&](int64_t i, int64_t row, int f) {
    float *dr = dx + row * t * e + f;
    const uint8_t *mr = mask ? mask + row * t : nullptr;
    const int64_t at = index[i];
    const float g = dout[i];
    // (gather's backward, then masked_fill's: nothing flows into a padded cell, chosen or not)
    for (int j = 0; j < t; ++j) dr[(int64_t)j * e] = (j == at && !(mr && !mr[j])) ? g : 0.0f;
  });
}

// ---- rows of K classes: one lane per row (K <= RL8_MAX_CLASSES) or one wave per row ---------------------------------
template <class F>
__device__ __forceinline__ void for_each_lane_row(int64_t rows, F &&f) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += stride) f(r);
}

// F.log_softmax as torch evaluates it: (z - max z) - log(sum exp(z - max z)).
__global__ __launch_bounds__(kBlock) void masked_log_softmax_lane_kernel(const float *__restrict__ x,
                                                                         const uint8_t *__restrict__ mask, int64_t rows,
                                                                         int k, float *__restrict__ out) {
  for_each_lane_row(rows, [&](int64_t r) {
    const MaskedRow z{x + r * k, mask ? mask + r * k : nullptr};
    float mx = z(0);
    for (int j = 1; j < k; ++j) {
      const float v = z(j);
      mx = v > mx ? v : mx;
    }
    float s = 0.0f;
    for (int j = 0; j < k; ++j) s = s + expf(z(j) - mx);
    const float ls = logf(s);
    for (int j = 0; j < k; ++j) out[r * k + j] = (z(j) - mx) - ls;
  });
}

__global__ __launch_bounds__(kBlock) void masked_log_softmax_wave_kernel(const float *__restrict__ x,
                                                                         const uint8_t *__restrict__ mask, int64_t rows,
                                                                         int k, float *__restrict__ out) {
  for_each_wave_row(rows, [&](int64_t r, int lane) {
    const MaskedRow z{x + r * k, mask ? mask + r * k : nullptr};
    float mx = -INFINITY;
    for (int j = lane; j < k; j += kWave) {
      const float v = z(j);
      mx = v > mx ? v : mx;
    }
    mx = wave_max(mx);
    float s = 0.0f;
    for (int j = lane; j < k; j += kWave) s = s + expf(z(j) - mx);
    const float ls = logf(wave_sum(s));
    for (int j = lane; j < k; j += kWave) out[r * k + j] = (z(j) - mx) - ls;
  });
}

// dx = dout - exp(out) * sum_k dout.
__global__ __launch_bounds__(kBlock) void masked_log_softmax_backward_lane_kernel(const float *__restrict__ dout,
                                                                                  const float *__restrict__ out,
                                                                                  int64_t rows, int k,
                                                                                  float *__restrict__ dx) {
  for_each_lane_row(rows, [&](int64_t r) {
    const float *g = dout + r * k, *o = out + r * k;
    float s = 0.0f;
    for (int j = 0; j < k; ++j) s = s + g[j];
    for (int j = 0; j < k; ++j) dx[r * k + j] = g[j] - expf(o[j]) * s;
  });
}

__global__ __launch_bounds__(kBlock) void masked_log_softmax_backward_wave_kernel(const float *__restrict__ dout,
                                                                                  const float *__restrict__ out,
                                                                                  int64_t rows, int k,
                                                                                  float *__restrict__ dx) {
  for_each_wave_row(rows, [&](int64_t r, int lane) {
    const float *g = dout + r * k, *o = out + r * k;
    float s = 0.0f;
    for (int j = lane; j < k; j += kWave) s = s + g[j];
    s = wave_sum(s);
    for (int j = lane; j < k; j += kWave) dx[r * k + j] = g[j] - expf(o[j]) * s;
  });
}

// One draw of Categorical(logits=z): argmax_j p_j / q_j, the first index on ties.  The arithmetic is
// categorical_normalise_dyn<true> (device_math.hip.h) followed by the loop of categorical_sample_kernel, operation for
// operation and in the same order, with the row read again where those keep it in an array: nl_j = z_j - lse,
// p_j = exp(nl_j - mx2) / s2.  mx2 = max_j nl_j is (max_j z_j) - lse because a rounded subtraction is monotone.
__device__ __forceinline__ float exp1_draw(const float *noise, int64_t r, int k, int j, uint64_t seed, uint64_t step,
                                           int64_t row_offset) {
  return noise ? noise[r * k + j] : rl8_exponential(seed, (uint64_t)(r + row_offset), step, (uint32_t)j);
}

__global__ __launch_bounds__(kBlock) void masked_sample_lane_kernel(const float *__restrict__ x,
                                                                    const uint8_t *__restrict__ mask,
                                                                    const float *__restrict__ noise, int64_t rows, int k,
                                                                    uint64_t seed, uint64_t step, int64_t row_offset,
                                                                    float *__restrict__ value_out,
                                                                    int64_t *__restrict__ index_out) {
  for_each_lane_row(rows, [&](int64_t r) {
    const MaskedRow z{x + r * k, mask ? mask + r * k : nullptr};
    float mx = z(0);
    for (int j = 1; j < k; ++j) {
      const float v = z(j);
      mx = v > mx ? v : mx;
    }
    float s = 0.0f;
    for (int j = 0; j < k; ++j) s += cr_expf(z(j) - mx);
    const float lse = mx + cr_logf(s);
    const float mx2 = mx - lse;
    float s2 = 0.0f;
    for (int j = 0; j < k; ++j) s2 += cr_expf((z(j) - lse) - mx2);
    int best = 0;
    float best_v = -INFINITY;
    for (int j = 0; j < k; ++j) {
      const float p = cr_expf((z(j) - lse) - mx2) / s2;
      const float v = p / exp1_draw(noise, r, k, j, seed, step, row_offset);
      if (v > best_v) {
        best_v = v;
        best = j;
      }
    }
    value_out[r] = z(best);
    index_out[r] = best;
  });
}

__global__ __launch_bounds__(kBlock) void masked_sample_wave_kernel(const float *__restrict__ x,
                                                                    const uint8_t *__restrict__ mask,
                                                                    const float *__restrict__ noise, int64_t rows, int k,
                                                                    uint64_t seed, uint64_t step, int64_t row_offset,
                                                                    float *__restrict__ value_out,
                                                                    int64_t *__restrict__ index_out) {
  for_each_wave_row(rows, [&](int64_t r, int lane) {
    const MaskedRow z{x + r * k, mask ? mask + r * k : nullptr};
    float mx = -INFINITY;
    for (int j = lane; j < k; j += kWave) {
      const float v = z(j);
      mx = v > mx ? v : mx;
    }
    mx = wave_max(mx);
    float s = 0.0f;
    for (int j = lane; j < k; j += kWave) s += cr_expf(z(j) - mx);
    const float lse = mx + cr_logf(wave_sum(s));
    const float mx2 = mx - lse;
    float s2 = 0.0f;
    for (int j = lane; j < k; j += kWave) s2 += cr_expf((z(j) - lse) - mx2);
    s2 = wave_sum(s2);
    int best = 0x7fffffff;  // (a lane that saw no finite ratio never beats one that did)
    float best_v = -INFINITY;
    for (int j = lane; j < k; j += kWave) {  // (ascending j within the lane: its first maximum)
      const float p = cr_expf((z(j) - lse) - mx2) / s2;
      const float v = p / exp1_draw(noise, r, k, j, seed, step, row_offset);
      if (v > best_v) {
        best_v = v;
        best = j;
      }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {  // the larger ratio, the smaller index on a tie: any order agrees
      const float ov = __shfl_xor(best_v, off, kWave);
      const int oj = __shfl_xor(best, off, kWave);
      if (ov > best_v || (ov == best_v && oj < best)) {
        best_v = ov;
        best = oj;
      }
    }
    if (best == 0x7fffffff) best = 0;  // (no ratio above -inf anywhere, e.g. NaN logits: class 0, as the lane route)
    if (lane == 0) {
      value_out[r] = z(best);
      index_out[r] = best;
    }
  });
}

inline bool aligned_to(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

}  // namespace
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_masked_rows_route(int k) {
  if (k < 1) return RL8_ESIZE;
  return k <= RL8_MAX_CLASSES ? RL8_MASKED_ROWS_LANE : RL8_MASKED_ROWS_WAVE;
}

// (rows kernels: 256 rows per block on the lane route, 4 on the wave route)
static int rows_grid(int64_t rows, int route) {
  return grid_for(rows, route == RL8_MASKED_ROWS_LANE ? kBlock : kWavesPerBlock);
}

RL8_API int rl8_masked_pool_f32(const float *x, const uint8_t *mask, int64_t rows, int t, int e, int mode, float *out,
                                int64_t *index_out, void *stream) {
  if (!x || !out || (mode == RL8_POOL_MAX && !index_out)) return RL8_ENULL;
  if (rows < 1 || t < 1 || e < 1) return RL8_ESIZE;
  if (mode != RL8_POOL_AVG && mode != RL8_POOL_MAX) return RL8_ECONFIG;
  if (!aligned_to(x, 4) || !aligned_to(out, 4) || (mode == RL8_POOL_MAX && !aligned_to(index_out, 8))) return RL8_EALIGN;
  const int grid = grid_for(rows * e, kBlock);
  if (mode == RL8_POOL_AVG)
    masked_avg_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(x, mask, rows, t, e, out);
  else
    masked_max_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(x, mask, rows, t, e, out, index_out);
  return launch_status();
}

RL8_API int rl8_masked_pool_backward_f32(const float *dout, const uint8_t *mask, const int64_t *index, int64_t rows, int t,
                                         int e, int mode, float *dx, void *stream) {
  if (!dout || !dx || (mode == RL8_POOL_MAX && !index)) return RL8_ENULL;
  if (rows < 1 || t < 1 || e < 1) return RL8_ESIZE;
  if (mode != RL8_POOL_AVG && mode != RL8_POOL_MAX) return RL8_ECONFIG;
  if (!aligned_to(dout, 4) || !aligned_to(dx, 4) || (mode == RL8_POOL_MAX && !aligned_to(index, 8))) return RL8_EALIGN;
  const int grid = grid_for(rows * e, kBlock);
  if (mode == RL8_POOL_AVG)
    masked_avg_backward_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(dout, mask, rows, t, e, dx);
  else
    masked_max_backward_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(dout, mask, index, rows, t, e, dx);
  return launch_status();
}

RL8_API int rl8_masked_log_softmax_f32(const float *x, const uint8_t *mask, int64_t rows, int k, float *out,
                                       void *stream) {
  if (!x || !out) return RL8_ENULL;
  if (rows < 1 || k < 1) return RL8_ESIZE;
  if (!aligned_to(x, 4) || !aligned_to(out, 4)) return RL8_EALIGN;
  const int route = rl8_masked_rows_route(k);
  if (route == RL8_MASKED_ROWS_LANE)
    masked_log_softmax_lane_kernel<<<rows_grid(rows, route), kBlock, 0, (hipStream_t)stream>>>(x, mask, rows, k, out);
  else
    masked_log_softmax_wave_kernel<<<rows_grid(rows, route), kBlock, 0, (hipStream_t)stream>>>(x, mask, rows, k, out);
  return launch_status();
}

RL8_API int rl8_masked_log_softmax_backward_f32(const float *dout, const float *out, int64_t rows, int k, float *dx,
                                                void *stream) {
  if (!dout || !out || !dx) return RL8_ENULL;
  if (rows < 1 || k < 1) return RL8_ESIZE;
  if (!aligned_to(dout, 4) || !aligned_to(out, 4) || !aligned_to(dx, 4)) return RL8_EALIGN;
  const int route = rl8_masked_rows_route(k);
  if (route == RL8_MASKED_ROWS_LANE)
    masked_log_softmax_backward_lane_kernel<<<rows_grid(rows, route), kBlock, 0, (hipStream_t)stream>>>(dout, out, rows,
                                                                                                        k, dx);
  else
    masked_log_softmax_backward_wave_kernel<<<rows_grid(rows, route), kBlock, 0, (hipStream_t)stream>>>(dout, out, rows,
                                                                                                        k, dx);
  return launch_status();
}

RL8_API int rl8_masked_categorical_sample_f32(const float *x, const uint8_t *mask, const float *noise, int64_t rows, int k,
                                              uint64_t seed, uint64_t step, int64_t row_offset, float *value_out,
                                              int64_t *index_out, void *stream) {
  if (!x || !value_out || !index_out) return RL8_ENULL;
  if (rows < 1 || k < 1) return RL8_ESIZE;
  if (!aligned_to(x, 4) || !aligned_to(noise, 4) || !aligned_to(value_out, 4) || !aligned_to(index_out, 8))
    return RL8_EALIGN;
  const int route = rl8_masked_rows_route(k);
  if (route == RL8_MASKED_ROWS_LANE)
    masked_sample_lane_kernel<<<rows_grid(rows, route), kBlock, 0, (hipStream_t)stream>>>(
        x, mask, noise, rows, k, seed, step, row_offset, value_out, index_out);
  else
    masked_sample_wave_kernel<<<rows_grid(rows, route), kBlock, 0, (hipStream_t)stream>>>(
        x, mask, noise, rows, k, seed, step, row_offset, value_out, index_out);
  return launch_status();
}
