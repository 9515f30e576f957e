// Host-side launch layer of the width-256 tower kernels (mlp_kernels.hip, mlp_f16_kernels.hip, mlp_rows_kernels.hip,
// mlp_split_kernels.hip): the grid cap, the grids of the fused backward, the segment walk of the weight-gradient
// entries, the run-time width -> compiled variant dispatch, and the functions one of these units calls in another.
// Nothing here runs on the device.
#pragma once

#include <limits.h>

#include <type_traits>

#include "split_tile.hip.h"

namespace rl8 {

// ---- grids --------------------------------------------------------------------------------------------------------------
// Workgroups of a tile kernel: RL8_MLP_GRID_CAP (tuning and tests; read once per process), else two per CU.
inline int tower_grid_cap() {
  static const int cap = env_int("RL8_MLP_GRID_CAP");
  return cap > 0 ? cap : 2 * kCUs;
}
inline int tower_grid(int64_t m, int tile_rows) { return grid_for(m, tile_rows, tower_grid_cap()); }

// A launch of a weight-gradient kernel covers at most kWgradSegmentRows samples; longer inputs are summed segment by
// segment (dW2 through the slab reduction's accumulate mode, the head-gradient partial rows in place).  Every accumulator
// is an fp32 chain over its workgroup's share of the samples: at 2^25 rows in one launch dW2 was 7e-5 (of its largest
// entry) off an fp64 evaluation, at 2^23 per launch 4e-5 -- the length the parity tests were validated at, kept whatever
// the caller's pass size.
constexpr int64_t kWgradSegmentRows = (int64_t)1 << 23;
constexpr int kWsChunk = 16;  // samples per k-step of the weight-gradient kernels

// One workgroup per CU owns the whole 256 x 256 output and a strided share of the 16-sample chunks.
inline int wgrad_grid(int64_t rows) { return grid_for(rows, kWsChunk, kCUs); }

// The two halves of the fused backward -- the data gradient on g1 workgroups, the weight gradient on g2 -- each zero the
// partial-row segments the other does not cover, so both take their grids from here, from m alone.
struct BackwardGrids {
  int g1, g2;
  int partial_rows() const { return g1 > g2 ? g1 : g2; }
};
inline BackwardGrids backward_grids(int64_t m) { return {tower_grid(m, kSplitRows), wgrad_grid(m)}; }

// ---- the segments of a weight-gradient call ---------------------------------------------------------------------------------
struct WgradSegment {
  int64_t at, rows;  // first row and row count
  int grid;
  bool later;  // not the first segment: the callee adds to what the earlier ones left
};

constexpr int kWgradGatesMinRows = 128;  // four gates per launch: eight chunks per gate at the least

// f(segment) for each segment of m rows in order, until one returns non-zero (returned).  The first segment runs
// wgrad_grid(its rows) workgroups -- backward_grids(m).g2 -- and a later one no more than the first, since it adds to the
// first one's slabs and rows.  groups == 4 (the LSTM's four gates in one launch): a quarter of the workgroups per gate, in
// multiples of 8, and RL8_ESIZE before any segment runs if one of them is too short for that.
template <class F>
inline int for_each_wgrad_segment(int64_t m, int groups, F &&f) {
  if (groups == 4 && (m - 1) % kWgradSegmentRows + 1 < kWgradGatesMinRows) return RL8_ESIZE;  // (the last one is the shortest)
  int first_grid = 0;
  for (int64_t at = 0; at < m; at += kWgradSegmentRows) {
    const int64_t rows = m - at < kWgradSegmentRows ? m - at : kWgradSegmentRows;
    int grid = wgrad_grid(rows);
    if (groups == 4) grid = grid_for(rows, kWsChunk, kCUs / 4) / 8 * 8 * 4;  // (each gate's share <= its chunks)
    if (at == 0) first_grid = grid;
    if (grid > first_grid) grid = first_grid;
    if (const int status = f(WgradSegment{at, rows, grid, at > 0})) return status;
  }
  return RL8_OK;
}

// ---- run-time width -> compiled variant -----------------------------------------------------------------------------------
template <int... W>
struct Widths {};

constexpr int kNoVariant = INT_MIN;  // no ABI status (RL8_E* are -1 .. -4) and no hipError_t

// f(std::integral_constant<int, W>) for the W of the list that equals `width`; kNoVariant if none does.
template <int... W, class F>
inline int dispatch_width(int width, Widths<W...>, F &&f) {
  int status = kNoVariant;
  (void)((width == W ? (status = f(std::integral_constant<int, W>{}), true) : false) || ...);
  return status;
}
// The same for kernels that also take their width at run time (variant 0): every width outside the list runs that one.
template <int... W, class F>
inline int dispatch_width_or_runtime(int width, Widths<W...> list, F &&f) {
  const int status = dispatch_width(width, list, f);
  return status == kNoVariant ? f(std::integral_constant<int, 0>{}) : status;
}
// What an entry point returns for it: the width checks in front of a dispatch keep it from happening.
inline int variant_status(int status) { return status == kNoVariant ? RL8_ESIZE : status; }

// ---- across the units -----------------------------------------------------------------------------------------------------
// mlp_rows_kernels.hip, called by the entry points of mlp_f16_kernels.hip.  The two data-gradient dispatchers return
// kNoVariant where the rows-per-wave kernels have no variant (the caller keeps the tile kernel or rejects the width).
int rows_in_class(int d_in);
int rows_out_class(int n_out);
int mlp_rows_forward_dispatch(hipStream_t s, const float *x, int64_t m, int d_in, const float *w1, const float *b1,
                              const void *w2s, const float *b2, const float *w3, const float *b3, int n_out, float *out,
                              float *h1, float *h2, uint32_t *gate);
int mlp_rows_backward_gate_dispatch(int grid, hipStream_t s, const float *x, const float *w1, const float *b1, const float *dout,
                                    int64_t m, int d_in, const void *w2ts, int n_out, float *partials, int stride, int head_rows,
                                    const uint32_t *gate2);
int mlp_rows_backward_general_dispatch(int grid, hipStream_t s, const float *x, const float *w1, const float *b1, const float *dout,
                                       int64_t m, int d_in, const void *w2ts, const float *w3, int n_out, float *partials, int stride,
                                       int head_rows, const uint32_t *gate2);

}  // namespace rl8
