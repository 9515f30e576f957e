// Device helpers shared by the fp32-MFMA attention units (attention_wide_kernels.hip, attention_long_kernels.hip): LDS
// tiles of 16 rows by 16 NF feature columns at a row pitch of 16 NF + 4 floats, a strip's own rows as B operands, the two
// products of the transposed-score layout, and the score masks.
//
// v_mfma_f32_16x16x4_f32: D[16][16] += A[16][4] B[4][16], lane l holding A[l % 16][l / 16], B[l / 16][l % 16] and
// D[4 (l / 16) + r][l % 16] in accumulator register r.
#pragma once

#include <math.h>

#include "common.hip.h"

namespace rl8 {
namespace attention_tiles {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kStrip = 16;  // rows of a wave's strip, and of an MFMA tile

// Row pitch of an LDS tile of 16 NF feature columns: pitch / 4 is odd, so row-major reads (16 rows x 4 columns per
// instruction) and permuted reads (4 rows x 16 columns) both touch 64 different banks.
constexpr int pitch_of(int nf) { return 16 * nf + 4; }

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ bool aligned16_dev(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// rows x d floats at src (row stride `stride`) -> dst [rows_p][PITCH], zeros in rows >= rows and columns d .. 16 NF.
template <int NF>
__device__ __forceinline__ void stage_rows(float *__restrict__ dst, const float *__restrict__ src, int64_t stride, int rows,
                                           int rows_p, int d) {
  constexpr int kPitch = pitch_of(NF), kCols = 16 * NF;
  if (aligned16_dev(src) && (stride & 3) == 0 && (d & 3) == 0) {  // (wave-uniform)
    for (int i = threadIdx.x; i < rows_p * (kCols / 4); i += blockDim.x) {
      const int r = i / (kCols / 4), c = 4 * (i - r * (kCols / 4));
      f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
      if (r < rows && c < d) x = *reinterpret_cast<const f32x4 *>(src + r * stride + c);
      *reinterpret_cast<f32x4 *>(dst + r * kPitch + c) = x;
    }
  } else {
    for (int i = threadIdx.x; i < rows_p * kCols; i += blockDim.x) {
      const int r = i / kCols, c = i - r * kCols;
      dst[r * kPitch + c] = (r < rows && c < d) ? src[r * stride + c] : 0.0f;
    }
  }
}

// A strip's own rows as B operands: x[c] = row (l % 16), feature 4 c + l / 16, zero outside the strip's rows and D.
template <int NF>
__device__ __forceinline__ void load_fragment(const float *__restrict__ row, bool live, int grp, int d, float (&x)[4 * NF]) {
#pragma unroll
  for (int c = 0; c < 4 * NF; ++c) x[c] = (live && 4 * c + grp < d) ? row[4 * c + grp] : 0.0f;
}

// acc[16 x 16] = tile[16 rows][16 NF] . x: rows of the LDS tile along the accumulator's rows.
template <int NF>
__device__ __forceinline__ f32x4 rows_times_fragment(const float *__restrict__ tile_lane, const float (&x)[4 * NF]) {
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < 4 * NF; ++c) acc = mfma(tile_lane[4 * c], x[c], acc);
  return acc;
}

// acc[f] (16 features x 16 columns) += tile^T . w, w = accumulator registers of a [16 rows x 16 columns] tile: register
// r contracts rows 4 g + r, which is the order the A operand is read in.
template <int NF>
__device__ __forceinline__ void transposed_times_tile(const float *__restrict__ tile_perm, const f32x4 &w,
                                                      f32x4 (&acc)[NF]) {
  constexpr int kPitch = pitch_of(NF);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = mfma(tile_perm[r * kPitch + 16 * f], w[r], acc[f]);
}

__device__ __forceinline__ float across_groups_max(float x) {
  const float y = fmaxf(x, __shfl_xor(x, 16, kWave));
  return fmaxf(y, __shfl_xor(y, 32, kWave));
}
__device__ __forceinline__ float across_groups_sum(float x) {
  const float y = x + __shfl_xor(x, 16, kWave);
  return y + __shfl_xor(y, 32, kWave);
}

// Which (batch, head, group of `per_group` strips) a workgroup works on.
struct Item {
  int64_t batch;
  int h, first_strip;
  __device__ __forceinline__ Item(int64_t item, int heads, int groups, int per_group = 4) {
    const int64_t bh = item / groups;
    first_strip = per_group * (int)(item - bh * groups);
    batch = bh / heads;
    h = (int)(bh - batch * heads);
  }
};

// The padding bytes of keys 4 w .. 4 w + 3 as one word, a key >= tk padded.
__device__ __forceinline__ uint32_t padding_word(const uint8_t *__restrict__ padded, int w, int tk) {
  uint32_t word = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key = 4 * w + j;
    if (key >= tk || (padded && padded[key])) word |= 0xffu << (8 * j);
  }
  return word;
}

// The padding bytes of a head's keys as LDS words, word w = keys 4 w .. 4 w + 3.
__device__ __forceinline__ void stage_padding(uint32_t *__restrict__ words, const uint8_t *__restrict__ padded, int tk,
                                              int tkp) {
  for (int w = threadIdx.x; w < tkp / 4; w += blockDim.x) words[w] = padding_word(padded, w, tk);
}

// The four scores of one accumulator, keys key0 .. key0 + 3 of query qi: scale, bias, -inf at a padded key.
__device__ __forceinline__ f32x4 finish_scores(f32x4 s, float scale, const float *__restrict__ bias_row, bool live,
                                               int key0, int tk, uint32_t pad_word) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float x = scale * s[r];
    if (bias_row) x = x + ((live && key0 + r < tk) ? bias_row[key0 + r] : 0.0f);
    s[r] = ((pad_word >> (8 * r)) & 0xffu) ? -INFINITY : x;
  }
  return s;
}

// delta = dout . out of the lane's query on the matrix cores, as the diagonal of out dO^T from the two rows' B-operand
// fragments: the same instructions in the same order as dP = V dO^T, so that where P sits on one key -- out = v --
// dP - delta is exactly 0 instead of the difference of two roundings.
template <int NF>
__device__ __forceinline__ float diagonal_dot(const float (&of)[4 * NF], const float (&gf)[4 * NF], int col) {
  f32x4 dt = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < 4 * NF; ++c) dt = mfma(of[c], gf[c], dt);
  const int r = col & 3;  // row `col` of column `col`: register col % 4 of the lane in group col / 4
  const float diagonal = r == 0 ? dt[0] : r == 1 ? dt[1] : r == 2 ? dt[2] : dt[3];
  return __shfl(diagonal, col + 16 * (col >> 2), kWave);
}

inline bool aligned_to(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// One instantiation per count of 16-feature tiles: f.template operator()<NF>().
template <class F>
inline int with_feature_tiles(int d, F &&f) {
  switch ((d + 15) / 16) {
    case 1: return f.template operator()<1>();
    case 2: return f.template operator()<2>();
    case 3: return f.template operator()<3>();
    default: return f.template operator()<4>();
  }
}

}  // namespace attention_tiles
}  // namespace rl8
