// The feedforward block of feedforward_kernels.hip for what that file leaves: rows of 33 <= F <= 128 features through
// 1 <= H <= 512 hidden units, fp32, on the matrix cores, forward and backward.  Compiled with -ffp-contract=off and
// without packed fp32 VALU instructions.
//   n   = LayerNorm_F(x; gamma, beta, eps)         biased variance from the centred values, rstd = 1 / sqrt(var + eps)
//   out = (residual ? x : 0) + W2 relu(W1 n + b1) + b2
// The operand and error contract is feedforward_kernels.hip's, clause for clause: x [R][F] dense, W1 [H][F], W2 [F][H],
// pointers 4-byte aligned and no more, the backward from x and dout alone, every backward output optional, no atomics.
//
// v_mfma_f32_16x16x4_f32: D[16][16] += A[16][4] B[4][16], lane l holding A[l % 16][l / 16], B[l / 16][l % 16] and
// D[4 (l / 16) + r][l % 16] in accumulator register r.  Below col = l % 16, grp = l / 16.
//
// Token tile.  A workgroup of four waves owns 64 tokens, a strip of 16 per wave; F is padded to 16 NF with zeros, NF
// (3 .. 8) a template parameter.  A lane holds its token's (token = col) features {4 c + grp : c < 4 NF} -- four lanes
// per row -- which is the B operand of a product over features as it stands.  LayerNorm runs on that fragment: sums
// over c in the lane, then over the four 16-lane groups by two xor exchanges (every lane of a token ends with the same
// bits); layer_norm_fragment is the ONE place n is formed, for every kernel here.
//
// Transposed products.  z^T = W1 n^T with hidden units along the accumulator's rows (A: rows of W1 from LDS, B: the
// fragment), b1 as the accumulator's initial value, ReLU on the accumulators; register r of a z^T tile IS the B operand
// of out^T += W2 a^T for the four hidden units {4 grp + r}, so the A operand (columns of W2) is read in that permuted
// order and the activations never leave the registers.  out^T (NF tiles, b2 as the initial value) stays in registers
// over the loop over H.  dx: z^T again by the forward's instructions in the forward's order (same tiles, same k order,
// so every gate has the forward's bits), da^T = W2^T dout^T (B: the strip's dout fragment), dz^T on the accumulators,
// dn^T += W1^T dz^T by the same accumulator-as-B trick; LayerNorm's backward per token from dn in accumulator layout
// (x read again in that layout, sums over registers, then over the four groups); the wave's sums of dn xhat and dn
// (dgamma, dbeta) over its tokens go to one partial row per wave.
//
// Weights through LDS in chunks of 32 hidden units, both as [32][16 NF + 4]: W1[chunk][F] as it lies, W2[F][chunk]
// transposed on the way in, zeros beyond F and H.  Pitch / 4 is odd, so the reads (row col, column 4 c + grp) and
// (row 4 grp + r, column 16 f + col) both touch 64 different banks.  Two buffers: chunk k + 1 is staged while chunk k
// is multiplied, one barrier per chunk, and the four strips share what was read from L2 once.  LDS per workgroup,
// forward and dx (4 x 32 x pitch + 64 floats): 26 880 B at NF = 3, 35 072 (4), 43 264 (5), 51 456 (6), 59 648 (7),
// 67 840 (8).
//
// Weight gradients: products over TOKENS.  One workgroup per (chunk of 32 hidden units, slice of the 64-token tiles:
// tile = slice, slice + slices, ...), its chunk of W1 and W2 staged once.  Deviation from the transposed form above:
// here z = n W1^T is formed with the TOKENS along the accumulator's rows (A: the n fragment, B: W1 from LDS -- the
// forward's factors with the operands swapped, in the forward's k order), because then register r of z, a and dz is
// the B operand of dW1^T += n^T dz and dW2 += dout^T a for the tokens {4 grp + r} as it stands, and only n and dout go
// through LDS (a [16][pitch] tile each per wave, written as fragments, read in the permuted token order).  Every
// wave keeps its own accumulators over its whole slice and writes one partial row (slice 4 + wave), laid out as the
// outputs are; feedforward_sum_kernel (feedforward_sum.hip.h, shared with the narrow family) adds the partial rows in
// fp64 in a fixed order.  LDS ((64 + 128) x pitch + 32 floats): 40 064 B at NF = 3, 52 352, 64 640, 76 928, 89 216,
// 101 504 at NF = 8.
#include <math.h>

#include "common.hip.h"
#include "feedforward_sum.hip.h"

namespace rl8 {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWideMinF = 33;
constexpr int kWideMaxF = 128;
constexpr int kWideMaxHidden = 512;
constexpr int kStrip = 16;                       // tokens of a wave's strip, and rows of an MFMA tile
constexpr int kTile = kStrip * kWavesPerBlock;   // tokens of a workgroup's tile
constexpr int kChunk = 32;                       // hidden units staged at a time
constexpr int kChunkTiles = kChunk / kStrip;
constexpr int kWideMaxGrid = 1024;               // forward and dx: 4 workgroups per CU, grid-stride beyond
constexpr int kWideWgradMaxGrid = 256;           // chunks x slices: one workgroup per CU

constexpr int pitch_of(int nf) { return 16 * nf + 4; }
inline int chunks_of(int hidden) { return (hidden + kChunk - 1) / kChunk; }
inline int64_t tiles_of(int64_t rows) { return (rows + kTile - 1) / kTile; }
inline int forward_lds_bytes(int nf) { return (4 * kChunk * pitch_of(nf) + 2 * kChunk) * (int)sizeof(float); }
inline int wgrad_lds_bytes(int nf) {
  return ((2 * kChunk + 2 * kTile) * pitch_of(nf) + kChunk) * (int)sizeof(float);
}
// Slices of the weight-gradient kernels' tiles: a function of the shape only.
inline int wgrad_slices(int64_t rows, int hidden) {
  const int64_t tiles = tiles_of(rows), cap = kWideWgradMaxGrid / chunks_of(hidden);
  return (int)(tiles < cap ? tiles : cap);
}

struct Relu {
  // NaN goes through, as torch.relu's; -0 becomes +0.
  __device__ __forceinline__ static float apply(float z) { return !(z <= 0.0f) ? z : 0.0f; }
  // torch's gate: closed at exactly 0.
  __device__ __forceinline__ static float gate(float z, float da) { return z > 0.0f ? da : 0.0f; }
};

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float across_groups_sum(float x) {
  const float y = x + __shfl_xor(x, 16, kWave);
  return y + __shfl_xor(y, 32, kWave);
}

// The sum over the 16 lanes of a group (every lane of the group ends with the same bits).
__device__ __forceinline__ float across_columns_sum(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x = x + __shfl_xor(x, off, kWave);
  return x;
}

// Hidden units j0 .. j0 + 31 into LDS: w1s[j][c] = W1[j0 + j][c], w2s[j][c] = W2[c][j0 + j], b1s[j] = b1[j0 + j], zeros
// for a unit >= hidden and a feature >= f (columns 16 NF .. pitch are never read).
template <int NF>
__device__ __forceinline__ void stage_chunk(float *__restrict__ w1s, float *__restrict__ w2s, float *__restrict__ b1s,
                                            const float *__restrict__ w1, const float *__restrict__ b1,
                                            const float *__restrict__ w2, int j0, int f, int hidden) {
  constexpr int kPitch = pitch_of(NF), kCols = 16 * NF;
  for (int i = threadIdx.x; i < kChunk * kCols; i += kBlock) {
    const int j = i / kCols, c = i - j * kCols;
    w1s[j * kPitch + c] = (j0 + j < hidden && c < f) ? w1[(j0 + j) * f + c] : 0.0f;
  }
  for (int i = threadIdx.x; i < kChunk * kCols; i += kBlock) {
    const int c = i / kChunk, j = i - c * kChunk;
    w2s[j * kPitch + c] = (j0 + j < hidden && c < f) ? w2[c * hidden + j0 + j] : 0.0f;
  }
  if (threadIdx.x < kChunk) b1s[threadIdx.x] = j0 + (int)threadIdx.x < hidden ? b1[j0 + threadIdx.x] : 0.0f;
}

// A token's row as a fragment: v[c] = row[4 c + grp], zero for a token past the rows and a feature >= f.
template <int NF>
__device__ __forceinline__ void load_fragment(const float *__restrict__ row, bool live, int grp, int f,
                                              float (&v)[4 * NF]) {
#pragma unroll
  for (int c = 0; c < 4 * NF; ++c) v[c] = (live && 4 * c + grp < f) ? row[4 * c + grp] : 0.0f;
}

struct Moments {
  float mean, rstd;
};

// xhat = (x - mean) rstd of one element, the ONE place it is formed (fragment and accumulator layout alike).
__device__ __forceinline__ float normalised(float x, Moments m) { return (x - m.mean) * m.rstd; }

// n of the lane's fragment of x (in: x, zero where there is none; out: n, zero at a feature >= f), the variance from
// the centred values.  A token past the rows has x = 0 and n = beta: finite, and it meets dout = 0 everywhere.
template <int NF>
__device__ __forceinline__ Moments layer_norm_fragment(float (&v)[4 * NF], int grp, int f,
                                                       const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, float eps) {
  const float inv_f = 1.0f / (float)f;
  float sum = 0.0f;
#pragma unroll
  for (int c = 0; c < 4 * NF; ++c) sum = sum + v[c];
  Moments m;
  m.mean = across_groups_sum(sum) * inv_f;
  float var = 0.0f;
#pragma unroll
  for (int c = 0; c < 4 * NF; ++c) {
    const float d = 4 * c + grp < f ? v[c] - m.mean : 0.0f;
    var = fmaf(d, d, var);
  }
  m.rstd = 1.0f / sqrtf(across_groups_sum(var) * inv_f + eps);
#pragma unroll
  for (int c = 0; c < 4 * NF; ++c) {
    const int feature = 4 * c + grp;
    v[c] = feature < f ? fmaf(normalised(v[c], m), gamma[feature], beta[feature]) : 0.0f;
  }
  return m;
}

// acc[16 x 16] += tile[16 rows][16 NF] . x: rows of the LDS tile along the accumulator's rows, x a fragment.
template <int NF>
__device__ __forceinline__ f32x4 rows_times_fragment(const float *__restrict__ tile_lane, const float (&x)[4 * NF],
                                                     f32x4 acc) {
#pragma unroll
  for (int c = 0; c < 4 * NF; ++c) acc = mfma(tile_lane[4 * c], x[c], acc);
  return acc;
}

// The same product with the operands swapped: the fragment's tokens along the accumulator's rows.
template <int NF>
__device__ __forceinline__ f32x4 fragment_times_rows(const float (&x)[4 * NF], const float *__restrict__ tile_lane,
                                                     f32x4 acc) {
#pragma unroll
  for (int c = 0; c < 4 * NF; ++c) acc = mfma(x[c], tile_lane[4 * c], acc);
  return acc;
}

// acc[f] (16 features x 16 columns) += tile^T . w, w = accumulator registers of a [16 rows x 16 columns] tile: register
// r contracts rows 4 grp + r, which is the order the A operand is read in.
template <int NF>
__device__ __forceinline__ void transposed_times_tile(const float *__restrict__ tile_perm, const f32x4 &w,
                                                      f32x4 (&acc)[NF]) {
  constexpr int kPitch = pitch_of(NF);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = mfma(tile_perm[r * kPitch + 16 * f], w[r], acc[f]);
}

// z^T of hidden units 16 t .. 16 t + 15 of the staged chunk for the strip whose n is `nf`: register r = unit 4 grp + r.
template <int NF>
__device__ __forceinline__ f32x4 pre_activation_tile(const float *__restrict__ w1c, const float *__restrict__ b1c, int t,
                                                     int col, int grp, const float (&nf)[4 * NF]) {
  const float *b = b1c + 16 * t + 4 * grp;
  return rows_times_fragment<NF>(w1c + (16 * t + col) * pitch_of(NF) + grp, nf, f32x4{b[0], b[1], b[2], b[3]});
}

template <int NF>
__global__ __launch_bounds__(kBlock) void feedforward_wide_forward_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
    const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2,
    const float *__restrict__ b2, int64_t rows, int f, int hidden, int residual, float *__restrict__ out) {
  constexpr int kPitch = pitch_of(NF), kBuffer = kChunk * kPitch;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *w1s = lds, *w2s = lds + 2 * kBuffer, *b1s = lds + 4 * kBuffer;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, col = lane & 15, grp = lane >> 4;
  const int chunks = (hidden + kChunk - 1) / kChunk;
  const int64_t tiles = (rows + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t token = tile * kTile + wave * kStrip + col;
    const bool strip = token - col < rows, live = token < rows;  // (strip: wave-uniform)
    const float *xrow = x + (live ? token : 0) * f;
    float nf[4 * NF];
    load_fragment<NF>(xrow, live, grp, f, nf);
    layer_norm_fragment<NF>(nf, grp, f, gamma, beta, eps);
    f32x4 acc[NF];
#pragma unroll
    for (int t = 0; t < NF; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int feature = 16 * t + 4 * grp + r;
        acc[t][r] = feature < f ? b2[feature] : 0.0f;
      }
    stage_chunk<NF>(w1s, w2s, b1s, w1, b1, w2, 0, f, hidden);
    __syncthreads();
    for (int k = 0; k < chunks; ++k) {
      const int at = k & 1, next = at ^ 1;
      if (k + 1 < chunks)
        stage_chunk<NF>(w1s + next * kBuffer, w2s + next * kBuffer, b1s + next * kChunk, w1, b1, w2, (k + 1) * kChunk, f,
                        hidden);
      if (strip) {
#pragma unroll
        for (int t = 0; t < kChunkTiles; ++t) {
          f32x4 a = pre_activation_tile<NF>(w1s + at * kBuffer, b1s + at * kChunk, t, col, grp, nf);
#pragma unroll
          for (int r = 0; r < 4; ++r) a[r] = Relu::apply(a[r]);
          transposed_times_tile<NF>(w2s + at * kBuffer + (16 * t + 4 * grp) * kPitch + col, a, acc);
        }
      }
      __syncthreads();  // (chunk k has been read, chunk k + 1 is in place)
    }
    if (live) {
      float *orow = out + token * f;
#pragma unroll
      for (int t = 0; t < NF; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int feature = 16 * t + 4 * grp + r;
          if (feature < f) orow[feature] = residual ? xrow[feature] + acc[t][r] : acc[t][r];
        }
    }
  }
}

// dx of the tile's tokens from x and dout; with LN, the wave's sums of dn xhat (dgamma) and dn (dbeta) over all its
// tokens to ln_partials[(block 4 + wave)][2 f] as well.  dx may be NULL when only those are wanted.
template <int NF, bool LN>
__global__ __launch_bounds__(kBlock) void feedforward_wide_backward_x_kernel(
    const float *__restrict__ x, const float *__restrict__ dout, const float *__restrict__ gamma,
    const float *__restrict__ beta, float eps, const float *__restrict__ w1, const float *__restrict__ b1,
    const float *__restrict__ w2, int64_t rows, int f, int hidden, int residual, float *__restrict__ dx,
    float *__restrict__ ln_partials) {
  constexpr int kPitch = pitch_of(NF), kBuffer = kChunk * kPitch;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *w1s = lds, *w2s = lds + 2 * kBuffer, *b1s = lds + 4 * kBuffer;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, col = lane & 15, grp = lane >> 4;
  const int chunks = (hidden + kChunk - 1) / kChunk;
  const int64_t tiles = (rows + kTile - 1) / kTile;
  const float inv_f = 1.0f / (float)f;
  f32x4 sg[LN ? NF : 1], sb[LN ? NF : 1];
#pragma unroll
  for (int t = 0; t < (LN ? NF : 1); ++t) sg[t] = sb[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t token = tile * kTile + wave * kStrip + col;
    const bool strip = token - col < rows, live = token < rows;
    const float *xrow = x + (live ? token : 0) * f, *grow = dout + (live ? token : 0) * f;
    float nf[4 * NF], gf[4 * NF];
    load_fragment<NF>(xrow, live, grp, f, nf);
    load_fragment<NF>(grow, live, grp, f, gf);
    const Moments m = layer_norm_fragment<NF>(nf, grp, f, gamma, beta, eps);
    f32x4 dn[NF];
#pragma unroll
    for (int t = 0; t < NF; ++t) dn[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    stage_chunk<NF>(w1s, w2s, b1s, w1, b1, w2, 0, f, hidden);
    __syncthreads();
    for (int k = 0; k < chunks; ++k) {
      const int at = k & 1, next = at ^ 1;
      if (k + 1 < chunks)
        stage_chunk<NF>(w1s + next * kBuffer, w2s + next * kBuffer, b1s + next * kChunk, w1, b1, w2, (k + 1) * kChunk, f,
                        hidden);
      if (strip) {
#pragma unroll
        for (int t = 0; t < kChunkTiles; ++t) {
          const f32x4 z = pre_activation_tile<NF>(w1s + at * kBuffer, b1s + at * kChunk, t, col, grp, nf);
          f32x4 dz = rows_times_fragment<NF>(w2s + at * kBuffer + (16 * t + col) * kPitch + grp, gf,
                                             f32x4{0.0f, 0.0f, 0.0f, 0.0f});
#pragma unroll
          for (int r = 0; r < 4; ++r) dz[r] = Relu::gate(z[r], dz[r]);
          transposed_times_tile<NF>(w1s + at * kBuffer + (16 * t + 4 * grp) * kPitch + col, dz, dn);
        }
      }
      __syncthreads();
    }
    if (strip) {
      // dx = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)), dxhat = dn gamma, in accumulator layout: register r of
      // tile t is feature 16 t + 4 grp + r of token col.  A token past the rows and a feature >= f have dn = 0.
      f32x4 xhat[NF];
      float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
      for (int t = 0; t < NF; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int feature = 16 * t + 4 * grp + r;
          const bool here = live && feature < f;
          xhat[t][r] = here ? normalised(xrow[feature], m) : 0.0f;
          if constexpr (LN) {
            sg[t][r] = fmaf(dn[t][r], xhat[t][r], sg[t][r]);
            sb[t][r] = sb[t][r] + dn[t][r];
          }
          dn[t][r] = here ? dn[t][r] * gamma[feature] : 0.0f;
          m1 = m1 + dn[t][r];
          m2 = fmaf(dn[t][r], xhat[t][r], m2);
        }
      m1 = across_groups_sum(m1) * inv_f;
      m2 = across_groups_sum(m2) * inv_f;
      if (dx && live) {
        float *orow = dx + token * f;
#pragma unroll
        for (int t = 0; t < NF; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int feature = 16 * t + 4 * grp + r;
            const float d = m.rstd * ((dn[t][r] - m1) - xhat[t][r] * m2);
            if (feature < f) orow[feature] = residual ? grow[feature] + d : d;
          }
      }
    }
  }
  if constexpr (LN) {
    // (every wave is back here, also one that had no strip: it adds 0)
    float *p = ln_partials + ((int64_t)blockIdx.x * kWavesPerBlock + wave) * (2 * f);
#pragma unroll
    for (int t = 0; t < NF; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int feature = 16 * t + 4 * grp + r;
        const float g = across_columns_sum(sg[t][r]), b = across_columns_sum(sb[t][r]);
        if (col == 0 && feature < f) {
          p[feature] = g;
          p[f + feature] = b;
        }
      }
  }
}

// dW1, db1, dW2 of hidden units chunk 32 .. chunk 32 + 31 (and db2 where chunk = 0) summed over the tokens of the
// workgroup's slice, one partial row per wave at partials[(slice 4 + wave)], laid out as the outputs are.
template <int NF>
__global__ __launch_bounds__(kBlock) void feedforward_wide_wgrad_kernel(
    const float *__restrict__ x, const float *__restrict__ dout, const float *__restrict__ gamma,
    const float *__restrict__ beta, float eps, const float *__restrict__ w1, const float *__restrict__ b1,
    const float *__restrict__ w2, int64_t rows, int f, int hidden, int chunks, int slices,
    float *__restrict__ partials) {
  constexpr int kPitch = pitch_of(NF), kBuffer = kChunk * kPitch;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, col = lane & 15, grp = lane >> 4;
  float *w1s = lds, *w2s = lds + kBuffer, *ns = lds + 2 * kBuffer + wave * kStrip * kPitch;
  float *gs = ns + kTile * kPitch, *b1s = lds + 2 * kBuffer + 2 * kTile * kPitch;
  const int chunk = blockIdx.x % chunks, slice = blockIdx.x / chunks, j0 = chunk * kChunk;
  const int64_t tiles = (rows + kTile - 1) / kTile;
  stage_chunk<NF>(w1s, w2s, b1s, w1, b1, w2, j0, f, hidden);
  // dw1[t][u], dw2[t][u]: register r = feature 16 t + 4 grp + r of hidden unit j0 + 16 u + col
  f32x4 dw1[NF][kChunkTiles], dw2[NF][kChunkTiles];
  float db1[kChunkTiles], db2[NF];
#pragma unroll
  for (int t = 0; t < NF; ++t) {
    db2[t] = 0.0f;
#pragma unroll
    for (int u = 0; u < kChunkTiles; ++u) dw1[t][u] = dw2[t][u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
#pragma unroll
  for (int u = 0; u < kChunkTiles; ++u) db1[u] = 0.0f;
  for (int64_t tile = slice; tile < tiles; tile += slices) {  // (the same trip count for the whole workgroup)
    const int64_t token = tile * kTile + wave * kStrip + col;
    const bool strip = token - col < rows, live = token < rows;
    float nf[4 * NF], gf[4 * NF];
    load_fragment<NF>(x + (live ? token : 0) * f, live, grp, f, nf);
    load_fragment<NF>(dout + (live ? token : 0) * f, live, grp, f, gf);
    layer_norm_fragment<NF>(nf, grp, f, gamma, beta, eps);
#pragma unroll
    for (int c = 0; c < 4 * NF; ++c) {
      ns[col * kPitch + 4 * c + grp] = nf[c];
      gs[col * kPitch + 4 * c + grp] = gf[c];
    }
    __syncthreads();  // (the weights on the first trip; the strip's n and dout for the lanes that read them)
    if (strip) {
      // tokens along the accumulator's rows: register r = token 4 grp + r of the strip, hidden unit 16 u + col
      f32x4 a[kChunkTiles], dz[kChunkTiles];
#pragma unroll
      for (int u = 0; u < kChunkTiles; ++u) {
        const float b = b1s[16 * u + col];
        const f32x4 z = fragment_times_rows<NF>(nf, w1s + (16 * u + col) * kPitch + grp, f32x4{b, b, b, b});
        const f32x4 da = fragment_times_rows<NF>(gf, w2s + (16 * u + col) * kPitch + grp,
                                                 f32x4{0.0f, 0.0f, 0.0f, 0.0f});
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          a[u][r] = Relu::apply(z[r]);
          dz[u][r] = Relu::gate(z[r], da[r]);
          db1[u] = db1[u] + dz[u][r];
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < NF; ++t) {
          const float n_t = ns[(4 * grp + r) * kPitch + 16 * t + col];  // feature 16 t + col of token 4 grp + r
          const float g_t = gs[(4 * grp + r) * kPitch + 16 * t + col];
          db2[t] = db2[t] + g_t;
#pragma unroll
          for (int u = 0; u < kChunkTiles; ++u) {
            dw1[t][u] = mfma(n_t, dz[u][r], dw1[t][u]);
            dw2[t][u] = mfma(g_t, a[u][r], dw2[t][u]);
          }
        }
    }
    __syncthreads();  // (the next trip writes over what this one reads)
  }
  float *p = partials + ((int64_t)slice * kWavesPerBlock + wave) * (2 * (int64_t)f * hidden + hidden + f);
#pragma unroll
  for (int u = 0; u < kChunkTiles; ++u) {
    const int j = j0 + 16 * u + col;
    const float s = across_groups_sum(db1[u]);
    if (j < hidden) {
      if (grp == 0) p[f * hidden + j] = s;
#pragma unroll
      for (int t = 0; t < NF; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int feature = 16 * t + 4 * grp + r;
          if (feature < f) {
            p[j * f + feature] = dw1[t][u][r];
            p[f * hidden + hidden + feature * hidden + j] = dw2[t][u][r];
          }
        }
    }
  }
#pragma unroll
  for (int t = 0; t < NF; ++t) {
    const float s = across_groups_sum(db2[t]);
    if (chunk == 0 && grp == 0 && 16 * t + col < f) p[2 * f * hidden + hidden + 16 * t + col] = s;
  }
}

inline bool aligned_to(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// One instantiation per count of 16-feature tiles, 3 .. 8: fn.template operator()<NF>().
template <class Fn>
inline int with_feature_tiles(int f, Fn &&fn) {
  switch ((f + 15) / 16) {
    case 3: return fn.template operator()<3>();
    case 4: return fn.template operator()<4>();
    case 5: return fn.template operator()<5>();
    case 6: return fn.template operator()<6>();
    case 7: return fn.template operator()<7>();
    default: return fn.template operator()<8>();
  }
}

inline int wide_grid(int64_t rows) { return grid_for(rows, kTile, kWideMaxGrid); }

struct WideForwardLaunch {
  const float *x, *gamma, *beta;
  float eps;
  const float *w1, *b1, *w2, *b2;
  int64_t rows;
  int f, hidden, residual;
  float *out;
  hipStream_t stream;
  template <int NF>
  int operator()() const {
    const int bytes = forward_lds_bytes(NF);
    if (const int e = allow_dynamic_lds<&feedforward_wide_forward_kernel<NF>>(bytes)) return e;
    feedforward_wide_forward_kernel<NF><<<wide_grid(rows), kBlock, bytes, stream>>>(
        x, gamma, beta, eps, w1, b1, w2, b2, rows, f, hidden, residual, out);
    return launch_status();
  }
};

struct WideBackwardLaunch {
  const float *x, *dout, *gamma, *beta;
  float eps;
  const float *w1, *b1, *w2;
  int64_t rows;
  int f, hidden, residual;
  float *dx;
  SumTargets to;
  float *workspace;
  hipStream_t stream;
  template <int NF>
  int operator()() const {
    const bool want_ln = to.dgamma || to.dbeta, want_w = to.dw1 || to.db1 || to.dw2 || to.db2;
    const int x_grid = wide_grid(rows), chunks = chunks_of(hidden), slices = wgrad_slices(rows, hidden);
    const int w_rows = slices * kWavesPerBlock, bytes = forward_lds_bytes(NF);
    float *ln_partials = workspace ? workspace + w_rows * wgrad_row_floats(f, hidden) : nullptr;
    if (const int e = allow_dynamic_lds<&feedforward_wide_backward_x_kernel<NF, true>>(bytes)) return e;
    if (const int e = allow_dynamic_lds<&feedforward_wide_backward_x_kernel<NF, false>>(bytes)) return e;
    if (const int e = allow_dynamic_lds<&feedforward_wide_wgrad_kernel<NF>>(wgrad_lds_bytes(NF))) return e;
    if (want_ln)
      feedforward_wide_backward_x_kernel<NF, true><<<x_grid, kBlock, bytes, stream>>>(
          x, dout, gamma, beta, eps, w1, b1, w2, rows, f, hidden, residual, dx, ln_partials);
    else if (dx)
      feedforward_wide_backward_x_kernel<NF, false><<<x_grid, kBlock, bytes, stream>>>(
          x, dout, gamma, beta, eps, w1, b1, w2, rows, f, hidden, residual, dx, nullptr);
    if (want_w)
      feedforward_wide_wgrad_kernel<NF><<<chunks * slices, kBlock, wgrad_lds_bytes(NF), stream>>>(
          x, dout, gamma, beta, eps, w1, b1, w2, rows, f, hidden, chunks, slices, workspace);
    if (want_w || want_ln) {
      const int elems = (int)wgrad_row_floats(f, hidden) + 2 * f;
      feedforward_sum_kernel<<<(elems + kSumElems - 1) / kSumElems, kBlock, 0, stream>>>(
          want_w ? workspace : nullptr, w_rows, want_ln ? ln_partials : nullptr, x_grid * kWavesPerBlock, f, hidden, to);
    }
    return launch_status();
  }
};

}  // namespace
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_feedforward_wide_supports(int f, int hidden) {
  if (f < 1 || hidden < 1) return RL8_ESIZE;
  return f >= kWideMinF && f <= kWideMaxF && hidden <= kWideMaxHidden ? 1 : 0;
}

RL8_API int rl8_feedforward_wide_limits(int *limits) {
  if (!limits) return RL8_ENULL;
  limits[0] = kTile;
  limits[1] = kWideMaxGrid;
  limits[2] = kWideWgradMaxGrid;
  limits[3] = kChunk;
  return RL8_OK;
}

RL8_API int64_t rl8_feedforward_wide_workspace_floats(int64_t rows, int f, int hidden) {
  if (rows < 1 || f < 1 || hidden < 1) return RL8_ESIZE;
  if (rl8_feedforward_wide_supports(f, hidden) != 1) return RL8_ECONFIG;
  return (int64_t)wgrad_slices(rows, hidden) * kWavesPerBlock * wgrad_row_floats(f, hidden) +
         (int64_t)wide_grid(rows) * kWavesPerBlock * 2 * f;
}

RL8_API int rl8_feedforward_wide_f32(const float *x, const float *gamma, const float *beta, float eps, const float *w1,
                                     const float *b1, const float *w2, const float *b2, int64_t rows, int f, int hidden,
                                     int residual, float *out, void *stream) {
  if (!x || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !out) return RL8_ENULL;
  if (rows < 1 || f < 1 || hidden < 1) return RL8_ESIZE;
  if (!aligned_to(x, 4) || !aligned_to(gamma, 4) || !aligned_to(beta, 4) || !aligned_to(w1, 4) || !aligned_to(b1, 4) ||
      !aligned_to(w2, 4) || !aligned_to(b2, 4) || !aligned_to(out, 4))
    return RL8_EALIGN;
  if (rl8_feedforward_wide_supports(f, hidden) != 1) return RL8_ECONFIG;
  return with_feature_tiles(f, WideForwardLaunch{x, gamma, beta, eps, w1, b1, w2, b2, rows, f, hidden, residual != 0,
                                                 out, (hipStream_t)stream});
}

RL8_API int rl8_feedforward_wide_backward_f32(const float *x, const float *dout, const float *gamma, const float *beta,
                                              float eps, const float *w1, const float *b1, const float *w2,
                                              int64_t rows, int f, int hidden, int residual, float *dx, float *dgamma,
                                              float *dbeta, float *dw1, float *db1, float *dw2, float *db2,
                                              float *workspace, void *stream) {
  const bool want_params = dgamma || dbeta || dw1 || db1 || dw2 || db2;
  if (!x || !dout || !gamma || !beta || !w1 || !b1 || !w2 || (want_params && !workspace)) return RL8_ENULL;
  if (rows < 1 || f < 1 || hidden < 1) return RL8_ESIZE;
  if (!aligned_to(x, 4) || !aligned_to(dout, 4) || !aligned_to(gamma, 4) || !aligned_to(beta, 4) ||
      !aligned_to(w1, 4) || !aligned_to(b1, 4) || !aligned_to(w2, 4) || !aligned_to(dx, 4) || !aligned_to(dgamma, 4) ||
      !aligned_to(dbeta, 4) || !aligned_to(dw1, 4) || !aligned_to(db1, 4) || !aligned_to(dw2, 4) ||
      !aligned_to(db2, 4) || !aligned_to(workspace, 4))
    return RL8_EALIGN;
  if (rl8_feedforward_wide_supports(f, hidden) != 1) return RL8_ECONFIG;
  if (!dx && !want_params) return RL8_OK;
  return with_feature_tiles(f, WideBackwardLaunch{x, dout, gamma, beta, eps, w1, b1, w2, rows, f, hidden, residual != 0,
                                                  dx, SumTargets{dw1, db1, dw2, db2, dgamma, dbeta},
                                                  want_params ? workspace : nullptr, (hipStream_t)stream});
}
