// Narrow policy / value towers: Linear(d_in, H) ReLU Linear(H, H) ReLU Linear(H, n_out)
// with H = 64 or 128 (the reference's example models use (64, 64) and (128, 128)),
// d_in <= 16, n_out <= 8, biased layers.  The 256-wide towers run mlp_kernels.hip /
// mlp_f16_kernels.hip; nothing here is shared with them.
//
// Forward: a workgroup (4 waves) walks 64-row tiles.  Layers 1 and 2 run on
// v_mfma_f32_32x32x2_f32 (exact k-ordered fp32 fma chains), the head on the VALU.  W2 stays in LDS for the whole kernel; only `out`
// goes to HBM -- no h1 / h2 is saved: at these widths storing them costs more than
// the backward recomputing them.
//
// Backward: one kernel recomputes z1 / h1 / z2 / h2 per tile from x (the same code,
// hence the same bits, as the forward), then forms dz2 = (dout W3) . [z2 > 0],
// dh1 = dz2 W2 (MFMA), dz1 = dh1 . [z1 > 0] and accumulates, across the tiles of the
// workgroup, dW2 += dz2^T h1 (MFMA with k over rows, in accumulators), dW1, dW3 and
// the bias gradients (per-lane partials, summed per tile and then across tiles).  Each workgroup writes one slab in the
// final gradient layout; mlp_narrow_reduce_kernel adds the slabs in slab order in
// fp64.  The grid is a function of m alone, so the gradients are bitwise
// reproducible.  ReLU'(0) = 0 (the masks test h > 0, i.e. z > 0).
//
// MFMA operand maps (gfx950, 32x32x2 f32): lane l holds A[i = l&31][k = l>>5] and
// B[k = l>>5][j = l&31]; D[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31], r < 16.
// Over one k-group of 8 the lane's four consecutive steps use k = 8g + 4*(l>>5) + e,
// e = 0..3, so an operand stored along k is one ds_read_b128.
//
// LDS (floats, row stride LS = H + 4 keeps rows 16-byte aligned and spreads the
// row walks of the A operands over the banks):
//   forward : W2 [H][LS] | h1 [64][LS] | h2 [64][LS] | x [64][KIN + 1] | W3^T [H][KOUT]
//   backward: W2 [H][LS] | h1 [64][LS] | dz2 [64][LS] | x [64][KIN + 1] | dout [64][KOUT]
//   backward with dx (DX): the same | W1 [H][KIN + 4]; dz1 takes the dz2 tile over
// H = 64: 52 / 57 / 62 KiB (two workgroups per CU); H = 128: 136 / 141 / 148 KiB (one).  (KIN = 16, KOUT = 8.)
//
// This header holds the kernels; mlp_narrow_kernels.hip launches the instantiations without dx,
// mlp_narrow_dx_kernels.hip those with it.
#pragma once

#include "mfma_tile.hip.h"

namespace rl8 {
namespace narrow {

constexpr int kRows = 64;  // rows per tile
constexpr int kThreads = 256;

template <int H>
struct Geo {
  static constexpr int LS = H + 4;
  static constexpr int NT = H / 32;         // 32-column tiles of a [64][H] activation
  static constexpr int MTW = NT / 2;        // 32-row tiles per wave (the wave owns column tile w % NT)
  static constexpr int TW = NT * NT / 4;    // 32x32 tiles of dW2 per wave
  static constexpr int C = 2 * (4 / NT);    // partial-sum contributors per column (lane halves x waves)
  static constexpr int kWgPerCU = H == 64 ? 2 : 1;
  static_assert(H == 64 || H == 128, "narrow towers: H = 64 or 128");
};

template <int H>
__host__ __device__ constexpr int grad_floats(int d_in, int n_out) {
  return H * d_in + H + H * H + H + n_out * H + n_out;
}
// A workgroup's slab: the gradient layout, then the low parts of db3 (db3 = hi + lo: the sums of dout are carried
// in fp64 to the reduction, so a bias gradient that cancels to a small value keeps its digits).
template <int H>
__host__ __device__ constexpr int slab_floats(int d_in, int n_out) {
  return grad_floats<H>(d_in, n_out) + n_out;
}

template <int H>
inline int grid_for(int64_t m) {
  const int64_t tiles = (m + kRows - 1) / kRows;
  const int64_t cap = (int64_t)kCUs * Geo<H>::kWgPerCU;
  return (int)(tiles < cap ? tiles : cap);
}

template <int H, int KIN, int KOUT>
constexpr size_t forward_lds_floats() {
  return (size_t)H * Geo<H>::LS + 2 * kRows * Geo<H>::LS + kRows * (KIN + 1) + H * KOUT;
}
template <int H, int KIN, int KOUT>
constexpr size_t backward_lds_floats() {
  return (size_t)H * Geo<H>::LS + 2 * kRows * Geo<H>::LS + kRows * (KIN + 1) + kRows * KOUT;
}

// W2 [H][H] (row-major, torch layout) -> LDS [H][LS].
template <int H>
__device__ __forceinline__ void stage_w2(const float *__restrict__ w2, float *w2s, int tid) {
#pragma unroll 4
  for (int idx = tid; idx < H * H; idx += kThreads) w2s[(idx / H) * Geo<H>::LS + idx % H] = w2[idx];
}

// One [64][W] tile of a row-major [m][width] array into registers (zero past m / width).
template <int W>
struct TileRegs {
  static constexpr int kPer = (kRows * W + kThreads - 1) / kThreads;
  float v[kPer];
  __device__ __forceinline__ void fetch(const float *__restrict__ src, int64_t m, int width, int64_t tile, int tid) {
    const int64_t r0 = tile * kRows;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int e = tid + kThreads * u, r = e / W, c = e % W;
      const int64_t row = r0 + r;
      v[u] = (e < kRows * W && c < width && row < m) ? src[row * width + c] : 0.0f;
    }
  }
  template <int STRIDE = W>
  __device__ __forceinline__ void store(float *dst, int tid) const {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int e = tid + kThreads * u;
      if (e < kRows * W) dst[(e / W) * STRIDE + e % W] = v[u];
    }
  }
};

// h1 [64][LS] = relu(x W1^T + b1) on the matrix cores (k = 2s + lane half, KIN / 2 steps): the wave's 32-column
// tile nt, rows 32 (mt0 + m) ..  xs [64][KIN + 1] (the odd stride spreads the 32 rows a step reads over the banks);
// w1f[s] = W1[32 nt + (l & 31)][2 s + (l >> 5)], b1c = b1[32 nt + (l & 31)].
template <int H, int KIN>
__device__ __forceinline__ void layer1(const float *xs, const float (&w1f)[KIN / 2], float b1c, int nt, int mt0,
                                       int lane, float *h1s) {
  constexpr int MTW = Geo<H>::MTW;
  const int l32 = lane & 31, hh = lane >> 5;
  f32x16 acc[MTW];
#pragma unroll
  for (int m = 0; m < MTW; ++m)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[m][v] = b1c;
#pragma unroll
  for (int st = 0; st < KIN / 2; ++st)
#pragma unroll
    for (int m = 0; m < MTW; ++m)
      acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[(32 * (mt0 + m) + l32) * (KIN + 1) + 2 * st + hh], w1f[st],
                                                    acc[m], 0, 0, 0);
#pragma unroll
  for (int m = 0; m < MTW; ++m)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const float z = acc[m][v];
      h1s[(32 * (mt0 + m) + (v & 3) + 8 * (v >> 2) + 4 * hh) * Geo<H>::LS + 32 * nt + l32] = z > 0.0f ? z : 0.0f;
    }
}

// acc[m] (rows 32 (mt0 + m) .., columns 32 nt ..) = b2 + h1 W2^T, on the matrix cores.
template <int H>
__device__ __forceinline__ void layer2(const float *h1s, const float *w2s, float b2r, int nt, int mt0, int lane,
                                       f32x16 (&acc)[Geo<H>::MTW]) {
  constexpr int LS = Geo<H>::LS, MTW = Geo<H>::MTW;
  const int l32 = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int m = 0; m < MTW; ++m)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[m][v] = b2r;
  const float *bp = w2s + (32 * nt + l32) * LS + 4 * hh;
  const float *ap = h1s + (32 * mt0 + l32) * LS + 4 * hh;
#pragma unroll 2
  for (int g = 0; g < H / 8; ++g) {
    const f32x4 b = *reinterpret_cast<const f32x4 *>(bp + 8 * g);
    f32x4 a[MTW];
#pragma unroll
    for (int m = 0; m < MTW; ++m) a[m] = *reinterpret_cast<const f32x4 *>(ap + 32 * m * LS + 8 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int m = 0; m < MTW; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][e], b[e], acc[m], 0, 0, 0);
  }
}

__device__ __forceinline__ int acc_row(int v, int hh) { return (v & 3) + 8 * (v >> 2) + 4 * hh; }

template <int H, int KIN, int KOUT>
__global__ __launch_bounds__(kThreads, Geo<H>::kWgPerCU) void mlp_narrow_forward_kernel(
    const float *__restrict__ x, int64_t m, int d_in, const float *__restrict__ w1, const float *__restrict__ b1,
    const float *__restrict__ w2, const float *__restrict__ b2, const float *__restrict__ w3,
    const float *__restrict__ b3, int n_out, float *__restrict__ out) {
  using G = Geo<H>;
  constexpr int LS = G::LS;
  extern __shared__ float lds[];
  float *w2s = lds, *h1s = w2s + H * LS, *h2s = h1s + kRows * LS, *xs = h2s + kRows * LS, *w3s = xs + kRows * (KIN + 1);
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = wave % G::NT, mt0 = (wave / G::NT) * G::MTW;

  stage_w2<H>(w2, w2s, tid);
  for (int idx = tid; idx < H * KOUT; idx += kThreads) {
    const int j = idx / KOUT, q = idx % KOUT;
    w3s[idx] = q < n_out ? w3[q * H + j] : 0.0f;
  }
  float w1f[KIN / 2];
#pragma unroll
  for (int st = 0; st < KIN / 2; ++st) {
    const int k = 2 * st + hh;
    w1f[st] = k < d_in ? w1[(32 * nt + l32) * d_in + k] : 0.0f;
  }
  const float b1c = b1[32 * nt + l32];
  const float b2r = b2[32 * nt + l32];
  float b3r[KOUT];
#pragma unroll
  for (int q = 0; q < KOUT; ++q) b3r[q] = q < n_out ? b3[q] : 0.0f;

  const int64_t tiles = (m + kRows - 1) / kRows;
  TileRegs<KIN> xr;
  xr.fetch(x, m, d_in, blockIdx.x, tid);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's readers of xs / h1s / h2s are done (and W2 / W3 are staged)
    xr.template store<KIN + 1>(xs, tid);
    if (tile + gridDim.x < tiles) xr.fetch(x, m, d_in, tile + gridDim.x, tid);
    __syncthreads();
    layer1<H, KIN>(xs, w1f, b1c, nt, mt0, lane, h1s);
    __syncthreads();
    f32x16 acc[G::MTW];
    layer2<H>(h1s, w2s, b2r, nt, mt0, lane, acc);
#pragma unroll
    for (int mm = 0; mm < G::MTW; ++mm)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float z = acc[mm][v];
        h2s[(32 * (mt0 + mm) + acc_row(v, hh)) * LS + 32 * nt + l32] = z > 0.0f ? z : 0.0f;
      }
    __syncthreads();
    // Head: thread (row tid / 4, part tid % 4) sums columns 4 (p + 4c) .. + 3; the parts meet
    // in a fixed order through two lane exchanges.
    const int r = tid >> 2, p = tid & 3;
    float o[KOUT];
#pragma unroll
    for (int q = 0; q < KOUT; ++q) o[q] = 0.0f;
#pragma unroll 2
    for (int c = 0; c < H / 16; ++c) {
      const int j0 = 4 * (p + 4 * c);
      const f32x4 hv = *reinterpret_cast<const f32x4 *>(h2s + r * LS + j0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int q = 0; q < KOUT; ++q) o[q] = fmaf(hv[e], w3s[(j0 + e) * KOUT + q], o[q]);
    }
    const int64_t row = tile * kRows + r;
#pragma unroll
    for (int q = 0; q < KOUT; ++q) {
      const float s1 = o[q] + __shfl_xor(o[q], 1);
      const float s2 = s1 + __shfl_xor(s1, 2);
      if (p == 0 && q < n_out && row < m) out[row * n_out + q] = s2 + b3r[q];
    }
  }
}

// The lane index behind an empty asm: what is computed from it is formed where it is used, per tile, and does not sit in
// registers through the other phases (the DX variant has none to spare at H = 64).
__device__ __forceinline__ int fresh(int tid) {
  asm volatile("" : "+v"(tid));
  return tid;
}

// The backward of one workgroup.  DX: dx [m][d_in] = dz1 W1 as well -- dz1 goes through the dz2 tile (dead once every
// wave has formed dh1), W1 through its own [H][KIN + 4] tile behind dout, and thread (row tid / 4, part tid % 4) forms
// the row's d_in dots over columns 4 (part + 4c) .. + 3 as the forward forms the head.  Nothing else differs, so the
// slab holds the same bits either way.
template <int H, int KIN, int KOUT, bool DX = false>
__global__ __launch_bounds__(kThreads, Geo<H>::kWgPerCU) void mlp_narrow_backward_kernel(
    const float *__restrict__ x, const float *__restrict__ dout, int64_t m, int d_in, const float *__restrict__ w1,
    const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2,
    const float *__restrict__ w3, int n_out, float *__restrict__ slabs, float *__restrict__ dx) {
  using G = Geo<H>;
  constexpr int LS = G::LS, MTW = G::MTW, TW = G::TW;
  extern __shared__ float lds[];
  float *w2s = lds, *h1s = w2s + H * LS, *dzs = h1s + kRows * LS, *xs = dzs + kRows * LS, *ds = xs + kRows * (KIN + 1);
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = wave % G::NT, mt0 = (wave / G::NT) * MTW;
  const int col = 32 * nt + l32;  // this lane's column of the [64][H] activations
  const int jt = (wave * TW) / G::NT, it0 = (wave * TW) % G::NT;  // this wave's dW2 tiles: (jt, it0 + u)

  stage_w2<H>(w2, w2s, tid);
  [[maybe_unused]] float *w1s = ds + kRows * KOUT;  // DX: W1 [H][KIN + 4], zero past d_in
  if constexpr (DX)
    for (int idx = tid; idx < H * KIN; idx += kThreads) {
      const int j = idx / KIN, k = idx % KIN;
      w1s[j * (KIN + 4) + k] = k < d_in ? w1[j * d_in + k] : 0.0f;
    }
  float w1f[KIN / 2];
#pragma unroll
  for (int st = 0; st < KIN / 2; ++st) {
    const int k = 2 * st + hh;
    w1f[st] = k < d_in ? w1[(32 * nt + l32) * d_in + k] : 0.0f;
  }
  const float b1c = b1[32 * nt + l32];
  const float b2r = b2[col];
  float w3c[KOUT];
#pragma unroll
  for (int q = 0; q < KOUT; ++q) w3c[q] = q < n_out ? w3[q * H + col] : 0.0f;

  f32x16 wacc[TW];
#pragma unroll
  for (int u = 0; u < TW; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) wacc[u][v] = 0.0f;
  double dw1[KIN], dw3[KOUT], db1 = 0.0, db2 = 0.0;  // (totals over tiles: fp64)
#pragma unroll
  for (int k = 0; k < KIN; ++k) dw1[k] = 0.0;
#pragma unroll
  for (int q = 0; q < KOUT; ++q) dw3[q] = 0.0;
  // db3: lane (q = lane % KOUT, s = lane / KOUT) of wave 0 sums rows s, s + 64 / KOUT, ...
  constexpr int kDb3Rows = KOUT;  // rows per lane per tile
  double db3 = 0.0;

  // This workgroup's slab, in the gradient layout [dW1 | db1 | dW2 | db2 | dW3 | db3].
  const int o_b1 = H * d_in, o_w2 = o_b1 + H, o_b2 = o_w2 + H * H, o_w3 = o_b2 + H, o_b3 = o_w3 + n_out * H;
  float *slab = slabs + (int64_t)blockIdx.x * slab_floats<H>(d_in, n_out);

  const int64_t tiles = (m + kRows - 1) / kRows;
  TileRegs<KIN> xr;
  TileRegs<KOUT> dr;
  xr.fetch(x, m, d_in, blockIdx.x, tid);
  dr.fetch(dout, m, n_out, blockIdx.x, tid);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's readers of xs / ds / h1s / dzs are done
    xr.template store<KIN + 1>(xs, tid);
    dr.store(ds, tid);
    if (tile + gridDim.x < tiles) {
      const int ft = DX ? fresh(tid) : tid;
      xr.fetch(x, m, d_in, tile + gridDim.x, ft);
      dr.fetch(dout, m, n_out, tile + gridDim.x, ft);
    }
    __syncthreads();
    layer1<H, KIN>(xs, w1f, b1c, nt, mt0, lane, h1s);
    if (wave == 0) {
      const int q = lane % KOUT, s = lane / KOUT;
#pragma unroll
      for (int u = 0; u < kDb3Rows; ++u) db3 += (double)ds[(s + (64 / KOUT) * u) * KOUT + q];
    }
    __syncthreads();
    {
      f32x16 acc[MTW];
      float tw3[KOUT], tb2 = 0.0f;
#pragma unroll
      for (int q = 0; q < KOUT; ++q) tw3[q] = 0.0f;
      layer2<H>(h1s, w2s, b2r, nt, mt0, lane, acc);
#pragma unroll
      for (int mm = 0; mm < MTW; ++mm)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int r = 32 * (mt0 + mm) + acc_row(v, hh);
          const float z = acc[mm][v], h2 = z > 0.0f ? z : 0.0f;
          float dh2 = 0.0f;
#pragma unroll
          for (int q = 0; q < KOUT; ++q) {
            const float g = ds[r * KOUT + q];
            dh2 = fmaf(g, w3c[q], dh2);
            tw3[q] = fmaf(g, h2, tw3[q]);
          }
          const float dz = z > 0.0f ? dh2 : 0.0f;
          tb2 += dz;
          dzs[r * LS + col] = dz;
        }
#pragma unroll
      for (int q = 0; q < KOUT; ++q) dw3[q] += tw3[q];
      db2 += tb2;
    }
    __syncthreads();
    // dW2[j][i] += sum_r dz2[r][j] h1[r][i]: A = dz2^T (rows j), B = h1 (columns i), k over the 64 rows.
#pragma unroll 1
    for (int g = 0; g < kRows / 8; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 8 * g + 4 * hh + e;
        const float a = dzs[r * LS + 32 * jt + l32];
#pragma unroll
        for (int u = 0; u < TW; ++u)
          wacc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, h1s[r * LS + 32 * (it0 + u) + l32], wacc[u], 0, 0, 0);
      }
    // dh1 = dz2 W2: A = dz2 (rows r, k = j), B[k = j][i] = W2[j][i].
    {
      f32x16 dacc[MTW];
#pragma unroll
      for (int mm = 0; mm < MTW; ++mm)
#pragma unroll
        for (int v = 0; v < 16; ++v) dacc[mm][v] = 0.0f;
      const float *ap = dzs + (32 * mt0 + l32) * LS + 4 * hh;
#pragma unroll 2
      for (int g = 0; g < H / 8; ++g) {
        f32x4 a[MTW];
#pragma unroll
        for (int mm = 0; mm < MTW; ++mm) a[mm] = *reinterpret_cast<const f32x4 *>(ap + 32 * mm * LS + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float b = w2s[(8 * g + 4 * hh + e) * LS + col];
#pragma unroll
          for (int mm = 0; mm < MTW; ++mm) dacc[mm] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mm][e], b, dacc[mm], 0, 0, 0);
        }
      }
      float tw1[KIN], tb1 = 0.0f;
#pragma unroll
      for (int k = 0; k < KIN; ++k) tw1[k] = 0.0f;
      if constexpr (DX) __syncthreads();  // every wave has read dz2 for the last time: the tile takes dz1
#pragma unroll
      for (int mm = 0; mm < MTW; ++mm)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int r = 32 * (mt0 + mm) + acc_row(v, hh);
          const float dz = h1s[r * LS + col] > 0.0f ? dacc[mm][v] : 0.0f;
          tb1 += dz;
#pragma unroll
          for (int k = 0; k < KIN; ++k) tw1[k] = fmaf(dz, xs[r * (KIN + 1) + k], tw1[k]);
          if constexpr (DX) dzs[r * LS + col] = dz;
        }
#pragma unroll
      for (int k = 0; k < KIN; ++k) dw1[k] += tw1[k];
      db1 += tb1;
    }
    if constexpr (DX) {
      __syncthreads();
      const int t = fresh(tid), r = t >> 2, p = t & 3;
      const int64_t row = tile * kRows + r;
      // (four inputs at a time: the weight-gradient accumulators leave no room for all KIN dots at once)
#pragma unroll 1
      for (int k0 = 0; k0 < KIN; k0 += 4) {
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int c = 0; c < H / 16; ++c) {
          const int j0 = 4 * (p + 4 * c);
          const f32x4 dv = *reinterpret_cast<const f32x4 *>(dzs + r * LS + j0);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const f32x4 wv = *reinterpret_cast<const f32x4 *>(w1s + (j0 + e) * (KIN + 4) + k0);
#pragma unroll
            for (int u = 0; u < 4; ++u) o[u] = fmaf(dv[e], wv[u], o[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float s1 = o[u] + __shfl_xor(o[u], 1);
          const float s2 = s1 + __shfl_xor(s1, 2);
          if (p == u && k0 + u < d_in && row < m) dx[row * d_in + k0 + u] = s2;
        }
      }
    }
  }

  // Epilogue.
#pragma unroll
  for (int u = 0; u < TW; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v)
      slab[o_w2 + (32 * jt + acc_row(v, hh)) * H + 32 * (it0 + u) + l32] = wacc[u][v];
  // Per-lane column partials -> LDS [contributor][column][field], summed over contributors in order.
  constexpr int F = KIN + 1 + KOUT + 1;
  static_assert(G::C * H * F + 128 <= H * LS + 2 * kRows * LS, "epilogue partials fit the freed LDS");
  __syncthreads();  // every read of w2s / h1s / dzs is done
  float *red = lds, *red3 = lds + G::C * H * F;
  {
    const int c = (wave / G::NT) * 2 + hh;
    float *dst = red + (c * H + col) * F;
#pragma unroll
    for (int k = 0; k < KIN; ++k) dst[k] = (float)dw1[k];
    dst[KIN] = (float)db1;
#pragma unroll
    for (int q = 0; q < KOUT; ++q) dst[KIN + 1 + q] = (float)dw3[q];
    dst[KIN + 1 + KOUT] = (float)db2;
    if (wave == 0) {
      const float hi = (float)db3;
      red3[lane] = hi;
      red3[64 + lane] = (float)(db3 - (double)hi);
    }
  }
  __syncthreads();
  if (tid < H) {
    double sum[F];
#pragma unroll
    for (int f = 0; f < F; ++f) sum[f] = 0.0;
#pragma unroll
    for (int c = 0; c < G::C; ++c)
#pragma unroll
      for (int f = 0; f < F; ++f) sum[f] += (double)red[(c * H + tid) * F + f];
#pragma unroll
    for (int k = 0; k < KIN; ++k)
      if (k < d_in) slab[tid * d_in + k] = (float)sum[k];
    slab[o_b1 + tid] = (float)sum[KIN];
#pragma unroll
    for (int q = 0; q < KOUT; ++q)
      if (q < n_out) slab[o_w3 + q * H + tid] = (float)sum[KIN + 1 + q];
    slab[o_b2 + tid] = (float)sum[KIN + 1 + KOUT];
  }
  if (tid < n_out) {
    double s = 0.0;
    for (int k = 0; k < 64 / KOUT; ++k) s += (double)red3[k * KOUT + tid] + (double)red3[64 + k * KOUT + tid];
    const float hi = (float)s;
    slab[o_b3 + tid] = hi;
    slab[o_b3 + n_out + tid] = (float)(s - (double)hi);
  }
}

// Compiled widths: H in {64, 128}; d_in padded to 4 or 16, n_out to 2 or 8 (zero weights in the padding).
template <template <int, int, int> class L, typename... A>
int dispatch(int hidden, int d_in, int n_out, A... args) {
  const bool narrow_in = d_in <= 4, narrow_out = n_out <= 2;
#define RL8_NARROW_CASE(H)                                                              \
  if (hidden == H) {                                                                    \
    if (narrow_in) return narrow_out ? L<H, 4, 2>::run(args...) : L<H, 4, 8>::run(args...); \
    return narrow_out ? L<H, 16, 2>::run(args...) : L<H, 16, 8>::run(args...);          \
  }
  RL8_NARROW_CASE(64)
  RL8_NARROW_CASE(128)
#undef RL8_NARROW_CASE
  return RL8_ESIZE;
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace narrow
}  // namespace rl8
