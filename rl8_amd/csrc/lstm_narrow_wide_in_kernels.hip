// Narrow LSTMs behind a wide input ("narrow-wide-in"): one layer, biased, batch_first, fp32, hidden width H = 64 or
// 128 and 17 <= d_in <= 128 input floats -- nn.LSTM(d_in, 64 | 128) on a locomotion-sized observation or behind an
// encoder.  lstm_narrow_forward_kernel keeps W_hh and a W_ih of <= 16 columns in registers (190-244 VGPRs); a W_ih of
// up to 128 columns does not fit beside W_hh, so -- as for the upper layers of a stack -- the input product leaves
// the time loop.  The recurrent forward from a pre-formed zin (lstm_narrow_stack_forward_kernel) and the backward
// through time (lstm_narrow_backward_kernel / _heads_kernel, which know nothing of x) are launched as they are
// (lstm_narrow_shared.hip.h); this file has the three products that touch x:
//
//   lstm_narrow_wide_in_proj_kernel   zin[n][4][H] = b_ih + b_hh + x[n] x W_ih^T      over n = b l row-steps
//   lstm_narrow_wide_in_wgrad_kernel  [dW_ih | db] = dz^T x [x | 1],  dW_hh = dz^T x [h_{t-1}]   (one launch each)
//   lstm_narrow_wide_in_dx_kernel     dx[n] = dz[n] x W_ih                             (only where x wants a gradient)
//
// d_in is a run-time argument.  x rows are d_in floats apart in HBM and zero-padded to a multiple of 16 columns in
// LDS / registers; what is compiled per width is a padding class (the trip counts of the unrolled k loops, since
// register arrays cannot be indexed at run time): 32 / 64 / 128 columns for the projection, 48 / 80 / 144 columns
// ([x | 1]) for the weight gradient, 1 / 2 output tiles per wave for dx.  A product with a padded zero adds +0 to an
// fma chain, so the class does not show in the result.
//
// Operand maps of v_mfma_f32_16x16x4_f32 as in lstm_narrow_kernels.hip: lane l holds A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15], D[row = 4 (l >> 4) + r][col = l & 15]; over a k-group of 16 the lane's four steps use
// k = 16 g + 4 (l >> 4) + e, so an operand stored along k is one ds_read_b128.  Every k order is fixed (g, e
// ascending on the MFMA's fma chain) and every grid is a function of (b, l): zin and the gradients do not depend on
// the grid and repeat bit for bit.  Rows past the end go through buffer descriptors (loads 0, stores dropped).
//
// HBM traffic of a training pass per row-step, in floats: projection d_in + 4H, forward 4H (zin) + 6H (hs, gates,
// cell states), backward through time 11H, weight gradient 2 x 4H (dz, once per launch) + d_in + H, dx 4H + d_in:
// 4 (37H + 3 d_in) bytes -- 9.5 KiB at H = 64, d_in = 24 and 20 KiB at H = 128, d_in = 128 -- of which 8H floats are
// the zin round trip the split costs (22H + 2 d_in floats for a narrow LSTM whose W_ih stays in registers).
#include "lstm_narrow_shared.hip.h"
#include "mfma_tile.hip.h"

namespace rl8 {
namespace lstm_narrow_wide_in {

constexpr int kMinIn = 17, kMaxIn = 128;
constexpr int kRows = 32;  // row-steps per tile of the projection and of dx

template <int H>
struct Geo {
  static constexpr int kWaves = H / 16;  // one wave per 16 hidden units, as in the narrow family
  static constexpr int kThreads = 64 * kWaves;
  static constexpr int kWgPerCU = H == 64 ? 2 : 1;  // two waves per SIMD either way: 256 VGPRs
  static constexpr int LD = 4 * H + 4;              // dx: LDS row pitch of dz
  static_assert(H == 64 || H == 128, "narrow LSTM: H = 64 or 128");
};

template <int H>
inline int rows_grid(int64_t n) {
  const int64_t tiles = (n + kRows - 1) / kRows;
  const int64_t cap = (int64_t)kCUs * Geo<H>::kWgPerCU;
  return (int)(tiles < cap ? tiles : cap);
}

__host__ __device__ inline int64_t grad_floats(int hidden, int d_in) { return (int64_t)4 * hidden * (hidden + d_in + 1); }
inline int64_t dz_floats(int64_t b, int l, int hidden) { return b * l * 4 * hidden; }
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// ---- Input projection.  Wave w owns hidden units [16w, 16w + 16) of all four gates; its slice of W_ih stays in
// registers for the whole kernel (KG k-groups of 16 x 4 gates: 4 KG floats per gate and lane, 128 registers in the
// widest class).  A tile is 32 row-steps of x in LDS, [32][16 KG + 4] (pitch = 4 mod 32 banks: the sixteen rows of a
// ds_read_b128 fall on distinct bank quads); the tile's 32 d_in floats are contiguous in HBM, so thread t takes
// elements t, t + threads, .. of them -- the next tile's during the products -- and scatters them to (row, column).
// The pad columns [d_in, 16 KG) are zeroed once and never written again.
template <int H, int KG>
__global__ __launch_bounds__(Geo<H>::kThreads, Geo<H>::kWgPerCU) void lstm_narrow_wide_in_proj_kernel(
    const float *__restrict__ x, int64_t n, int d_in, const float *__restrict__ w_ih, const float *__restrict__ b_ih,
    const float *__restrict__ b_hh, float *__restrict__ zin) {
  using G = Geo<H>;
  constexpr int MT = kRows / 16, R = kRows, KP = 16 * KG, LS = KP + 4, kPer = R * KP / G::kThreads;
  static_assert(R * KP % G::kThreads == 0, "whole elements per thread");
  __shared__ __attribute__((aligned(16))) float tile[R * LS];  // [R][LS]: x rows | zeros
  const int tid = threadIdx.x, lane = tid & 63, qq = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int u = 16 * wave + l16;  // this lane's hidden unit

  // B operand: wx[q][4g + e] = W_ih[qH + u][16g + 4qq + e], zero past d_in.
  float wx[4][4 * KG], bias[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t j = (int64_t)q * H + u;
#pragma unroll
    for (int g = 0; g < KG; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 16 * g + 4 * qq + e;
        wx[q][4 * g + e] = k < d_in ? w_ih[j * d_in + k] : 0.0f;
      }
    bias[q] = b_ih[j] + b_hh[j];
  }
  // Element tid + threads i of a tile's R d_in floats lands at dst[i] in LDS (-1: beyond the tile).
  int dst[kPer];
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int e = tid + G::kThreads * i;
    dst[i] = e < R * d_in ? (e / d_in) * LS + e % d_in : -1;
  }
  for (int i = tid; i < R * LS; i += G::kThreads) tile[i] = 0.0f;

  const int v_z = (4 * qq * 4 * H + u) * 4;
  const int64_t tiles = (n + R - 1) / R;
  float pv[kPer];  // (rows past n fall outside the descriptor: zeros)
  auto fetch = [&](int64_t ti) {
    const int64_t n0 = ti * R;
    const int rows = (int)(n - n0 < R ? n - n0 : R);
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(x + n0 * d_in, (uint32_t)(rows * d_in) * 4);
#pragma unroll
    for (int i = 0; i < kPer; ++i) pv[i] = buffer_load_f32(xr, (tid + G::kThreads * i) * 4, 0);
  };
  if ((int64_t)blockIdx.x < tiles) fetch(blockIdx.x);
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const int64_t n0 = ti * R;
    const int rows = (int)(n - n0 < R ? n - n0 : R);
    __syncthreads();  // the previous tile's readers (the first time: the zeroing) are done
#pragma unroll
    for (int i = 0; i < kPer; ++i)
      if (dst[i] >= 0) tile[dst[i]] = pv[i];
    __syncthreads();
    if (ti + gridDim.x < tiles) fetch(ti + gridDim.x);  // lands during the products
    f32x4 acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[mt][q] = f32x4{bias[q], bias[q], bias[q], bias[q]};
    // k-groups of 16 with the next group's operands read a group ahead; the fence keeps the compiler from hoisting
    // every group's reads (registers beyond the budget: scratch)
    f32x4 a[MT], an[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4 *>(tile + (16 * mt + l16) * LS + 4 * qq);
#pragma unroll
    for (int g = 0; g < KG; ++g) {
      if (g + 1 < KG) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          an[mt] = *reinterpret_cast<const f32x4 *>(tile + (16 * mt + l16) * LS + 16 * (g + 1) + 4 * qq);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            acc[mt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][e], wx[q][4 * g + e], acc[mt][q], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = an[mt];
      __builtin_amdgcn_sched_barrier(0);
    }
    // zin[n][q][u] as lstm_narrow_stack_forward_kernel loads it (rows past n: stores dropped)
    const __amdgpu_buffer_rsrc_t zr = buffer_rsrc(zin + n0 * 4 * H, (uint32_t)rows * 4 * H * 4);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          buffer_store_f32(acc[mt][q][r], zr, v_z + ((16 * mt + r) * 4 * H + q * H) * 4, 0);
  }
}

// ---- Input gradient: dx[n][d_in] = dz[n][4H] x W_ih over n row-steps, K = 4H.  The tile's 32 rows of dz sit in LDS
// once ([32][4H + 4], 33 / 66 KiB) and are shared by the waves; wave w owns the 16-column output tiles w, w + waves
// (TPW of them) with their W_ih^T fragments in registers (H floats per tile and lane).  A wave whose first tile lies
// past d_in only stages.  Columns >= d_in are never written.
template <int H, int TPW>
__global__ __launch_bounds__(Geo<H>::kThreads, Geo<H>::kWgPerCU) void lstm_narrow_wide_in_dx_kernel(
    int64_t n, int d_in, const float *__restrict__ w_ih, const float *__restrict__ dz, float *__restrict__ dx) {
  using G = Geo<H>;
  constexpr int MT = kRows / 16, R = kRows, LD = G::LD, kPer = R * 4 * H / G::kThreads;
  static_assert(16 * G::kWaves * TPW <= kMaxIn && TPW >= 1, "output tiles");
  extern __shared__ float lds[];  // [R][LD]: dz rows
  const int tid = threadIdx.x, lane = tid & 63, qq = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool active = 16 * wave < d_in;  // (wave-uniform)

  // B operand: wt[tp][4g + e] = W_ih[16g + 4qq + e][col], k over the 4H gate columns; zero past d_in.
  float wt[TPW][H];
  int col[TPW];
#pragma unroll
  for (int tp = 0; tp < TPW; ++tp) {
    col[tp] = 16 * (wave + G::kWaves * tp) + l16;
#pragma unroll
    for (int g = 0; g < H / 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        wt[tp][4 * g + e] = col[tp] < d_in ? w_ih[(int64_t)(16 * g + 4 * qq + e) * d_in + col[tp]] : 0.0f;
  }

  const int64_t tiles = (n + R - 1) / R;
  float pv[kPer];  // (the next tile's rows in registers; rows past n fall outside the descriptor: zeros)
  auto fetch = [&](int64_t ti) {
    const int64_t n0 = ti * R;
    const int rows = (int)(n - n0 < R ? n - n0 : R);
    const __amdgpu_buffer_rsrc_t zr = buffer_rsrc(dz + n0 * 4 * H, (uint32_t)rows * 4 * H * 4);
#pragma unroll
    for (int i = 0; i < kPer; ++i) pv[i] = buffer_load_f32(zr, (tid + G::kThreads * i) * 4, 0);
  };
  if ((int64_t)blockIdx.x < tiles) fetch(blockIdx.x);
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const int64_t n0 = ti * R;
    const int rows = (int)(n - n0 < R ? n - n0 : R);
    __syncthreads();  // the previous tile's readers are done
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int e = tid + G::kThreads * i;
      lds[(e / (4 * H)) * LD + e % (4 * H)] = pv[i];
    }
    __syncthreads();
    if (ti + gridDim.x < tiles) fetch(ti + gridDim.x);  // lands during the products
    if (!active) continue;
    f32x4 acc[MT][TPW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int tp = 0; tp < TPW; ++tp) acc[mt][tp] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 a[MT], an[MT];  // (read a group ahead, fenced: as in the projection)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4 *>(lds + (16 * mt + l16) * LD + 4 * qq);
#pragma unroll
    for (int g = 0; g < H / 4; ++g) {
      if (g + 1 < H / 4) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          an[mt] = *reinterpret_cast<const f32x4 *>(lds + (16 * mt + l16) * LD + 16 * (g + 1) + 4 * qq);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int tp = 0; tp < TPW; ++tp)
            acc[mt][tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][e], wt[tp][4 * g + e], acc[mt][tp], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = an[mt];
      __builtin_amdgcn_sched_barrier(0);
    }
    // (rows past n fall outside the descriptor: stores dropped; columns past d_in belong to the next row: not stored)
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(dx + n0 * d_in, (uint32_t)(rows * d_in) * 4);
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp)
      if (col[tp] < d_in) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            buffer_store_f32(acc[mt][tp][r], xr, ((16 * mt + 4 * qq + r) * d_in + col[tp]) * 4, 0);
      }
  }
}

// ---- Weight gradient, with the structure of lstm_narrow_stack_wgrad_kernel: blockIdx.x = sequence chunk, blockIdx.y
// = 64 gate columns, wave w = 16 of them x all NT 16-column tiles of the right-hand side; fp32 MFMA per 64-row stage,
// fp64 across stages; one slab per chunk in the gradient layout [dW_ih (4H d_in) | dW_hh (4H H) | db (4H)].  The
// right-hand columns are split over two launches, so that the fp64 totals (8 NT registers) stay at <= 72:
//   HPART = false  a = [x_t (d_in) | 1 | 0..], 16 NT columns, NT = 3 / 5 / 9  -> dW_ih and db
//   HPART = true   a = [h_{t-1} (h0 at t = 0)], NT = H / 16                   -> dW_hh
// Every load of a stage is issued before its LDS stores.
constexpr int kWgradRows = 64;    // rows per stage
constexpr int kWgradZPitch = 80;  // LDS pitch of the dz stage (64 columns)
constexpr int kWgradThreads = 256;

template <int H, int NT, bool HPART>
__global__ __launch_bounds__(kWgradThreads, 2) void lstm_narrow_wide_in_wgrad_kernel(
    const float *__restrict__ x, int64_t b, int l, int d_in, const float *__restrict__ h0,
    const float *__restrict__ hs, const float *__restrict__ dz, int64_t per_chunk, float *__restrict__ slabs) {
  constexpr int KW = 16 * NT, AS = KW % 32 == 16 ? KW : KW + 16, ZS = kWgradZPitch;
  static_assert(!HPART || KW == H, "the h launch has H columns");
  __shared__ float zs[kWgradRows * ZS];
  __shared__ float as[kWgradRows * AS];
  const int tid = threadIdx.x, lane = tid & 63, qq = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t s0 = blockIdx.x * per_chunk;
  const int64_t s1 = s0 + per_chunk < b ? s0 + per_chunk : b;
  const int64_t r0 = s0 * l, r1 = s1 * l;
  const int j0 = 64 * blockIdx.y;

  double tot[NT][4];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) tot[n][r] = 0.0;
  // wave w stages rows w, w + 4, ... of every stage: (sequence, step) of its next row, advanced 4 rows at a time
  int64_t seq = s0 + wave / l;
  int t = wave % l;
  for (int64_t rb = r0; rb < r1; rb += kWgradRows) {
    constexpr int kRowsPerWave = kWgradRows / 4, NK = (KW + 63) / 64;
    const int rows = (int)(r1 - rb < kWgradRows ? r1 - rb : kWgradRows);
    // (rows past the chunk fall outside the stage's descriptors: zeros)
    const __amdgpu_buffer_rsrc_t zr = buffer_rsrc(dz + rb * 4 * H, (uint32_t)rows * 4 * H * 4);
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(HPART ? nullptr : x + rb * d_in, (uint32_t)(rows * d_in) * 4);
    const float *hp[kRowsPerWave];
    if constexpr (HPART) {
#pragma unroll
      for (int i = 0; i < kRowsPerWave; ++i) {
        hp[i] = t > 0 ? hs + (rb + wave + 4 * i - 1) * H : h0 + seq * H;
        t += 4;
        while (t >= l) {
          t -= l;
          ++seq;
        }
      }
    }
    float v[kRowsPerWave][NK], zv[kRowsPerWave];
#pragma unroll
    for (int i = 0; i < kRowsPerWave; ++i) {
      const int rr = wave + 4 * i;
#pragma unroll
      for (int nk = 0; nk < NK; ++nk) {
        const int k = lane + 64 * nk;
        if constexpr (HPART) v[i][nk] = rr < rows ? hp[i][k] : 0.0f;
        else
          v[i][nk] = k < d_in ? buffer_load_f32(xr, (rr * d_in + k) * 4, 0) : (k == d_in && rr < rows ? 1.0f : 0.0f);
      }
      zv[i] = buffer_load_f32(zr, (rr * 4 * H + j0 + lane) * 4, 0);
    }
    __syncthreads();  // the previous stage's readers are done
#pragma unroll
    for (int i = 0; i < kRowsPerWave; ++i) {
      const int rr = wave + 4 * i;
#pragma unroll
      for (int nk = 0; nk < NK; ++nk)
        if (lane + 64 * nk < KW) as[rr * AS + lane + 64 * nk] = v[i][nk];
      zs[rr * ZS + lane] = zv[i];
    }
    __syncthreads();
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int s = 0; s < kWgradRows / 4; ++s) {
      const int kr = 4 * s + qq;
      const float a = zs[kr * ZS + 16 * wave + l16];
#pragma unroll
      for (int n = 0; n < NT; ++n)
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, as[kr * AS + 16 * n + l16], acc[n], 0, 0, 0);
    }
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) tot[n][r] += (double)acc[n][r];
  }

  float *slab = slabs + (int64_t)blockIdx.x * grad_floats(H, d_in);
  const int o_hh = 4 * H * d_in, o_b = o_hh + 4 * H * H;
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + 16 * wave + 4 * qq + r, k = 16 * n + l16;
      const float g = (float)tot[n][r];
      if constexpr (HPART) {
        slab[o_hh + j * H + k] = g;
      } else {
        if (k < d_in) slab[j * d_in + k] = g;
        else if (k == d_in) slab[o_b + j] = g;
      }
    }
}

// grads[e] = sum over the slabs, in slab (chunk) order, in fp64.
__global__ __launch_bounds__(kBlock) void lstm_narrow_wide_in_reduce_kernel(const float *__restrict__ slabs,
                                                                            int slab_count, int64_t floats,
                                                                            float *__restrict__ grads) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= floats) return;
  double s = 0.0;
  for (int g = 0; g < slab_count; ++g) s += (double)slabs[(int64_t)g * floats + e];
  grads[e] = (float)s;
}

template <int H>
int launch_proj(hipStream_t s, const float *x, int64_t n, int d_in, const float *w_ih, const float *b_ih,
                const float *b_hh, float *zin) {
  const int grid = rows_grid<H>(n), threads = Geo<H>::kThreads;
  if (d_in <= 32) lstm_narrow_wide_in_proj_kernel<H, 2><<<grid, threads, 0, s>>>(x, n, d_in, w_ih, b_ih, b_hh, zin);
  else if (d_in <= 64) lstm_narrow_wide_in_proj_kernel<H, 4><<<grid, threads, 0, s>>>(x, n, d_in, w_ih, b_ih, b_hh, zin);
  else lstm_narrow_wide_in_proj_kernel<H, 8><<<grid, threads, 0, s>>>(x, n, d_in, w_ih, b_ih, b_hh, zin);
  return launch_status();
}

template <int H, int TPW>
int launch_dx_class(hipStream_t s, int64_t n, int d_in, const float *w_ih, const float *dz, float *dx) {
  constexpr size_t bytes = sizeof(float) * kRows * Geo<H>::LD;
  static_assert(bytes * Geo<H>::kWgPerCU <= 160 * 1024, "dx LDS");
  constexpr auto *kernel = &lstm_narrow_wide_in_dx_kernel<H, TPW>;
  if (const int e = allow_dynamic_lds<kernel>((int)bytes)) return e;
  kernel<<<rows_grid<H>(n), Geo<H>::kThreads, bytes, s>>>(n, d_in, w_ih, dz, dx);
  return launch_status();
}

inline int launch_dx(hipStream_t s, int hidden, int64_t n, int d_in, const float *w_ih, const float *dz, float *dx) {
  if (hidden == 128) return launch_dx_class<128, 1>(s, n, d_in, w_ih, dz, dx);
  return d_in <= 64 ? launch_dx_class<64, 1>(s, n, d_in, w_ih, dz, dx) : launch_dx_class<64, 2>(s, n, d_in, w_ih, dz, dx);
}

// The two weight-gradient launches: columns [x | 1] in their padding class, then columns [h_{t-1}].
template <int H>
int launch_wgrad(hipStream_t s, const float *x, int64_t b, int l, int d_in, const float *h0, const float *hs,
                 const float *dz, float *slabs) {
  int64_t per = 0;
  int count = 0;
  lstm_narrow::shared_chunks(H, b, &per, &count);
  const dim3 grid(count, 4 * H / 64);
  if (d_in + 1 <= 48)
    lstm_narrow_wide_in_wgrad_kernel<H, 3, false><<<grid, kWgradThreads, 0, s>>>(x, b, l, d_in, h0, hs, dz, per, slabs);
  else if (d_in + 1 <= 80)
    lstm_narrow_wide_in_wgrad_kernel<H, 5, false><<<grid, kWgradThreads, 0, s>>>(x, b, l, d_in, h0, hs, dz, per, slabs);
  else
    lstm_narrow_wide_in_wgrad_kernel<H, 9, false><<<grid, kWgradThreads, 0, s>>>(x, b, l, d_in, h0, hs, dz, per, slabs);
  if (const int st = launch_status()) return st;
  lstm_narrow_wide_in_wgrad_kernel<H, H / 16, true><<<grid, kWgradThreads, 0, s>>>(x, b, l, d_in, h0, hs, dz, per, slabs);
  return launch_status();
}

inline int slab_count(int hidden, int64_t b) {
  int64_t per = 0;
  int count = 0;
  lstm_narrow::shared_chunks(hidden, b, &per, &count);
  return count;
}

}  // namespace lstm_narrow_wide_in
}  // namespace rl8

using namespace rl8;
namespace wide = rl8::lstm_narrow_wide_in;

RL8_API int rl8_lstm_narrow_wide_in_supports(int hidden, int d_in) {
  return (hidden == 64 || hidden == 128) && d_in >= wide::kMinIn && d_in <= wide::kMaxIn;
}

// (hidden first: lstm_narrow::shared_sizes_ok is written for the two widths)
static bool lstm_narrow_wide_in_ok(int64_t b, int l, int hidden, int d_in) {
  return rl8_lstm_narrow_wide_in_supports(hidden, d_in) && lstm_narrow::shared_sizes_ok(b, l, hidden);
}

RL8_API int64_t rl8_lstm_narrow_wide_in_workspace_bytes(int64_t b, int l, int hidden, int d_in) {
  if (!lstm_narrow_wide_in_ok(b, l, hidden, d_in)) return RL8_ESIZE;
  return (wide::dz_floats(b, l, hidden) + (int64_t)wide::slab_count(hidden, b) * wide::grad_floats(hidden, d_in)) *
         (int64_t)sizeof(float);
}

RL8_API int rl8_lstm_narrow_wide_in_forward_f32(const float *x, int64_t b, int l, int d_in, const float *h0,
                                                const float *c0, const float *w_ih, const float *w_hh,
                                                const float *b_ih, const float *b_hh, int hidden, float *zin,
                                                float *hs, float *hn, float *cn, float *save_gates, float *save_c,
                                                void *stream) {
  if (!x || !h0 || !c0 || !w_ih || !w_hh || !b_ih || !b_hh || !zin || !hs || !hn || !cn) return RL8_ENULL;
  if ((save_gates == nullptr) != (save_c == nullptr)) return RL8_ENULL;
  if (!lstm_narrow_wide_in_ok(b, l, hidden, d_in)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)h0, (const void *)c0, (const void *)w_ih, (const void *)w_hh,
                        (const void *)b_ih, (const void *)b_hh, (const void *)hs, (const void *)hn, (const void *)cn,
                        (const void *)save_gates, (const void *)save_c})
    if (!wide::aligned4(p)) return RL8_EALIGN;
  if (!aligned16(zin)) return RL8_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int st = hidden == 64 ? wide::launch_proj<64>(s, x, b * l, d_in, w_ih, b_ih, b_hh, zin)
                              : wide::launch_proj<128>(s, x, b * l, d_in, w_ih, b_ih, b_hh, zin);
  if (st != RL8_OK) return st;
  return lstm_narrow::shared_recurrent_forward(s, hidden, zin, b, l, h0, c0, w_hh, hs, hn, cn, save_gates, save_c);
}

static int lstm_narrow_wide_in_wgrad(hipStream_t s, const float *x, int64_t b, int l, int d_in, const float *h0,
                                     int hidden, const float *hs, float *workspace) {
  const float *dz = workspace;
  float *slabs = workspace + wide::dz_floats(b, l, hidden);
  return hidden == 64 ? wide::launch_wgrad<64>(s, x, b, l, d_in, h0, hs, dz, slabs)
                      : wide::launch_wgrad<128>(s, x, b, l, d_in, h0, hs, dz, slabs);
}

RL8_API int rl8_lstm_narrow_wide_in_backward_f32(const float *x, int64_t b, int l, int d_in, const float *h0,
                                                 const float *c0, const float *w_hh, int hidden, const float *hs,
                                                 const float *gates, const float *cs, const float *dhs,
                                                 float *workspace, void *stream) {
  if (!x || !h0 || !c0 || !w_hh || !hs || !gates || !cs || !dhs || !workspace) return RL8_ENULL;
  if (!lstm_narrow_wide_in_ok(b, l, hidden, d_in)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)h0, (const void *)c0, (const void *)w_hh, (const void *)hs,
                        (const void *)gates, (const void *)cs, (const void *)dhs})
    if (!wide::aligned4(p)) return RL8_EALIGN;
  if (!aligned16(workspace)) return RL8_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int st = lstm_narrow::shared_backward(s, hidden, b, l, c0, w_hh, gates, cs, dhs, nullptr, nullptr, workspace);
  if (st != RL8_OK) return st;
  return lstm_narrow_wide_in_wgrad(s, x, b, l, d_in, h0, hidden, hs, workspace);
}

RL8_API int rl8_lstm_narrow_wide_in_backward_heads_f32(const float *x, int64_t b, int l, int d_in, const float *h0,
                                                       const float *c0, const float *w_hh, int hidden,
                                                       const float *hs, const float *gates, const float *cs,
                                                       const float *heads_dout, const float *heads_w,
                                                       float *workspace, void *stream) {
  if (!x || !h0 || !c0 || !w_hh || !hs || !gates || !cs || !heads_dout || !heads_w || !workspace) return RL8_ENULL;
  if (!lstm_narrow_wide_in_ok(b, l, hidden, d_in)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)h0, (const void *)c0, (const void *)w_hh, (const void *)hs,
                        (const void *)gates, (const void *)cs, (const void *)heads_w})
    if (!wide::aligned4(p)) return RL8_EALIGN;
  if (!aligned16(heads_dout) || !aligned16(workspace)) return RL8_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int st =
      lstm_narrow::shared_backward(s, hidden, b, l, c0, w_hh, gates, cs, nullptr, heads_dout, heads_w, workspace);
  if (st != RL8_OK) return st;
  return lstm_narrow_wide_in_wgrad(s, x, b, l, d_in, h0, hidden, hs, workspace);
}

RL8_API int rl8_lstm_narrow_wide_in_reduce_f32(const float *workspace, int64_t b, int l, int hidden, int d_in,
                                               float *grads_out, void *stream) {
  if (!workspace || !grads_out) return RL8_ENULL;
  if (!lstm_narrow_wide_in_ok(b, l, hidden, d_in)) return RL8_ESIZE;
  if (!aligned16(workspace) || !wide::aligned4(grads_out)) return RL8_EALIGN;
  const int64_t floats = wide::grad_floats(hidden, d_in);
  wide::lstm_narrow_wide_in_reduce_kernel<<<(unsigned)((floats + kBlock - 1) / kBlock), kBlock, 0,
                                            (hipStream_t)stream>>>(workspace + wide::dz_floats(b, l, hidden),
                                                                   wide::slab_count(hidden, b), floats, grads_out);
  return launch_status();
}

RL8_API int rl8_lstm_narrow_wide_in_input_grad_f32(const float *workspace, int64_t b, int l, int d_in,
                                                   const float *w_ih, int hidden, float *dx, void *stream) {
  if (!workspace || !w_ih || !dx) return RL8_ENULL;
  if (!lstm_narrow_wide_in_ok(b, l, hidden, d_in)) return RL8_ESIZE;
  if (!aligned16(workspace) || !wide::aligned4(w_ih) || !wide::aligned4(dx)) return RL8_EALIGN;
  return wide::launch_dx((hipStream_t)stream, hidden, b * l, d_in, w_ih, workspace, dx);
}
