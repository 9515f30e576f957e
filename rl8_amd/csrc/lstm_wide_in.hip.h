// Device code shared by the width-256 LSTM forwards whose operand row carries more than one extra k-group:
// lstm_wide_in_kernels.hip (one layer behind 8 to 128 input floats) and lstm_stack256_kernels.hip (a layer above the
// first of a stack, whose input row is the 256 floats of the layer below).  The operand row of the recurrent product is
// [h_{t-1} (256) | x_t (d_in) | 1 | 0..], K = 256 + 8 xg with xg = ceil((d_in + 1) / 8) extra k-groups; the forward is
// compiled per CLASS of xg (the LDS row pitch and the shape of the x fetch) and runs the exact 32 + xg groups of the
// packed weights.  Each unit instantiates its own classes; nothing here is a kernel until it does.
#pragma once
#include "lstm_gates.hip.h"
#include "mfma_tile.hip.h"
#include "tower_launch.hip.h"

namespace rl8 {
namespace lstm_wide_in {

constexpr int kRows = 32;  // sequences per tile
constexpr int kGateOrder[4] = {0, 2, 1, 3};

__host__ __device__ constexpr int extra_groups(int d_in) { return (d_in + 1 + 7) / 8; }  // x, the ones column, zeros
__host__ __device__ constexpr int k_groups(int d_in) { return kGroups + extra_groups(d_in); }
constexpr int lds_stride(int xg_class) { return kHidden + 8 * xg_class + 1; }
constexpr size_t forward_lds_bytes(int xg_class) { return sizeof(float) * kRows * lds_stride(xg_class); }
// The widest input a class is compiled for: 8 XG - 1 floats and the ones column fill its groups, except where the
// envelope ends on a multiple of 8 (128 in 17 groups, 256 in 33) and the last group holds the ones column alone.
constexpr int class_max_in(int xg_class) { return xg_class <= 16 ? 8 * xg_class - 1 : 8 * (xg_class - 1); }

// TileGemmT<1>'s pipeline (B fragments three sets deep, A fragments two) over a k-depth taken at run time: kg >= 34
// groups, six per trip, the 0..5 left over behind the loop.  Reloads past the last group are clamped to it and unused.
template <int STRIDE>
struct WideGemm {
  __amdgpu_buffer_rsrc_t bp;
  int bvoff, bvoff1, a_off, kg;
  BFrag b[3];

  __device__ __forceinline__ WideGemm(__amdgpu_buffer_rsrc_t w, int wave, int lane, int groups)
      : bp(w), bvoff((2 * wave) * groups * kWave * 16 + lane * 4), bvoff1(bvoff + groups * kWave * 16),
        a_off((lane & 31) * STRIDE + 4 * (lane >> 5)), kg(groups) {}

  __device__ __forceinline__ void load_b(BFrag &f, int g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f.b0[e] = buffer_load_f32(bp, bvoff + e * (kWave * 4), g * (kWave * 16));
      f.b1[e] = buffer_load_f32(bp, bvoff1 + e * (kWave * 4), g * (kWave * 16));
    }
  }

  __device__ __forceinline__ void prefetch() {
    load_b(b[0], 0);
    load_b(b[1], 1);
    load_b(b[2], 2);
  }

  template <bool FIRST>
  __device__ __forceinline__ void step(AFragT<1> &fa, BFrag &fb, const float *a0p, int g, f32x16 (&acc)[1][2]) {
    mma_frag<FIRST, 1>(fa, fb, acc);
    load_a<1, STRIDE>(fa, a0p, g + 2 < kg ? g + 2 : kg - 1);
    load_b(fb, g + 3 < kg ? g + 3 : kg - 1);
  }

  // ACCUMULATE: add to what `acc` already holds instead of starting from zero.
  template <bool ACCUMULATE = false>
  __device__ __forceinline__ void run(const float *__restrict__ a_tile, f32x16 (&acc)[1][2]) {
    __builtin_amdgcn_s_setprio(0);  // (the matrix loop below every VALU phase: mfma_tile.hip.h)
    const float *a0p = a_tile + a_off;
    AFragT<1> a[2];
    load_a<1, STRIDE>(a[0], a0p, 0);
    load_a<1, STRIDE>(a[1], a0p, 1);
    // A set = g mod 2, B set = g mod 3
    step<!ACCUMULATE>(a[0], b[0], a0p, 0, acc);
    step<false>(a[1], b[1], a0p, 1, acc);
    step<false>(a[0], b[2], a0p, 2, acc);
    step<false>(a[1], b[0], a0p, 3, acc);
    step<false>(a[0], b[1], a0p, 4, acc);
    step<false>(a[1], b[2], a0p, 5, acc);
    const int main_end = kg / 6 * 6;
#pragma unroll 1
    for (int g = 6; g < main_end; g += 6) {
      step<false>(a[0], b[0], a0p, g, acc);
      step<false>(a[1], b[1], a0p, g + 1, acc);
      step<false>(a[0], b[2], a0p, g + 2, acc);
      step<false>(a[1], b[0], a0p, g + 3, acc);
      step<false>(a[0], b[1], a0p, g + 4, acc);
      step<false>(a[1], b[2], a0p, g + 5, acc);
    }
    const int rest = kg - main_end;  // uniform
    if (rest > 0) step<false>(a[0], b[0], a0p, main_end, acc);
    if (rest > 1) step<false>(a[1], b[1], a0p, main_end + 1, acc);
    if (rest > 2) step<false>(a[0], b[2], a0p, main_end + 2, acc);
    if (rest > 3) step<false>(a[1], b[0], a0p, main_end + 3, acc);
    if (rest > 4) step<false>(a[0], b[1], a0p, main_end + 4, acc);
    __builtin_amdgcn_s_setprio(kValuPhasePriority);
  }
};

// Forward over b sequences of l steps.  XG: the class of extra k-groups (8 XG >= d_in + 1).  SAVE: also store the
// post-activation gates ([b][l][4][256], order i, f, g, o) and the cell states ([b][l][256]).
template <int XG, bool SAVE>
__global__ __launch_bounds__(kBlock, 2) void lstm_wide_in_forward_kernel(
    const float *__restrict__ x, int64_t b, int l, int d_in, const float *__restrict__ h0,
    const float *__restrict__ c0, const float *__restrict__ w_packed, float *__restrict__ hs, float *__restrict__ hn,
    float *__restrict__ cn, float *__restrict__ save_gates, float *__restrict__ save_c) {
  constexpr int kStride = lds_stride(XG);
  // x_t of a class that ends at 256 floats is another layer's hs: one dense, 16-byte-aligned 1-KiB row per sequence, which
  // goes HBM -> LDS as the h0 rows do (no registers held over the products); the narrower classes' through registers.
  constexpr bool kDirectX = class_max_in(XG) == kHidden;
  constexpr int kXPerThread = kDirectX ? 1 : (class_max_in(XG) + 7) / 8;  // 8 threads per row: columns tid % 8 + 8 u
  static_assert(kDirectX || 8 * kXPerThread >= class_max_in(XG), "the fetch covers the class");
  static_assert(8 * XG >= class_max_in(XG) + 1, "the class holds its widest input and the ones column");
  extern __shared__ float lds[];
  float *ht = lds;  // [32][kStride]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5, l31 = lane & 31;
  const int kg = k_groups(d_in);
  const int gate_floats = 8 * kg * 4 * kWave;

  __amdgpu_buffer_rsrc_t wrsrc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) wrsrc[q] = buffer_rsrc(w_packed + q * gate_floats, gate_floats * 4);
  WideGemm<kStride> gemm(wrsrc[0], wave, lane, kg);
  __builtin_amdgcn_s_setprio(kValuPhasePriority);
  // accumulator slot (nt, r) of this lane: row (r&3) + 8(r>>2) + 4*hh, unit 64*wave + 32*nt + l31 (lstm_forward_kernel)
  const int unit4 = (64 * wave + l31) * 4;
  const int v_state = 4 * hh * kHidden * 4 + unit4;          // [rows][256]: c0, hn, cn
  const int v_seq = 4 * hh * l * kHidden * 4 + unit4;        // [rows][l][256]: hs, cs
  const int v_gates = 4 * hh * l * 4 * kHidden * 4 + unit4;  // [rows][l][4][256]
  // columns 256 + d_in .. of the tile: the ones column, then zeros; x_t (columns 256 .. 256 + d_in) is written per step
  constexpr int kPad = 8 * XG + 1;
  for (int i = tid; i < kRows * kPad; i += kBlock) {
    const int row = i / kPad, c = i - row * kPad;
    if (c >= d_in) ht[row * kStride + kHidden + c] = c == d_in ? 1.0f : 0.0f;
  }
  const int x_row = tid >> 3, x_col = tid & 7;
  const int x_voff = (x_row * l * d_in + x_col) * 4;  // + 32 u; the step in the scalar offset
  float *x_lds = ht + x_row * kStride + kHidden + x_col;  // + 8 u

  const int64_t tiles = (b + kRows - 1) / kRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t b0 = tile * kRows;
    const int rows = (int)((b - b0) < kRows ? (b - b0) : kRows);
    const __amdgpu_buffer_rsrc_t h0rsrc = buffer_rsrc(h0 + b0 * kHidden, rows * kHidden * 4);
    const __amdgpu_buffer_rsrc_t c0rsrc = buffer_rsrc(c0 + b0 * kHidden, rows * kHidden * 4);
    const __amdgpu_buffer_rsrc_t xrsrc = buffer_rsrc(x + b0 * l * d_in, (uint32_t)(rows * l * d_in * 4));
    float xr[kXPerThread];
    auto fetch_x = [&](int t) {
      if constexpr (!kDirectX) {
#pragma unroll
        for (int u = 0; u < kXPerThread; ++u) xr[u] = buffer_load_f32(xrsrc, x_voff + 32 * u, t * d_in * 4);
      }
    };
    auto stage_x = [&]() {  // (a column >= d_in holds a neighbour's value: not written)
      if constexpr (!kDirectX) {
#pragma unroll
        for (int u = 0; u < kXPerThread; ++u)
          if (x_col + 8 * u < d_in) x_lds[8 * u] = xr[u];
      }
    };
    // kDirectX: step t's x rows -> columns 256.. of the tile, wave w rows w, w + 4, ..; rows past the end = 0.  Issued
    // where no wave reads the tile any more and waited for (wait_vmcnt0) before the barrier that opens the next products.
    auto load_x_rows = [&](int t) {
      const __amdgpu_buffer_rsrc_t xs = buffer_rsrc(x + (b0 * l + t) * kHidden, ((rows - 1) * l + 1) * kHidden * 4);
#pragma unroll
      for (int u = 0; u < kRows / 4; ++u) {
        const int row = wave + 4 * u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xs, ht + row * kStride + kHidden, 16, lane * 16, row * l * (kHidden * 4), 0,
                                                 0);
      }
    };
    fetch_x(0);
    __syncthreads();  // the previous tile's last readers of ht are done
    // h0 tile -> LDS (one 1-KiB row per direct-to-LDS load; rows past the end = 0)
#pragma unroll
    for (int u = 0; u < kRows / 4; ++u) {
      const int row = wave + 4 * u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(h0rsrc, ht + row * kStride, 16, lane * 16, row * (kHidden * 4), 0, 0);
    }
    if constexpr (kDirectX) load_x_rows(0);
    float c[2][16], h[2][16];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        c[nt][r] = buffer_load_f32(c0rsrc, v_state + nt * 128, ((r & 3) + 8 * (r >> 2)) * (kHidden * 4));
    gemm.bp = wrsrc[kGateOrder[0]];
    gemm.prefetch();
    wait_vmcnt0();
    stage_x();
    __syncthreads();

    for (int t = 0; t < l; ++t) {
      if (t + 1 < l) fetch_x(t + 1);  // lands during the products
      const int64_t row_step0 = b0 * l + t;  // tile row 0 at this step (row pitch l)
      const __amdgpu_buffer_rsrc_t hsrsrc =
          buffer_rsrc(hs + row_step0 * kHidden, ((rows - 1) * l + 1) * kHidden * 4);
      const __amdgpu_buffer_rsrc_t csrsrc =
          buffer_rsrc(SAVE ? save_c + row_step0 * kHidden : nullptr, ((rows - 1) * l + 1) * kHidden * 4);
      const __amdgpu_buffer_rsrc_t gsrsrc = buffer_rsrc(
          SAVE ? save_gates + row_step0 * 4 * kHidden : nullptr, ((rows - 1) * l + 1) * 4 * kHidden * 4);
      float p[2][16];
#pragma unroll
      for (int step = 0; step < 4; ++step) {
        const int q = kGateOrder[step];
        f32x16 acc[1][2];
        gemm.run(ht, acc);
        if (step < 3) {
          gemm.bp = wrsrc[kGateOrder[step + 1]];
          gemm.prefetch();
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float a = q == 2 ? tanh_f(acc[0][nt][r]) : sigmoid_f(acc[0][nt][r]);
            if constexpr (SAVE)
              buffer_store_f32(a, gsrsrc, v_gates + nt * 128 + q * (kHidden * 4),
                               ((r & 3) + 8 * (r >> 2)) * l * (4 * kHidden * 4));
            if (q == 0) {
              p[nt][r] = a;
            } else if (q == 2) {
              p[nt][r] *= a;
            } else if (q == 1) {
              c[nt][r] = __builtin_fmaf(a, c[nt][r], p[nt][r]);
            } else {
              h[nt][r] = a * tanh_f(c[nt][r]);
            }
          }
      }
      __syncthreads();  // every wave has read the tile for all four gates
      if constexpr (kDirectX)
        if (t + 1 < l) load_x_rows(t + 1);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int sr = (r & 3) + 8 * (r >> 2);
          ht[(sr + 4 * hh) * kStride + 64 * wave + 32 * nt + l31] = h[nt][r];
          buffer_store_f32(h[nt][r], hsrsrc, v_seq + nt * 128, sr * l * (kHidden * 4));
          if constexpr (SAVE) buffer_store_f32(c[nt][r], csrsrc, v_seq + nt * 128, sr * l * (kHidden * 4));
        }
      if (t + 1 < l) {
        stage_x();
        gemm.bp = wrsrc[kGateOrder[0]];
        gemm.prefetch();
        if constexpr (kDirectX) wait_vmcnt0();
      }
      __syncthreads();
    }
    // final states
    const __amdgpu_buffer_rsrc_t hnrsrc = buffer_rsrc(hn + b0 * kHidden, rows * kHidden * 4);
    const __amdgpu_buffer_rsrc_t cnrsrc = buffer_rsrc(cn + b0 * kHidden, rows * kHidden * 4);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int sr = (r & 3) + 8 * (r >> 2);
        buffer_store_f32(h[nt][r], hnrsrc, v_state + nt * 128, sr * (kHidden * 4));
        buffer_store_f32(c[nt][r], cnrsrc, v_state + nt * 128, sr * (kHidden * 4));
      }
  }
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

template <int XG, bool SAVE>
static int launch_forward(int grid, hipStream_t s, const float *x, int64_t b, int l, int d_in, const float *h0,
                          const float *c0, const float *w_packed, float *hs, float *hn, float *cn, float *save_gates,
                          float *save_c) {
  if (const int e = allow_dynamic_lds<&lstm_wide_in_forward_kernel<XG, SAVE>>()) return e;
  lstm_wide_in_forward_kernel<XG, SAVE><<<grid, kBlock, forward_lds_bytes(XG), s>>>(x, b, l, d_in, h0, c0, w_packed, hs, hn,
                                                                                    cn, save_gates, save_c);
  return launch_status();
}

}  // namespace lstm_wide_in
}  // namespace rl8
