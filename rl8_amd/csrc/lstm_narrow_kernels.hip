// Narrow LSTMs: one layer, biased, batch_first, fp32, hidden width H = 64 or 128 and
// d_in <= 16 inputs (the reference's recurrent example is nn.LSTM(4, 64)).  The
// 256-wide LSTM runs lstm_kernels.hip / lstm_split_kernels.hip / lstm_rows_kernels.hip;
// only the gate non-linearities (lstm_gates.hip.h) are shared with them.
// Layers 1.. of a stack (num_layers >= 2) run the lstm_narrow_stack_* kernels further down, on an H-wide input.
//
// Layout: a workgroup has H / 16 waves; wave w owns hidden units [16w, 16w + 16) of
// all four gates for every row of the tile, on v_mfma_f32_16x16x4_f32 (exact
// k-ordered fp32 fma chains).  Lane l holds, per 16-row block mt, rows
// 16 mt + 4 (l >> 4) + r (r < 4) of unit 16 w + (l & 15): i, f, g, o and c of one
// (row, unit) sit in the same lane and slot, so the cell update runs on the
// accumulators.
//
// MFMA operand maps (16x16x4 f32): lane l holds A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15]; D[row = 4 (l >> 4) + r][col = l & 15], r < 4.  Over a
// k-group of 16 the lane's four steps use k = 16 g + 4 (l >> 4) + e, e = 0..3, so an
// operand stored along k is one ds_read_b128.
//
// Forward: the weights stay in registers for the whole kernel (W_hh: H floats per
// lane, W_ih: KIN, the summed biases: 4); the operand row [h_{t-1} | x_t] of each
// sequence of the tile is in LDS.  Per step acc = b_ih + b_hh + [h_{t-1} | x_t] x
// [W_hh | W_ih]^T, then the gates and the cell update on the accumulators; h_t goes
// back to LDS for the next step.  The time loop runs inside the kernel; SAVE also
// stores the post-activation gates [B][L][4][H] (torch order i, f, g, o) and the
// cell states [B][L][H] for the backward.
//
// Backward through time (reverse steps): the gate gradients dz from the saved gates /
// cell states and dL/dh_t (the caller's plus the carry), dh_{t-1} = dz x W_hh (MFMA:
// dz through LDS, W_hh in registers), dc carried.  dz goes to the workspace;
// lstm_narrow_wgrad_kernel forms dW = dz^T x [h_{t-1} | x_t | 1] per (sequence chunk,
// 64 gate columns) workgroup with k over rows -- fp32 over 64 rows, fp64 beyond -- and
// writes one slab per chunk; lstm_narrow_reduce_kernel adds the slabs in chunk order
// in fp64.  Every grid is a function of b alone, so the gradients repeat bit for bit.
// No gradient is formed for h0 or c0; the one for x is a launch of its own (lstm_narrow_input_grad_kernel, below the
// stack kernels) for callers with learned parameters in front of the LSTM.
//
// LDS: forward [R][H + KIN + 4] (R = 32 / 16 rows at H = 64 / 128: 9-11 KiB), backward [32][4H + 4] (33 / 66 KiB),
// weight gradient 64 rows of dz (64 columns) and of [h | x | 1] (<= 61 KiB).
#include "lstm_gates.hip.h"
#include "mfma_tile.hip.h"

namespace rl8 {
namespace lstm_narrow {

constexpr int kMaxIn = 16;

template <int H>
struct Geo {
  static constexpr int kWaves = H / 16;           // one wave per 16 hidden units
  static constexpr int kThreads = 64 * kWaves;
  static constexpr int MT = H == 64 ? 2 : 1;      // forward: 16-row blocks per tile
  static constexpr int R = 16 * MT;               // forward: sequences per tile
  static constexpr int kWgPerCU = H == 64 ? 2 : 1;
  static constexpr int MTB = 2;                   // backward: 16-row blocks per tile
  static constexpr int RB = 16 * MTB;             // backward: sequences per tile
  static constexpr int LD = 4 * H + 4;            // backward: LDS row pitch of dz
  static constexpr int kChunks = H == 64 ? 256 : 128;  // weight gradient: most sequence chunks (slabs)
  static_assert(H == 64 || H == 128, "narrow LSTM: H = 64 or 128");
};

template <int H, int KIN>
constexpr int fwd_pitch() { return H + KIN + 4; }

// Weight gradient: B columns [h (H) | x (KIN) | 1 | 0 ..] padded to 16-column tiles.
template <int H, int KIN>
constexpr int wgrad_cols() { return H + (KIN == 4 ? 16 : 32); }
template <int H, int KIN>
constexpr int wgrad_pitch() { return wgrad_cols<H, KIN>() % 32 == 16 ? wgrad_cols<H, KIN>() : wgrad_cols<H, KIN>() + 16; }
constexpr int kWgradRows = 64;    // rows per stage
constexpr int kWgradZPitch = 80;  // LDS pitch of the dz stage (64 columns)
constexpr int kWgradThreads = 256;

__host__ __device__ inline int64_t grad_floats(int hidden, int d_in) { return (int64_t)4 * hidden * (hidden + d_in + 1); }

// Sequences per weight-gradient chunk and the chunk count: functions of b alone.
template <int H>
inline void chunks_for(int64_t b, int64_t *per, int *count) {
  const int64_t want = b < Geo<H>::kChunks ? b : Geo<H>::kChunks;
  *per = (b + want - 1) / want;
  *count = (int)((b + *per - 1) / *per);
}

template <int H>
inline int tile_grid(int64_t b, int rows) {
  const int64_t tiles = (b + rows - 1) / rows;
  const int64_t cap = (int64_t)kCUs * Geo<H>::kWgPerCU;
  return (int)(tiles < cap ? tiles : cap);
}

// x_t of a tile's rows in registers (a load issued a step ahead), then into LDS
// columns [H, H + KIN) (zeros past d_in and past b: offsets outside the descriptor).
template <int H, int KIN>
struct XRegs {
  static constexpr int kN = Geo<H>::R * KIN;
  static constexpr int kPer = (kN + Geo<H>::kThreads - 1) / Geo<H>::kThreads;
  float v[kPer];
  int off[kPer];  // byte offset of this thread's elements in the tile's [rows][l][d_in] block, at t = 0
  __device__ __forceinline__ void begin(int l, int d_in, int tid) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int e = tid + Geo<H>::kThreads * u, r = e / KIN, k = e % KIN;
      off[u] = (e < kN && k < d_in) ? (r * l * d_in + k) * 4 : 0x7fffffff;
    }
  }
  __device__ __forceinline__ void fetch(__amdgpu_buffer_rsrc_t xr, int t, int d_in) {
#pragma unroll
    for (int u = 0; u < kPer; ++u)
      v[u] = off[u] == 0x7fffffff ? 0.0f : buffer_load_f32(xr, off[u] + t * d_in * 4, 0);
  }
  __device__ __forceinline__ void store(float *tile, int tid) const {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int e = tid + Geo<H>::kThreads * u;
      if (e < kN) tile[(e / KIN) * fwd_pitch<H, KIN>() + H + e % KIN] = v[u];
    }
  }
};

template <int H, int KIN, bool SAVE>
__global__ __launch_bounds__(Geo<H>::kThreads, Geo<H>::kWgPerCU) void lstm_narrow_forward_kernel(
    const float *__restrict__ x, int64_t b, int l, int d_in, const float *__restrict__ h0,
    const float *__restrict__ c0, const float *__restrict__ w_ih, const float *__restrict__ w_hh,
    const float *__restrict__ b_ih, const float *__restrict__ b_hh, float *__restrict__ hs, float *__restrict__ hn,
    float *__restrict__ cn, float *__restrict__ save_gates, float *__restrict__ save_c) {
  using G = Geo<H>;
  constexpr int MT = G::MT, R = G::R, LS = fwd_pitch<H, KIN>(), KS = KIN / 4;
  __shared__ float tile[R * LS];  // [R][LS]: h_{t-1} | x_t | pad
  const int tid = threadIdx.x, lane = tid & 63, qq = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int u = 16 * wave + l16;  // this lane's hidden unit

  // B operands: wh[q][4g + e] = W_hh[qH + u][16g + 4qq + e]; wx[q][s] = W_ih[qH + u][KS qq + s].
  float wh[4][H / 4], wx[4][KS], bias[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t j = (int64_t)q * H + u;
#pragma unroll
    for (int g = 0; g < H / 16; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) wh[q][4 * g + e] = w_hh[j * H + 16 * g + 4 * qq + e];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = KS * qq + s;
      wx[q][s] = k < d_in ? w_ih[j * d_in + k] : 0.0f;
    }
    bias[q] = b_ih[j] + b_hh[j];
  }

  // Lane parts of the byte offsets (rows 4qq + .., unit u): [rows][H] states, [rows][l][H] / [rows][l][4H] sequences.
  const int v_state = (4 * qq * H + u) * 4, v_seq = (4 * qq * l * H + u) * 4, v_gates = (4 * qq * l * 4 * H + u) * 4;
  const int64_t tiles = (b + R - 1) / R;
  XRegs<H, KIN> xr;
  xr.begin(l, d_in, tid);
  float c[MT][4], h[MT][4];
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const int64_t b0 = ti * R;
    const int rows = (int)(b - b0 < R ? b - b0 : R);
    const __amdgpu_buffer_rsrc_t xsr = buffer_rsrc(x + b0 * l * d_in, (uint32_t)(rows * l * d_in) * 4);
    xr.fetch(xsr, 0, d_in);
    __syncthreads();  // the previous tile's readers of the tile are done
    for (int i = tid; i < R * H; i += G::kThreads) {
      const int r = i / H, j = i % H;
      tile[r * LS + j] = b0 + r < b ? h0[(b0 + r) * H + j] : 0.0f;
    }
    xr.store(tile, tid);
    // Per-tile / per-step buffer descriptors, the whole byte offset in the VGPR (which the range check covers):
    // rows past b fall outside the descriptor (loads 0, stores dropped).
    const __amdgpu_buffer_rsrc_t c0r = buffer_rsrc(c0 + b0 * H, (uint32_t)rows * H * 4);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) c[mt][r] = buffer_load_f32(c0r, v_state + (16 * mt + r) * H * 4, 0);
    __syncthreads();

    for (int t = 0; t < l; ++t) {
      const int64_t rs0 = b0 * l + t;  // (tile row 0, step t); row pitch l
      const uint32_t span = (uint32_t)((rows - 1) * l + 1) * 4;
      const __amdgpu_buffer_rsrc_t hsr = buffer_rsrc(hs + rs0 * H, span * H);
      const __amdgpu_buffer_rsrc_t gsr = buffer_rsrc(SAVE ? save_gates + rs0 * 4 * H : nullptr, span * 4 * H);
      const __amdgpu_buffer_rsrc_t csr = buffer_rsrc(SAVE ? save_c + rs0 * H : nullptr, span * H);
      if (t + 1 < l) xr.fetch(xsr, t + 1, d_in);  // lands during the products
      f32x4 acc[MT][4];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[mt][q] = f32x4{bias[q], bias[q], bias[q], bias[q]};
      // k-groups of 16 with the next group's operands read a group ahead; the fence keeps the compiler from
      // hoisting every group's reads (registers beyond the budget: scratch)
      f32x4 a[MT], an[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4 *>(tile + (16 * mt + l16) * LS + 4 * qq);
#pragma unroll
      for (int g = 0; g < H / 16; ++g) {
        if (g + 1 < H / 16) {
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
              acc[mt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][e], wh[q][4 * g + e], acc[mt][q], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = an[mt];
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const float a = tile[(16 * mt + l16) * LS + H + KS * qq + s];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            acc[mt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wx[q][s], acc[mt][q], 0, 0, 0);
        }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ig = sigmoid_f(acc[mt][0][r]), fg = sigmoid_f(acc[mt][1][r]);
          const float gg = tanh_f(acc[mt][2][r]), og = sigmoid_f(acc[mt][3][r]);
          c[mt][r] = __builtin_fmaf(fg, c[mt][r], ig * gg);
          h[mt][r] = og * tanh_f(c[mt][r]);
          const int sr = 16 * mt + r;
          buffer_store_f32(h[mt][r], hsr, v_seq + sr * l * H * 4, 0);
          if constexpr (SAVE) {
            buffer_store_f32(ig, gsr, v_gates + (sr * l * 4 * H) * 4, 0);
            buffer_store_f32(fg, gsr, v_gates + (sr * l * 4 * H + H) * 4, 0);
            buffer_store_f32(gg, gsr, v_gates + (sr * l * 4 * H + 2 * H) * 4, 0);
            buffer_store_f32(og, gsr, v_gates + (sr * l * 4 * H + 3 * H) * 4, 0);
            buffer_store_f32(c[mt][r], csr, v_seq + sr * l * H * 4, 0);
          }
        }
      __syncthreads();  // every wave has read h_{t-1} and x_t
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(16 * mt + 4 * qq + r) * LS + u] = h[mt][r];
      if (t + 1 < l) xr.store(tile, tid);
      __syncthreads();
    }
    const __amdgpu_buffer_rsrc_t hnr = buffer_rsrc(hn + b0 * H, (uint32_t)rows * H * 4);
    const __amdgpu_buffer_rsrc_t cnr = buffer_rsrc(cn + b0 * H, (uint32_t)rows * H * 4);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        buffer_store_f32(h[mt][r], hnr, v_state + (16 * mt + r) * H * 4, 0);
        buffer_store_f32(c[mt][r], cnr, v_state + (16 * mt + r) * H * 4, 0);
      }
  }
}

// Backward through time over b sequences of l steps; dz [b][l][4][H] (pre-activation gate gradients) out.
template <int H>
__global__ __launch_bounds__(Geo<H>::kThreads, Geo<H>::kWgPerCU) void lstm_narrow_backward_kernel(
    int64_t b, int l, const float *__restrict__ c0, const float *__restrict__ w_hh, const float *__restrict__ gates,
    const float *__restrict__ cs, const float *__restrict__ dhs, float *__restrict__ dz) {
  constexpr bool HEADS = false;
  const float *heads_dout = nullptr, *heads_w = nullptr;
#include "lstm_narrow_backward_body.hip.h"
}

// The same with dL/dh_t formed from heads_dout [b][l][4] and heads_w [4][H] (zero-padded beyond the heads' outputs)
// instead of read from dhs [b][l][H].
template <int H>
__global__ __launch_bounds__(Geo<H>::kThreads, Geo<H>::kWgPerCU) void lstm_narrow_backward_heads_kernel(
    int64_t b, int l, const float *__restrict__ c0, const float *__restrict__ w_hh, const float *__restrict__ gates,
    const float *__restrict__ cs, const float *__restrict__ heads_dout, const float *__restrict__ heads_w,
    float *__restrict__ dz) {
  constexpr bool HEADS = true;
  const float *dhs = nullptr;
#include "lstm_narrow_backward_body.hip.h"
}

// dW[j][k] += sum over the chunk's rows (b, t) of dz[b][t][j] * a[b][t][k], a = [h_{t-1} (h0 at t = 0) | x_t | 1 | 0..]:
// blockIdx.x = sequence chunk, blockIdx.y = 64 gate columns, wave w = 16 of them x all KW columns.  One slab per
// chunk in the gradient layout [dW_ih (4H d_in) | dW_hh (4H H) | db (4H)].
template <int H, int KIN>
__global__ __launch_bounds__(kWgradThreads, 2) void lstm_narrow_wgrad_kernel(
    const float *__restrict__ x, int64_t b, int l, int d_in, const float *__restrict__ h0,
    const float *__restrict__ hs, const float *__restrict__ dz, int64_t per_chunk, float *__restrict__ slabs) {
  constexpr int KW = wgrad_cols<H, KIN>(), AS = wgrad_pitch<H, KIN>(), ZS = kWgradZPitch, NT = KW / 16;
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
    // The wave's 16 rows of the stage: sources first, then every load in flight at once, then the LDS stores.
    constexpr int kRowsPerWave = kWgradRows / 4, NK = (KW + 63) / 64;
    const float *hp[kRowsPerWave];
#pragma unroll
    for (int i = 0; i < kRowsPerWave; ++i) {
      hp[i] = t > 0 ? hs + (rb + wave + 4 * i - 1) * H : h0 + seq * H;
      t += 4;
      while (t >= l) {
        t -= l;
        ++seq;
      }
    }
    float v[kRowsPerWave][NK], zv[kRowsPerWave];
#pragma unroll
    for (int i = 0; i < kRowsPerWave; ++i) {
      const int64_t row = rb + wave + 4 * i;
      const bool valid = row < r1;
#pragma unroll
      for (int n = 0; n < NK; ++n) {
        const int k = lane + 64 * n;
        v[i][n] = !valid || k >= KW ? 0.0f
                  : k < H           ? hp[i][k]
                  : k < H + d_in    ? x[row * d_in + (k - H)]
                                    : (k == H + d_in ? 1.0f : 0.0f);
      }
      zv[i] = valid ? dz[row * (4 * H) + j0 + lane] : 0.0f;
    }
    __syncthreads();  // the previous stage's readers are done
#pragma unroll
    for (int i = 0; i < kRowsPerWave; ++i) {
      const int rr = wave + 4 * i;
#pragma unroll
      for (int n = 0; n < NK; ++n)
        if (lane + 64 * n < KW) as[rr * AS + lane + 64 * n] = v[i][n];
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
      const float v = (float)tot[n][r];
      if (k < H) slab[o_hh + j * H + k] = v;
      else if (k < H + d_in) slab[j * d_in + (k - H)] = v;
      else if (k == H + d_in) slab[o_b + j] = v;
    }
}

// grads[e] = sum over the slabs, in slab order, in fp64.
__global__ __launch_bounds__(kBlock) void lstm_narrow_reduce_kernel(const float *__restrict__ slabs, int slab_count,
                                                                    int64_t floats, float *__restrict__ grads) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= floats) return;
  double s = 0.0;
  for (int g = 0; g < slab_count; ++g) s += (double)slabs[(int64_t)g * floats + e];
  grads[e] = (float)s;
}

template <int H, int KIN>
int launch_forward(hipStream_t s, const float *x, int64_t b, int l, int d_in, const float *h0, const float *c0,
                   const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, float *hs, float *hn,
                   float *cn, float *save_gates, float *save_c) {
  const int grid = tile_grid<H>(b, Geo<H>::R);
  if (save_gates)
    lstm_narrow_forward_kernel<H, KIN, true><<<grid, Geo<H>::kThreads, 0, s>>>(
        x, b, l, d_in, h0, c0, w_ih, w_hh, b_ih, b_hh, hs, hn, cn, save_gates, save_c);
  else
    lstm_narrow_forward_kernel<H, KIN, false><<<grid, Geo<H>::kThreads, 0, s>>>(
        x, b, l, d_in, h0, c0, w_ih, w_hh, b_ih, b_hh, hs, hn, cn, save_gates, save_c);
  return launch_status();
}

template <int H>
int launch_backward(hipStream_t s, int64_t b, int l, const float *c0, const float *w_hh, const float *gates,
                    const float *cs, const float *dhs, float *dz) {
  constexpr size_t bytes = sizeof(float) * Geo<H>::RB * Geo<H>::LD;
  static_assert(bytes * Geo<H>::kWgPerCU <= 160 * 1024, "backward LDS");
  constexpr auto *kernel = &lstm_narrow_backward_kernel<H>;
  if (const int e = allow_dynamic_lds<kernel>((int)bytes)) return e;
  kernel<<<tile_grid<H>(b, Geo<H>::RB), Geo<H>::kThreads, bytes, s>>>(b, l, c0, w_hh, gates, cs, dhs, dz);
  return launch_status();
}

template <int H>
int launch_backward_heads(hipStream_t s, int64_t b, int l, const float *c0, const float *w_hh, const float *gates,
                          const float *cs, const float *heads_dout, const float *heads_w, float *dz) {
  constexpr size_t bytes = sizeof(float) * Geo<H>::RB * Geo<H>::LD;
  constexpr auto *kernel = &lstm_narrow_backward_heads_kernel<H>;
  if (const int e = allow_dynamic_lds<kernel>((int)bytes)) return e;
  kernel<<<tile_grid<H>(b, Geo<H>::RB), Geo<H>::kThreads, bytes, s>>>(b, l, c0, w_hh, gates, cs, heads_dout, heads_w,
                                                                      dz);
  return launch_status();
}

template <int H, int KIN>
int launch_wgrad(hipStream_t s, const float *x, int64_t b, int l, int d_in, const float *h0, const float *hs,
                 const float *dz, float *slabs) {
  int64_t per = 0;
  int count = 0;
  chunks_for<H>(b, &per, &count);
  lstm_narrow_wgrad_kernel<H, KIN><<<dim3(count, 4 * H / 64), kWgradThreads, 0, s>>>(x, b, l, d_in, h0, hs, dz, per,
                                                                                      slabs);
  return launch_status();
}

// ---- Stacked LSTMs: layers 1.. of nn.LSTM(d_in, H, num_layers >= 2), whose input is the lower layer's h_t (H floats
// wide).  A second H-wide weight block does not fit the forward's registers, so the input product leaves the time
// loop: lstm_narrow_stack_proj_kernel forms zin[n][4][H] = b_ih + b_hh + x[n] x W_ih^T for all n = b l row-steps
// (W_ih in registers in the layout W_hh has in the forward, 32 row-steps per tile, the next tile's rows loaded into
// registers during the products); lstm_narrow_stack_forward_kernel is the forward step with the accumulators loaded
// from zin[b][t] (a step ahead) and the LDS row [h_{t-1}] alone.  The backward through time is
// lstm_narrow_backward_kernel as it is; lstm_narrow_stack_dx_kernel then forms dx[n] = dz[n] x W_ih (the lower layer's
// dL/dhs) over row-steps, with the operand maps of the backward's dh_{t-1} product, and lstm_narrow_stack_wgrad_kernel
// the slabs [dW_ih (4H H) | dW_hh (4H H) | db (4H)] in two launches: columns [h_{t-1}] and columns [x_t | 1].  Every
// k order is fixed and every grid a function of b and l, so zin does not depend on the grid and the gradients repeat
// bit for bit.
//
// HBM traffic of a training pass per row-step and upper layer, in floats: projection H + 4H, forward 4H (zin) + 6H
// (hs, gates, cell states), backward through time 11H, dx 4H + H, weight gradient 2 x 4H (dz, once per launch) + 2H:
// 4 x 41H bytes (10.25 KiB at H = 64, 20.5 KiB at H = 128) against 4 (22H + 2 d_in) for layer 0.  zin (4H floats
// per row-step) lives for the forward only; dz is reused from layer to layer.
constexpr int kStackRows = 32;  // row-steps per tile of the projection and of dx

template <int H>
__global__ __launch_bounds__(Geo<H>::kThreads, Geo<H>::kWgPerCU) void lstm_narrow_stack_proj_kernel(
    const float *__restrict__ x, int64_t n, const float *__restrict__ w_ih, const float *__restrict__ b_ih,
    const float *__restrict__ b_hh, float *__restrict__ zin) {
  using G = Geo<H>;
  constexpr int MT = kStackRows / 16, R = kStackRows, LS = H + 4, kPer = R * H / G::kThreads;
  __shared__ float tile[R * LS];  // [R][LS]: x rows
  const int tid = threadIdx.x, lane = tid & 63, qq = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int u = 16 * wave + l16;

  // B operand as W_hh in the forward: wh[q][4g + e] = W_ih[qH + u][16g + 4qq + e].
  float wh[4][H / 4], bias[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t j = (int64_t)q * H + u;
#pragma unroll
    for (int g = 0; g < H / 16; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) wh[q][4 * g + e] = w_ih[j * H + 16 * g + 4 * qq + e];
    bias[q] = b_ih[j] + b_hh[j];
  }
  const int v_z = (4 * qq * 4 * H + u) * 4;
  const int64_t tiles = (n + R - 1) / R;
  // The tile's R H floats are contiguous: element tid + kThreads i sits at that float offset (0 past the last row).
  float pv[kPer];
  auto fetch = [&](int64_t ti) {
    const int64_t n0 = ti * R;
    const int rows = (int)(n - n0 < R ? n - n0 : R);
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(x + n0 * H, (uint32_t)rows * H * 4);
#pragma unroll
    for (int i = 0; i < kPer; ++i) pv[i] = buffer_load_f32(xr, (tid + G::kThreads * i) * 4, 0);
  };
  if ((int64_t)blockIdx.x < tiles) fetch(blockIdx.x);
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const int64_t n0 = ti * R;
    const int rows = (int)(n - n0 < R ? n - n0 : R);
    __syncthreads();  // the previous tile's readers are done
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int e = tid + G::kThreads * i;
      tile[(e / H) * LS + e % H] = pv[i];
    }
    __syncthreads();
    if (ti + gridDim.x < tiles) fetch(ti + gridDim.x);  // lands during the products
    f32x4 acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[mt][q] = f32x4{bias[q], bias[q], bias[q], bias[q]};
    f32x4 a[MT], an[MT];  // (read a group ahead, fenced: as in the forward)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4 *>(tile + (16 * mt + l16) * LS + 4 * qq);
#pragma unroll
    for (int g = 0; g < H / 16; ++g) {
      if (g + 1 < H / 16) {
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
            acc[mt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][e], wh[q][4 * g + e], acc[mt][q], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = an[mt];
      __builtin_amdgcn_sched_barrier(0);
    }
    // (rows past n fall outside the descriptor: stores dropped)
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

template <int H, bool SAVE>
__global__ __launch_bounds__(Geo<H>::kThreads, Geo<H>::kWgPerCU) void lstm_narrow_stack_forward_kernel(
    const float *__restrict__ zin, int64_t b, int l, const float *__restrict__ h0, const float *__restrict__ c0,
    const float *__restrict__ w_hh, float *__restrict__ hs, float *__restrict__ hn, float *__restrict__ cn,
    float *__restrict__ save_gates, float *__restrict__ save_c) {
  using G = Geo<H>;
  constexpr int MT = G::MT, R = G::R, LS = H + 4;
  __shared__ float tile[R * LS];  // [R][LS]: h_{t-1} | pad
  const int tid = threadIdx.x, lane = tid & 63, qq = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int u = 16 * wave + l16;

  float wh[4][H / 4];  // wh[q][4g + e] = W_hh[qH + u][16g + 4qq + e]
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int g = 0; g < H / 16; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) wh[q][4 * g + e] = w_hh[((int64_t)q * H + u) * H + 16 * g + 4 * qq + e];

  const int v_state = (4 * qq * H + u) * 4, v_seq = (4 * qq * l * H + u) * 4, v_gates = (4 * qq * l * 4 * H + u) * 4;
  const int64_t tiles = (b + R - 1) / R;
  float c[MT][4], h[MT][4];
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const int64_t b0 = ti * R;
    const int rows = (int)(b - b0 < R ? b - b0 : R);
    // (descriptors as in lstm_narrow_forward_kernel: rows past b read 0 and drop their stores)
    const uint32_t span = (uint32_t)((rows - 1) * l + 1) * 4;
    f32x4 zn[MT][4];  // zin of the next step, loaded a step ahead
    auto fetch = [&](int t) {
      const __amdgpu_buffer_rsrc_t zr = buffer_rsrc(zin + (b0 * l + t) * 4 * H, span * 4 * H);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            zn[mt][q][r] = buffer_load_f32(zr, v_gates + ((16 * mt + r) * l * 4 * H + q * H) * 4, 0);
    };
    fetch(0);
    __syncthreads();  // the previous tile's readers of the tile are done
    for (int i = tid; i < R * H; i += G::kThreads) {
      const int r = i / H, j = i % H;
      tile[r * LS + j] = b0 + r < b ? h0[(b0 + r) * H + j] : 0.0f;
    }
    const __amdgpu_buffer_rsrc_t c0r = buffer_rsrc(c0 + b0 * H, (uint32_t)rows * H * 4);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) c[mt][r] = buffer_load_f32(c0r, v_state + (16 * mt + r) * H * 4, 0);
    __syncthreads();

    for (int t = 0; t < l; ++t) {
      const int64_t rs0 = b0 * l + t;
      const __amdgpu_buffer_rsrc_t hsr = buffer_rsrc(hs + rs0 * H, span * H);
      const __amdgpu_buffer_rsrc_t gsr = buffer_rsrc(SAVE ? save_gates + rs0 * 4 * H : nullptr, span * 4 * H);
      const __amdgpu_buffer_rsrc_t csr = buffer_rsrc(SAVE ? save_c + rs0 * H : nullptr, span * H);
      f32x4 acc[MT][4];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[mt][q] = zn[mt][q];
      if (t + 1 < l) fetch(t + 1);  // lands during the products
      f32x4 a[MT], an[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f32x4 *>(tile + (16 * mt + l16) * LS + 4 * qq);
#pragma unroll
      for (int g = 0; g < H / 16; ++g) {
        if (g + 1 < H / 16) {
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
              acc[mt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][e], wh[q][4 * g + e], acc[mt][q], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = an[mt];
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ig = sigmoid_f(acc[mt][0][r]), fg = sigmoid_f(acc[mt][1][r]);
          const float gg = tanh_f(acc[mt][2][r]), og = sigmoid_f(acc[mt][3][r]);
          c[mt][r] = __builtin_fmaf(fg, c[mt][r], ig * gg);
          h[mt][r] = og * tanh_f(c[mt][r]);
          const int sr = 16 * mt + r;
          buffer_store_f32(h[mt][r], hsr, v_seq + sr * l * H * 4, 0);
          if constexpr (SAVE) {
            buffer_store_f32(ig, gsr, v_gates + (sr * l * 4 * H) * 4, 0);
            buffer_store_f32(fg, gsr, v_gates + (sr * l * 4 * H + H) * 4, 0);
            buffer_store_f32(gg, gsr, v_gates + (sr * l * 4 * H + 2 * H) * 4, 0);
            buffer_store_f32(og, gsr, v_gates + (sr * l * 4 * H + 3 * H) * 4, 0);
            buffer_store_f32(c[mt][r], csr, v_seq + sr * l * H * 4, 0);
          }
        }
      __syncthreads();  // every wave has read h_{t-1}
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(16 * mt + 4 * qq + r) * LS + u] = h[mt][r];
      __syncthreads();
    }
    const __amdgpu_buffer_rsrc_t hnr = buffer_rsrc(hn + b0 * H, (uint32_t)rows * H * 4);
    const __amdgpu_buffer_rsrc_t cnr = buffer_rsrc(cn + b0 * H, (uint32_t)rows * H * 4);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        buffer_store_f32(h[mt][r], hnr, v_state + (16 * mt + r) * H * 4, 0);
        buffer_store_f32(c[mt][r], cnr, v_state + (16 * mt + r) * H * 4, 0);
      }
  }
}

// dx[n][H] = dz[n][4H] x W_ih over n row-steps: wave w forms units [16w, 16w + 16) of the tile's 32 rows.
template <int H>
__global__ __launch_bounds__(Geo<H>::kThreads, Geo<H>::kWgPerCU) void lstm_narrow_stack_dx_kernel(
    int64_t n, const float *__restrict__ w_ih, const float *__restrict__ dz, float *__restrict__ dx) {
  using G = Geo<H>;
  constexpr int MT = kStackRows / 16, R = kStackRows, LD = G::LD, kPer = R * 4 * H / G::kThreads;
  extern __shared__ float lds[];  // [R][LD]: dz rows
  const int tid = threadIdx.x, lane = tid & 63, qq = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int u = 16 * wave + l16;

  float wt[H];  // wt[4g + e] = W_ih[16g + 4qq + e][u], k over the 4H gate columns
#pragma unroll
  for (int g = 0; g < H / 4; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) wt[4 * g + e] = w_ih[(int64_t)(16 * g + 4 * qq + e) * H + u];

  const int64_t tiles = (n + R - 1) / R;
  float pv[kPer];  // (the next tile's rows in registers, as in the projection)
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
    if (ti + gridDim.x < tiles) fetch(ti + gridDim.x);
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 a[MT], an[MT];
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
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][e], wt[4 * g + e], acc[mt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = an[mt];
      __builtin_amdgcn_sched_barrier(0);
    }
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(dx + n0 * H, (uint32_t)rows * H * 4);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) buffer_store_f32(acc[mt][r], xr, ((16 * mt + 4 * qq + r) * H + u) * 4, 0);
  }
}

// lstm_narrow_wgrad_kernel for an H-wide x, half of the columns per launch: XPART = false a = [h_{t-1} (h0 at t = 0)]
// -> dW_hh, XPART = true a = [x_t | 1 | 0..] -> dW_ih and db.  One slab per chunk: [dW_ih (4H H) | dW_hh (4H H) | db].
template <int H, bool XPART>
__global__ __launch_bounds__(kWgradThreads, 2) void lstm_narrow_stack_wgrad_kernel(
    const float *__restrict__ x, int64_t b, int l, const float *__restrict__ h0, const float *__restrict__ hs,
    const float *__restrict__ dz, int64_t per_chunk, float *__restrict__ slabs) {
  constexpr int KW = XPART ? H + 16 : H, AS = KW % 32 == 16 ? KW : KW + 16, ZS = kWgradZPitch, NT = KW / 16;
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
  int64_t seq = s0 + wave / l;  // (sequence, step) of the wave's next row, as in lstm_narrow_wgrad_kernel
  int t = wave % l;
  for (int64_t rb = r0; rb < r1; rb += kWgradRows) {
    constexpr int kRowsPerWave = kWgradRows / 4, NK = (KW + 63) / 64;
    const float *ap[kRowsPerWave];
#pragma unroll
    for (int i = 0; i < kRowsPerWave; ++i) {
      if constexpr (XPART) {
        ap[i] = x + (rb + wave + 4 * i) * H;
      } else {
        ap[i] = t > 0 ? hs + (rb + wave + 4 * i - 1) * H : h0 + seq * H;
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
      const int64_t row = rb + wave + 4 * i;
      const bool valid = row < r1;
#pragma unroll
      for (int n = 0; n < NK; ++n) {
        const int k = lane + 64 * n;
        v[i][n] = !valid || k >= KW ? 0.0f : k < H ? ap[i][k] : (k == H ? 1.0f : 0.0f);
      }
      zv[i] = valid ? dz[row * (4 * H) + j0 + lane] : 0.0f;
    }
    __syncthreads();  // the previous stage's readers are done
#pragma unroll
    for (int i = 0; i < kRowsPerWave; ++i) {
      const int rr = wave + 4 * i;
#pragma unroll
      for (int n = 0; n < NK; ++n)
        if (lane + 64 * n < KW) as[rr * AS + lane + 64 * n] = v[i][n];
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

  float *slab = slabs + (int64_t)blockIdx.x * grad_floats(H, H);
  constexpr int o_hh = 4 * H * H, o_b = 2 * o_hh;
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + 16 * wave + 4 * qq + r, k = 16 * n + l16;
      const float v = (float)tot[n][r];
      if constexpr (XPART) {
        if (k < H) slab[j * H + k] = v;
        else if (k == H) slab[o_b + j] = v;
      } else {
        slab[o_hh + j * H + k] = v;
      }
    }
}

template <int H>
inline int stack_grid(int64_t n) {
  const int64_t tiles = (n + kStackRows - 1) / kStackRows;
  const int64_t cap = (int64_t)kCUs * Geo<H>::kWgPerCU;
  return (int)(tiles < cap ? tiles : cap);
}

template <int H>
int launch_stack_forward(hipStream_t s, const float *x, int64_t b, int l, const float *h0, const float *c0,
                         const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, float *zin,
                         float *hs, float *hn, float *cn, float *save_gates, float *save_c) {
  lstm_narrow_stack_proj_kernel<H><<<stack_grid<H>(b * l), Geo<H>::kThreads, 0, s>>>(x, b * l, w_ih, b_ih, b_hh, zin);
  if (const int st = launch_status()) return st;
  const int grid = tile_grid<H>(b, Geo<H>::R);
  if (save_gates)
    lstm_narrow_stack_forward_kernel<H, true><<<grid, Geo<H>::kThreads, 0, s>>>(zin, b, l, h0, c0, w_hh, hs, hn, cn,
                                                                                save_gates, save_c);
  else
    lstm_narrow_stack_forward_kernel<H, false><<<grid, Geo<H>::kThreads, 0, s>>>(zin, b, l, h0, c0, w_hh, hs, hn, cn,
                                                                                 save_gates, save_c);
  return launch_status();
}

template <int H>
int launch_stack_backward(hipStream_t s, const float *x, int64_t b, int l, const float *h0, const float *c0,
                          const float *w_ih, const float *w_hh, const float *hs, const float *gates, const float *cs,
                          const float *dhs, float *dz, float *slabs, float *dx) {
  if (const int st = launch_backward<H>(s, b, l, c0, w_hh, gates, cs, dhs, dz)) return st;
  constexpr size_t bytes = sizeof(float) * kStackRows * Geo<H>::LD;
  static_assert(bytes * Geo<H>::kWgPerCU <= 160 * 1024, "dx LDS");
  constexpr auto *kernel = &lstm_narrow_stack_dx_kernel<H>;
  if (const int e = allow_dynamic_lds<kernel>((int)bytes)) return e;
  kernel<<<stack_grid<H>(b * l), Geo<H>::kThreads, bytes, s>>>(b * l, w_ih, dz, dx);
  if (const int st = launch_status()) return st;
  int64_t per = 0;
  int count = 0;
  chunks_for<H>(b, &per, &count);
  const dim3 grid(count, 4 * H / 64);
  lstm_narrow_stack_wgrad_kernel<H, false><<<grid, kWgradThreads, 0, s>>>(x, b, l, h0, hs, dz, per, slabs);
  if (const int st = launch_status()) return st;
  lstm_narrow_stack_wgrad_kernel<H, true><<<grid, kWgradThreads, 0, s>>>(x, b, l, h0, hs, dz, per, slabs);
  return launch_status();
}

// ---- Input gradient of layer 0 (a model with learned parameters in front of the LSTM: an embedding, an encoder):
// dx[n][d_in] = dz[n][4H] x W_ih over n = b l row-steps, from the dz either backward entry left in the workspace.
// One 16-column output tile (W_ih zero-padded from d_in in registers), 32 row-steps per workgroup tile as in
// lstm_narrow_stack_dx_kernel.  There are only two 16 x 16 output blocks per tile, so the waves split k instead of the
// columns: wave w multiplies gate columns [64w, 64w + 64) of both row blocks -- its A operand is 16 bytes per lane
// straight from HBM (lane l: row l & 15, columns 64w + 16g + 4 (l >> 4) + e: the k-group layout of the operand maps
// above, no LDS staging), the next tile's loads in flight during the products -- and leaves a [32][KIN] partial in
// LDS; the partials are then added in wave order.  Every k order is fixed (within a wave g, e ascending on the MFMA's
// fma chain, then waves ascending), so dx does not depend on the grid and repeats bit for bit.
// HBM per row-step: 4H floats in, d_in out (1 KiB + 4 d_in bytes at H = 64, 2 KiB + 4 d_in at H = 128).
// LDS: [H / 16][32][KIN + 4] floats (4 / 10 KiB at H = 64, 8 / 20 KiB at H = 128 for KIN = 4 / 16).
template <int H, int KIN>
__global__ __launch_bounds__(Geo<H>::kThreads, Geo<H>::kWgPerCU) void lstm_narrow_input_grad_kernel(
    int64_t n, int d_in, const float *__restrict__ w_ih, const float *__restrict__ dz, float *__restrict__ dx) {
  using G = Geo<H>;
  constexpr int MT = kStackRows / 16, R = kStackRows, W = G::kWaves, KG = 4, PS = KIN + 4;
  static_assert(16 * KG * W == 4 * H, "64 gate columns per wave");
  __shared__ float part[W * R * PS];  // [W][R][PS]: each wave's partial sums
  const int tid = threadIdx.x, lane = tid & 63, qq = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  float wt[4 * KG];  // B operand: wt[4g + e] = W_ih[64 wave + 16g + 4qq + e][l16], zero past d_in
#pragma unroll
  for (int g = 0; g < KG; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      wt[4 * g + e] = l16 < d_in ? w_ih[(int64_t)(64 * wave + 16 * g + 4 * qq + e) * d_in + l16] : 0.0f;

  const int v_z = (l16 * 4 * H + 64 * wave + 4 * qq) * 4;  // row l16 of a 16-row block, this lane's 16 bytes of group 0
  const int64_t tiles = (n + R - 1) / R;
  u32x4 pv[MT][KG];  // (the next tile's operands in registers; rows past n fall outside the descriptor: zeros)
  auto fetch = [&](int64_t ti) {
    const int64_t n0 = ti * R;
    const int rows = (int)(n - n0 < R ? n - n0 : R);
    const __amdgpu_buffer_rsrc_t zr = buffer_rsrc(dz + n0 * 4 * H, (uint32_t)rows * 4 * H * 4);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < KG; ++g)
        pv[mt][g] = __builtin_amdgcn_raw_buffer_load_b128(zr, v_z + (16 * mt * 4 * H + 16 * g) * 4, 0, 0);
  };
  if ((int64_t)blockIdx.x < tiles) fetch(blockIdx.x);
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const int64_t n0 = ti * R;
    const int rows = (int)(n - n0 < R ? n - n0 : R);
    u32x4 a[MT][KG];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < KG; ++g) a[mt][g] = pv[mt][g];
    if (ti + gridDim.x < tiles) fetch(ti + gridDim.x);  // lands during the products and the sum
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int g = 0; g < KG; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[mt][g][e]), wt[4 * g + e], acc[mt], 0, 0, 0);
    __syncthreads();  // the previous tile's sum has read the partials
    if (l16 < KIN) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(wave * R + 16 * mt + 4 * qq + r) * PS + l16] = acc[mt][r];
    }
    __syncthreads();
    // (rows past n fall outside the descriptor: stores dropped)
    const __amdgpu_buffer_rsrc_t xr = buffer_rsrc(dx + n0 * d_in, (uint32_t)(rows * d_in) * 4);
    for (int o = tid; o < R * KIN; o += G::kThreads) {
      const int row = o / KIN, col = o % KIN;
      float s = part[row * PS + col];
#pragma unroll
      for (int w = 1; w < W; ++w) s += part[(w * R + row) * PS + col];
      if (col < d_in) buffer_store_f32(s, xr, (row * d_in + col) * 4, 0);
    }
  }
}

template <int H, int KIN>
int launch_input_grad(hipStream_t s, int64_t n, int d_in, const float *w_ih, const float *dz, float *dx) {
  lstm_narrow_input_grad_kernel<H, KIN><<<stack_grid<H>(n), Geo<H>::kThreads, 0, s>>>(n, d_in, w_ih, dz, dx);
  return launch_status();
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

inline int slab_count(int hidden, int64_t b) {
  int64_t per = 0;
  int count = 0;
  if (hidden == 64) chunks_for<64>(b, &per, &count);
  else chunks_for<128>(b, &per, &count);
  return count;
}

// Floats of dz [b][l][4H] at the front of the workspace (a multiple of four: the slabs stay 16-byte aligned).
inline int64_t dz_floats(int64_t b, int l, int hidden) { return b * l * 4 * hidden; }

}  // namespace lstm_narrow
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_lstm_narrow_supports(int hidden, int d_in) {
  return (hidden == 64 || hidden == 128) && d_in >= 1 && d_in <= lstm_narrow::kMaxIn;
}

// Buffer descriptors address a tile's rows of [b][l][4H] with 32-bit byte offsets (l < 16384 at H = 128); the row
// indices are int64.
static bool lstm_narrow_sizes_ok(int64_t b, int l, int hidden) {
  return b >= 1 && l >= 1 && b * (int64_t)l < ((int64_t)1 << 40) && (int64_t)64 * l * 4 * hidden * 4 < ((int64_t)1 << 31);
}

RL8_API int64_t rl8_lstm_narrow_workspace_bytes(int64_t b, int l, int hidden, int d_in) {
  if (!lstm_narrow_sizes_ok(b, l, hidden) || !rl8_lstm_narrow_supports(hidden, d_in)) return RL8_ESIZE;
  return (lstm_narrow::dz_floats(b, l, hidden) +
          (int64_t)lstm_narrow::slab_count(hidden, b) * lstm_narrow::grad_floats(hidden, d_in)) *
         (int64_t)sizeof(float);
}

RL8_API int rl8_lstm_narrow_forward_f32(const float *x, int64_t b, int l, int d_in, const float *h0, const float *c0,
                                        const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                        int hidden, float *hs, float *hn, float *cn, float *save_gates, float *save_c,
                                        void *stream) {
  if (!x || !h0 || !c0 || !w_ih || !w_hh || !b_ih || !b_hh || !hs || !hn || !cn) return RL8_ENULL;
  if ((save_gates == nullptr) != (save_c == nullptr)) return RL8_ENULL;
  if (!lstm_narrow_sizes_ok(b, l, hidden) || !rl8_lstm_narrow_supports(hidden, d_in)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)h0, (const void *)c0, (const void *)w_ih, (const void *)w_hh,
                        (const void *)b_ih, (const void *)b_hh, (const void *)hs, (const void *)hn, (const void *)cn,
                        (const void *)save_gates, (const void *)save_c})
    if (!lstm_narrow::aligned4(p)) return RL8_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const bool narrow_in = d_in <= 4;
  if (hidden == 64)
    return narrow_in ? lstm_narrow::launch_forward<64, 4>(s, x, b, l, d_in, h0, c0, w_ih, w_hh, b_ih, b_hh, hs, hn, cn,
                                                          save_gates, save_c)
                     : lstm_narrow::launch_forward<64, 16>(s, x, b, l, d_in, h0, c0, w_ih, w_hh, b_ih, b_hh, hs, hn,
                                                           cn, save_gates, save_c);
  return narrow_in ? lstm_narrow::launch_forward<128, 4>(s, x, b, l, d_in, h0, c0, w_ih, w_hh, b_ih, b_hh, hs, hn, cn,
                                                         save_gates, save_c)
                   : lstm_narrow::launch_forward<128, 16>(s, x, b, l, d_in, h0, c0, w_ih, w_hh, b_ih, b_hh, hs, hn, cn,
                                                          save_gates, save_c);
}

RL8_API int rl8_lstm_narrow_backward_f32(const float *x, int64_t b, int l, int d_in, const float *h0, const float *c0,
                                         const float *w_hh, int hidden, const float *hs, const float *gates,
                                         const float *cs, const float *dhs, float *workspace, void *stream) {
  if (!x || !h0 || !c0 || !w_hh || !hs || !gates || !cs || !dhs || !workspace) return RL8_ENULL;
  if (!lstm_narrow_sizes_ok(b, l, hidden) || !rl8_lstm_narrow_supports(hidden, d_in)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)h0, (const void *)c0, (const void *)w_hh, (const void *)hs,
                        (const void *)gates, (const void *)cs, (const void *)dhs})
    if (!lstm_narrow::aligned4(p)) return RL8_EALIGN;
  if (!aligned16(workspace)) return RL8_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  float *dz = workspace, *slabs = workspace + lstm_narrow::dz_floats(b, l, hidden);
  const bool narrow_in = d_in <= 4;
  int st;
  if (hidden == 64) {
    st = lstm_narrow::launch_backward<64>(s, b, l, c0, w_hh, gates, cs, dhs, dz);
    if (st != RL8_OK) return st;
    return narrow_in ? lstm_narrow::launch_wgrad<64, 4>(s, x, b, l, d_in, h0, hs, dz, slabs)
                     : lstm_narrow::launch_wgrad<64, 16>(s, x, b, l, d_in, h0, hs, dz, slabs);
  }
  st = lstm_narrow::launch_backward<128>(s, b, l, c0, w_hh, gates, cs, dhs, dz);
  if (st != RL8_OK) return st;
  return narrow_in ? lstm_narrow::launch_wgrad<128, 4>(s, x, b, l, d_in, h0, hs, dz, slabs)
                   : lstm_narrow::launch_wgrad<128, 16>(s, x, b, l, d_in, h0, hs, dz, slabs);
}

// rl8_lstm_narrow_backward_f32 with dL/dhs given by the output heads it came through (heads_dout [b][l][4], heads_w
// [4][H], both zero-padded beyond the heads' outputs): the same workspace, the same weight-gradient kernel after it.
RL8_API int rl8_lstm_narrow_backward_heads_f32(const float *x, int64_t b, int l, int d_in, const float *h0,
                                               const float *c0, const float *w_hh, int hidden, const float *hs,
                                               const float *gates, const float *cs, const float *heads_dout,
                                               const float *heads_w, float *workspace, void *stream) {
  if (!x || !h0 || !c0 || !w_hh || !hs || !gates || !cs || !heads_dout || !heads_w || !workspace) return RL8_ENULL;
  if (!lstm_narrow_sizes_ok(b, l, hidden) || !rl8_lstm_narrow_supports(hidden, d_in)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)h0, (const void *)c0, (const void *)w_hh, (const void *)hs,
                        (const void *)gates, (const void *)cs, (const void *)heads_w})
    if (!lstm_narrow::aligned4(p)) return RL8_EALIGN;
  if (!aligned16(heads_dout) || !aligned16(workspace)) return RL8_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  float *dz = workspace, *slabs = workspace + lstm_narrow::dz_floats(b, l, hidden);
  const bool narrow_in = d_in <= 4;
  int st;
  if (hidden == 64) {
    st = lstm_narrow::launch_backward_heads<64>(s, b, l, c0, w_hh, gates, cs, heads_dout, heads_w, dz);
    if (st != RL8_OK) return st;
    return narrow_in ? lstm_narrow::launch_wgrad<64, 4>(s, x, b, l, d_in, h0, hs, dz, slabs)
                     : lstm_narrow::launch_wgrad<64, 16>(s, x, b, l, d_in, h0, hs, dz, slabs);
  }
  st = lstm_narrow::launch_backward_heads<128>(s, b, l, c0, w_hh, gates, cs, heads_dout, heads_w, dz);
  if (st != RL8_OK) return st;
  return narrow_in ? lstm_narrow::launch_wgrad<128, 4>(s, x, b, l, d_in, h0, hs, dz, slabs)
                   : lstm_narrow::launch_wgrad<128, 16>(s, x, b, l, d_in, h0, hs, dz, slabs);
}

RL8_API int rl8_lstm_narrow_reduce_f32(const float *workspace, int64_t b, int l, int hidden, int d_in,
                                       float *grads_out, void *stream) {
  if (!workspace || !grads_out) return RL8_ENULL;
  if (!lstm_narrow_sizes_ok(b, l, hidden) || !rl8_lstm_narrow_supports(hidden, d_in)) return RL8_ESIZE;
  if (!aligned16(workspace) || !lstm_narrow::aligned4(grads_out)) return RL8_EALIGN;
  const int64_t floats = lstm_narrow::grad_floats(hidden, d_in);
  lstm_narrow::lstm_narrow_reduce_kernel<<<(unsigned)((floats + kBlock - 1) / kBlock), kBlock, 0,
                                           (hipStream_t)stream>>>(workspace + lstm_narrow::dz_floats(b, l, hidden),
                                                                  lstm_narrow::slab_count(hidden, b), floats,
                                                                  grads_out);
  return launch_status();
}

// dL/dx of layer 0 from the dz that either backward entry above left at the front of `workspace`.
RL8_API int rl8_lstm_narrow_input_grad_f32(const float *workspace, int64_t b, int l, int d_in, const float *w_ih,
                                           int hidden, float *dx, void *stream) {
  if (!workspace || !w_ih || !dx) return RL8_ENULL;
  if (!lstm_narrow_sizes_ok(b, l, hidden) || !rl8_lstm_narrow_supports(hidden, d_in)) return RL8_ESIZE;
  if (!aligned16(workspace) || !lstm_narrow::aligned4(w_ih) || !lstm_narrow::aligned4(dx)) return RL8_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = b * l;
  const bool narrow_in = d_in <= 4;
  if (hidden == 64)
    return narrow_in ? lstm_narrow::launch_input_grad<64, 4>(s, n, d_in, w_ih, workspace, dx)
                     : lstm_narrow::launch_input_grad<64, 16>(s, n, d_in, w_ih, workspace, dx);
  return narrow_in ? lstm_narrow::launch_input_grad<128, 4>(s, n, d_in, w_ih, workspace, dx)
                   : lstm_narrow::launch_input_grad<128, 16>(s, n, d_in, w_ih, workspace, dx);
}

// ---- Stacked LSTMs: one upper layer (its input is H floats wide) per call.

RL8_API int rl8_lstm_stack_supports(int hidden) { return hidden == 64 || hidden == 128; }

RL8_API int64_t rl8_lstm_stack_workspace_bytes(int64_t b, int l, int hidden) {
  if (!rl8_lstm_stack_supports(hidden) || !lstm_narrow_sizes_ok(b, l, hidden)) return RL8_ESIZE;
  return (lstm_narrow::dz_floats(b, l, hidden) +
          (int64_t)lstm_narrow::slab_count(hidden, b) * lstm_narrow::grad_floats(hidden, hidden)) *
         (int64_t)sizeof(float);
}

RL8_API int rl8_lstm_stack_forward_f32(const float *x, int64_t b, int l, const float *h0, const float *c0,
                                       const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                       int hidden, float *zin, float *hs, float *hn, float *cn, float *save_gates,
                                       float *save_c, void *stream) {
  if (!x || !h0 || !c0 || !w_ih || !w_hh || !b_ih || !b_hh || !zin || !hs || !hn || !cn) return RL8_ENULL;
  if ((save_gates == nullptr) != (save_c == nullptr)) return RL8_ENULL;
  if (!rl8_lstm_stack_supports(hidden) || !lstm_narrow_sizes_ok(b, l, hidden)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)h0, (const void *)c0, (const void *)w_ih, (const void *)w_hh,
                        (const void *)b_ih, (const void *)b_hh, (const void *)hs, (const void *)hn, (const void *)cn,
                        (const void *)save_gates, (const void *)save_c})
    if (!lstm_narrow::aligned4(p)) return RL8_EALIGN;
  if (!aligned16(zin)) return RL8_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  return hidden == 64 ? lstm_narrow::launch_stack_forward<64>(s, x, b, l, h0, c0, w_ih, w_hh, b_ih, b_hh, zin, hs, hn,
                                                              cn, save_gates, save_c)
                      : lstm_narrow::launch_stack_forward<128>(s, x, b, l, h0, c0, w_ih, w_hh, b_ih, b_hh, zin, hs,
                                                               hn, cn, save_gates, save_c);
}

RL8_API int rl8_lstm_stack_backward_f32(const float *x, int64_t b, int l, const float *h0, const float *c0,
                                        const float *w_ih, const float *w_hh, int hidden, const float *hs,
                                        const float *gates, const float *cs, const float *dhs, float *workspace,
                                        float *dx, void *stream) {
  if (!x || !h0 || !c0 || !w_ih || !w_hh || !hs || !gates || !cs || !dhs || !workspace || !dx) return RL8_ENULL;
  if (!rl8_lstm_stack_supports(hidden) || !lstm_narrow_sizes_ok(b, l, hidden)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)h0, (const void *)c0, (const void *)w_ih, (const void *)w_hh,
                        (const void *)hs, (const void *)gates, (const void *)cs, (const void *)dhs, (const void *)dx})
    if (!lstm_narrow::aligned4(p)) return RL8_EALIGN;
  if (!aligned16(workspace)) return RL8_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  float *dz = workspace, *slabs = workspace + lstm_narrow::dz_floats(b, l, hidden);
  return hidden == 64 ? lstm_narrow::launch_stack_backward<64>(s, x, b, l, h0, c0, w_ih, w_hh, hs, gates, cs, dhs, dz,
                                                               slabs, dx)
                      : lstm_narrow::launch_stack_backward<128>(s, x, b, l, h0, c0, w_ih, w_hh, hs, gates, cs, dhs, dz,
                                                                slabs, dx);
}

RL8_API int rl8_lstm_stack_reduce_f32(const float *workspace, int64_t b, int l, int hidden, float *grads_out,
                                      void *stream) {
  if (!workspace || !grads_out) return RL8_ENULL;
  if (!rl8_lstm_stack_supports(hidden) || !lstm_narrow_sizes_ok(b, l, hidden)) return RL8_ESIZE;
  if (!aligned16(workspace) || !lstm_narrow::aligned4(grads_out)) return RL8_EALIGN;
  const int64_t floats = lstm_narrow::grad_floats(hidden, hidden);
  lstm_narrow::lstm_narrow_reduce_kernel<<<(unsigned)((floats + kBlock - 1) / kBlock), kBlock, 0,
                                           (hipStream_t)stream>>>(workspace + lstm_narrow::dz_floats(b, l, hidden),
                                                                  lstm_narrow::slab_count(hidden, b), floats,
                                                                  grads_out);
  return launch_status();
}
