// N1, "wide input" family: Linear(d_in, 256) ReLU Linear(256, 256) ReLU Linear(256, n_out) with biased layers,
// 17 <= d_in <= 128, n_out <= 8, in fp32 throughout on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains).  The towers of
// mlp_kernels.hip form layer 1 on the VALU, one thread per column with d_in weights in registers: past 16 inputs that
// neither fits the registers nor pays (fp32 MFMA and VALU do not overlap, mfma_tile.hip.h: at d_in = 128 such a layer 1
// would cost more than layer 2).  Here layer 1 is a k-loop on the matrix cores as well.
//
// Forward (one launch): a workgroup (4 waves) walks 64-row tiles.  The x tile goes to LDS WHOLE, zero-padded to the
// k-granule of 8, into the [64][257] tile that later holds h1 and then h2 -- x is dead once layer 1 sits in the
// accumulators, so it costs one barrier and no LDS of its own.  W1 comes from a fragment-ordered, zero-padded copy
// (rl8_mlp_wide_in_pack_w1_f32: the layout of rl8_mlp_pack_w2_f32 with ceil(d_in / 8) k-groups per column tile), one
// coalesced 256-byte load per MFMA operand through L2.  Layer 2 and the head are those of mlp_tower_forward_kernel
// (TileGemm over rl8_mlp_pack_w2_f32's packing, h2 over h1 in the one tile).  The training variant stores h1 and h2.
//
// Data gradient (one launch per row segment): the tile kernel of mlp_tower_backward_kernel, which here also stores
// dZ1 = (dZ2 W2) . [h1 > 0] and carries no dW1 sums (a thread cannot hold 128 per column); partial row per workgroup
// [db1 (256) | db2 (256) | dW3 (n_out * 256) | db3 (n_out)].  ReLU'(0) = 0.
//
// Input-layer weight gradient: dW1 [256][d_in] (+)= dZ1^T x, k over the rows, after mlp_wgrad_kernel: 8 waves, wave w
// owns the 32 rows 32 w .. of dW1 and all ceil(d_in / 32) column tiles; 32-row tiles of dZ1 arrive by direct-to-LDS
// loads, of x through registers, double-buffered, one barrier per tile.  One slab per workgroup, summed in slab order;
// the grid is a function of the row count alone: bitwise reproducible.  (dW2 = dZ2^T h1 has both operands in memory:
// the existing rl8_mlp_wgrad_split_strided_f32 / rl8_mlp_wgrad_f32 form it.)
//
// LDS (dynamic) and workgroups per CU (160 KiB):
//   forward, both variants : W3^T [256][8] + tile [64][257]                   = 73 984 B, 2 per CU
//   data gradient          : dOut [2][8][64] + tile [64][257]                 = 69 888 B, 2 per CU
//   weight gradient        : 2 x (dZ1 [32][320] + x [32][32 CT + 32]), CT = ceil(d_in / 32) column tiles
//                            = 98 304 / 106 496 / 114 688 / 122 880 B for CT = 1..4, 1 per CU (8 waves)
#include "mfma_tile.hip.h"
#include "tower_launch.hip.h"

namespace rl8 {
namespace wide_in {

constexpr int kMinIn = kMaxIn + 1;  // the towers of mlp_kernels.hip end at kMaxIn
constexpr int kMaxWideIn = 128;

inline bool supports(int d_in, int n_out) {
  return d_in >= kMinIn && d_in <= kMaxWideIn && n_out >= 1 && n_out <= kMaxOut;
}
__host__ __device__ constexpr int k_groups(int d_in) { return (d_in + 7) / 8; }

// w1 [256][d_in] row-major -> fragment order with kg = ceil(d_in / 8) k-groups per column tile, zeros past d_in:
// packed[((n*kg + g)*4 + e)*64 + l] = w1[32n + (l&31)][8g + 4(l>>5) + e]
__global__ __launch_bounds__(kBlock) void mlp_wide_in_pack_w1_kernel(const float *__restrict__ w1, int d_in, int kg,
                                                                     float *__restrict__ packed) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= kHidden * 8 * kg) return;
  const int l = idx & 63, e = (idx >> 6) & 3, ng = idx >> 8, g = ng % kg, n = ng / kg;
  const int k = 8 * g + 4 * (l >> 5) + e;
  packed[idx] = k < d_in ? w1[(32 * n + (l & 31)) * d_in + k] : 0.0f;
}

constexpr size_t forward_lds_bytes() { return sizeof(float) * (kMaxOut * kHidden + kTileRows * kLdsStride); }
constexpr size_t backward_lds_bytes() { return sizeof(float) * (2 * kTileRows * kMaxOut + kTileRows * kLdsStride); }

// KIN: d_in rounded up to 32, 64 or 128 (how many floats of a row a thread block fetches; the k-loop itself runs
// ceil(d_in / 8) groups).  KOUT: n_out rounded up to 2, 4 or 8.  SAVE: also store h1 / h2 ([m][256] each).
template <int KIN, int KOUT, bool SAVE>
__global__ __launch_bounds__(kBlock, 2) void mlp_wide_in_forward_kernel(
    const float *__restrict__ x, int64_t m, int d_in, const float *__restrict__ w1p, const float *__restrict__ b1,
    const float4 *__restrict__ w2p, const float *__restrict__ b2, const float *__restrict__ w3,
    const float *__restrict__ b3, int n_out, float *__restrict__ out, float *__restrict__ save_h1,
    float *__restrict__ save_h2) {
  typedef float outvec __attribute__((ext_vector_type(KOUT)));
  constexpr int kHeadUnroll = KOUT <= 2 ? 64 : 8;
  extern __shared__ float lds[];
  float *w3s = lds;                       // [256][KOUT]: head weights, unit-major
  float *ht = w3s + kMaxOut * kHidden;    // [64][257]: x (columns < 8 kg), then h1, then h2
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5;
  const int kg = k_groups(d_in);

  for (int idx = tid; idx < KOUT * kHidden; idx += kBlock) {
    const int j = idx / KOUT, q = idx - j * KOUT;
    w3s[idx] = q < n_out ? w3[q * kHidden + j] : 0.0f;
  }
  float b1r[2], b2r[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    b1r[nt] = b1[64 * wave + 32 * nt + (lane & 31)];
    b2r[nt] = b2[64 * wave + 32 * nt + (lane & 31)];
  }
  outvec b3r;
#pragma unroll
  for (int q = 0; q < KOUT; ++q) b3r[q] = q < n_out ? b3[q] : 0.0f;
  TileGemm gemm(buffer_rsrc(w2p, kHidden * kHidden * 4), wave, lane);
  // W1 fragments: the wave's two column tiles 2 wave + nt, k-group g at g * 1 KiB (a uniform offset)
  const __amdgpu_buffer_rsrc_t w1rsrc = buffer_rsrc(w1p, kHidden * 8 * kg * 4);
  const int w1voff = (2 * wave) * kg * (kWave * 16) + lane * 4, w1tile = kg * (kWave * 16);
  const int a_off = (lane & 31) * kLdsStride + 4 * hh;
  __builtin_amdgcn_s_setprio(kValuPhasePriority);

  const int64_t tiles = (m + kTileRows - 1) / kTileRows;
  // Observation tile: element (row idx / KIN, column idx % KIN) is owned by thread idx (+256, ...); fetched one tile
  // ahead so that its HBM latency hides under the matrix phases.  Zeros past d_in and past m.
  constexpr int kXPerThread = kTileRows * KIN / kBlock;
  float xreg[kXPerThread];
  auto fetch_x = [&](int64_t tile) {
    const int64_t r0 = tile * kTileRows;
#pragma unroll
    for (int u = 0; u < kXPerThread; ++u) {
      const int idx = tid + u * kBlock, s = idx / KIN, c = idx % KIN;
      xreg[u] = (c < d_in && r0 + s < m) ? x[(r0 + s) * d_in + c] : 0.0f;
    }
  };
  if ((int64_t)blockIdx.x < tiles) fetch_x(blockIdx.x);

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kTileRows;
    const int rows = (int)((m - r0) < kTileRows ? (m - r0) : kTileRows);
    // Stores of this tile's h1 / h2 rows: descriptor based at the tile, sized to its valid rows (stores past the end
    // of a partial tile are dropped).
    const __amdgpu_buffer_rsrc_t h1rsrc = buffer_rsrc(SAVE ? save_h1 + r0 * kHidden : nullptr, rows * kHidden * 4);
    const __amdgpu_buffer_rsrc_t h2rsrc = buffer_rsrc(SAVE ? save_h2 + r0 * kHidden : nullptr, rows * kHidden * 4);
    __syncthreads();  // the previous tile's head has read h2 (and w3s is staged)
#pragma unroll
    for (int u = 0; u < kXPerThread; ++u) {
      const int idx = tid + u * kBlock;
      ht[(idx / KIN) * kLdsStride + idx % KIN] = xreg[u];
    }
    __syncthreads();
    if (tile + gridDim.x < tiles) fetch_x(tile + gridDim.x);
    // Layer 1 (MFMA): acc = b1 + x W1^T, k-groups of 8 over the zero-padded d_in.
    f32x16 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][nt][r] = b1r[nt];
    __builtin_amdgcn_s_setprio(0);
    {
      // two operand sets: a group's fragments are requested while the group before it runs (the last reloads are unused)
      AFragT<2> fa[2];
      BFrag fb[2];
      auto load = [&](int set, int g) {
        load_a<2, kLdsStride>(fa[set], ht + a_off, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          fb[set].b0[e] = buffer_load_f32(w1rsrc, w1voff + e * (kWave * 4), g * (kWave * 16));
          fb[set].b1[e] = buffer_load_f32(w1rsrc, w1voff + w1tile + e * (kWave * 4), g * (kWave * 16));
        }
      };
      load(0, 0);
#pragma unroll 1
      for (int g = 0; g < kg; g += 2) {
        load(1, g + 1 < kg ? g + 1 : kg - 1);
        mma_frag<false, 2>(fa[0], fb[0], acc);
        load(0, g + 2 < kg ? g + 2 : kg - 1);
        if (g + 1 < kg) mma_frag<false, 2>(fa[1], fb[1], acc);
      }
    }
    __builtin_amdgcn_s_setprio(kValuPhasePriority);
    __syncthreads();  // every wave has read all of x: the tile takes h1
    gemm.prefetch();  // first W2 fragments, requested ahead of this tile's h1 stores
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int j = 64 * wave + 32 * nt + (lane & 31);
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = relu1(acc[mt][nt][r]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int sr = 32 * mt + (r & 3) + 8 * (r >> 2);  // + 4*hh
          ht[(sr + 4 * hh) * kLdsStride + j] = v[r];
          if constexpr (SAVE) buffer_store_f32(v[r], h1rsrc, (4 * hh * kHidden + j) * 4, sr * (kHidden * 4));
        }
      }
    __syncthreads();
    // Layer 2 (MFMA).
    gemm.run(ht, acc);
    __syncthreads();  // every wave has read all of h1: the tile may be overwritten
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int j = 64 * wave + 32 * nt + (lane & 31);
        f32x2 pre[8];
#pragma unroll
        for (int r = 0; r < 16; r += 2)
          pre[r / 2] = f32x2{acc[mt][nt][r], acc[mt][nt][r + 1]} + f32x2{b2r[nt], b2r[nt]};
        __builtin_amdgcn_sched_barrier(0);
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = relu1(pre[r / 2][r & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int sr = 32 * mt + (r & 3) + 8 * (r >> 2);  // + 4*hh
          ht[(sr + 4 * hh) * kLdsStride + j] = v[r];
          if constexpr (SAVE) buffer_store_f32(v[r], h2rsrc, (4 * hh * kHidden + j) * 4, sr * (kHidden * 4));
        }
      }
    __syncthreads();
    // Head (VALU), as in mlp_tower_forward_kernel: 4 lanes per row; lane (a, q4) of wave w owns row 4a + w and the
    // units j = q4 (mod 4); one packed fma per unit, then two lane shuffles.
    {
      const int s = 4 * (lane >> 2) + wave, q4 = lane & 3;
      outvec oacc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int q = 0; q < KOUT; ++q) oacc[c][q] = 0.0f;
      const float *row = ht + s * kLdsStride + q4;
      const outvec *wq = reinterpret_cast<const outvec *>(w3s) + q4;
#pragma unroll kHeadUnroll
      for (int jj = 0; jj < 64; ++jj) {
        const float hv = row[4 * jj];
        outvec hvv;
#pragma unroll
        for (int q = 0; q < KOUT; ++q) hvv[q] = hv;
        oacc[jj & 3] = __builtin_elementwise_fma(hvv, wq[4 * jj], oacc[jj & 3]);
      }
      const outvec o = (oacc[0] + oacc[1]) + (oacc[2] + oacc[3]);
#pragma unroll
      for (int q = 0; q < KOUT; ++q) {
        float v = o[q];
        v += __shfl_xor(v, 1, kWave);
        v += __shfl_xor(v, 2, kWave);
        if (q < n_out && q4 == 0 && s < rows) out[(r0 + s) * n_out + q] = v + b3r[q];
      }
    }
  }
}

// Data gradient over m rows:
//   dZ2 = (dOut x W3) * (h2 > 0)            VALU, thread = column, two rows per packed op
//   dH1 = dZ2 x W2                          MFMA (W2 packed transposed)
//   dZ1 = dH1 * (h1 > 0)                    accumulator epilogue
// dZ1 and dZ2 are stored ([m][256] each) for the two large products dW1 = dZ1^T x and dW2 = dZ2^T h1; dW3, db3, db2
// and db1 leave as one row of per-workgroup partials [db1 | db2 | dW3 | db3], summed by the caller in a fixed order.
template <int KOUT>
__global__ __launch_bounds__(kBlock, 2) void mlp_wide_in_backward_kernel(
    const float *__restrict__ h1, const float *__restrict__ h2, const float *__restrict__ dout, int64_t m,
    const float4 *__restrict__ w2tp, const float *__restrict__ w3, int n_out, float *__restrict__ dz1_out,
    float *__restrict__ dz2_out, float *__restrict__ partials, int partial_stride) {
  extern __shared__ float lds[];
  float *ds0 = lds;                             // [2][KOUT][64] dOut tile (output-major), zero-padded; tile parity
  float *zt = ds0 + 2 * kTileRows * kMaxOut;    // [64][257]: h2 -> dZ2
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5;

  float w3r[KOUT];  // column `tid` of W3, zero-padded
#pragma unroll
  for (int q = 0; q < KOUT; ++q) w3r[q] = q < n_out ? w3[q * kHidden + tid] : 0.0f;
  constexpr int kPairs = KOUT <= 2 ? 4 : 2;  // row pairs per block of phase 1 (one accumulator set each)
  constexpr int kSets = 4;                   // accumulator sets of phase 3
  f32x2 dw3[KOUT][kPairs], db2[kPairs];
#pragma unroll
  for (int u = 0; u < kPairs; ++u) {
    db2[u] = f32x2{0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < KOUT; ++q) dw3[q][u] = f32x2{0.0f, 0.0f};
  }
  f32x2 db1[kSets];  // columns 64*wave + 32*nt + (lane&31), this half's rows
#pragma unroll
  for (int c = 0; c < kSets; ++c) db1[c] = f32x2{0.0f, 0.0f};
  constexpr int kDoutPerThread = (kTileRows * KOUT + kBlock - 1) / kBlock;
  float db3 = 0.0f;  // output tid % KOUT, this thread's share of the rows
  TileGemm gemm(buffer_rsrc(w2tp, kHidden * kHidden * 4), wave, lane);
  __builtin_amdgcn_s_setprio(kValuPhasePriority);

  const int64_t tiles = (m + kTileRows - 1) / kTileRows;
  // As in mlp_tower_backward_kernel: the h2 tile by direct-to-LDS loads (rows past the end arrive as zeros) as soon as
  // the previous tile's matrix loop has released the LDS tile, dOut through registers at the same point, h1 in
  // accumulator layout (its sign is the ReLU mask) half ahead of phase 1 and half behind the matrix loop.
  float dreg[kDoutPerThread];
  auto request_tile = [&](int64_t tile) {
    const int64_t r0 = tile * kTileRows;
    const int rows = (int)((m - r0) < kTileRows ? (m - r0) : kTileRows);
    const __amdgpu_buffer_rsrc_t h2rsrc = buffer_rsrc(h2 + r0 * kHidden, rows * kHidden * 4);
#pragma unroll
    for (int u = 0; u < kTileRows / 4; ++u) {
      const int row = wave + 4 * u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(h2rsrc, zt + row * kLdsStride, 16, lane * 16, row * (kHidden * 4), 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kDoutPerThread; ++u) {
      const int idx = tid + u * kBlock;
      const int s = idx / KOUT, q = idx - s * KOUT;
      dreg[u] = (idx < kTileRows * KOUT && s < rows && q < n_out) ? dout[(r0 + s) * n_out + q] : 0.0f;
    }
  };
  if ((int64_t)blockIdx.x < tiles) request_tile(blockIdx.x);
  int parity = 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1) {
    const int64_t r0 = tile * kTileRows;
    const int rows = (int)((m - r0) < kTileRows ? (m - r0) : kTileRows);
    const __amdgpu_buffer_rsrc_t h1rsrc = buffer_rsrc(h1 + r0 * kHidden, rows * kHidden * 4);
    const __amdgpu_buffer_rsrc_t dz2rsrc = buffer_rsrc(dz2_out + r0 * kHidden, rows * kHidden * 4);
    const __amdgpu_buffer_rsrc_t dz1rsrc = buffer_rsrc(dz1_out + r0 * kHidden, rows * kHidden * 4);
    float *ds = ds0 + parity * kTileRows * kMaxOut;
#pragma unroll
    for (int u = 0; u < kDoutPerThread; ++u) {
      const int idx = tid + u * kBlock;
      if (idx < kTileRows * KOUT) {
        const int s = idx / KOUT, q = idx - s * KOUT;
        ds[q * kTileRows + s] = dreg[u];  // rows (s, s+1) adjacent: one 8-byte read per packed operand
        db3 += dreg[u];
      }
    }
    wait_vmcnt0();    // this wave's h2 rows have landed
    __syncthreads();  // ... everyone's have; ds is written
    float h1a[2][2][16];
    auto fetch_h1 = [&](int mt) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int sr = 32 * mt + (r & 3) + 8 * (r >> 2);
          h1a[mt][nt][r] = buffer_load_f32(h1rsrc, (4 * hh * kHidden + 64 * wave + 32 * nt + (lane & 31)) * 4,
                                           sr * (kHidden * 4));
        }
    };
    gemm.prefetch();
    fetch_h1(0);
    // Phase 1 (VALU, thread = column j, two rows per packed op): dZ2 and the head gradients.
#pragma unroll 2
    for (int s0 = 0; s0 < kTileRows; s0 += 2 * kPairs) {
      f32x2 hv[kPairs], d[KOUT][kPairs], g[kPairs];
#pragma unroll
      for (int u = 0; u < kPairs; ++u) {
        const int s = s0 + 2 * u;
        hv[u] = f32x2{zt[s * kLdsStride + tid], zt[(s + 1) * kLdsStride + tid]};
#pragma unroll
        for (int q = 0; q < KOUT; ++q) d[q][u] = *reinterpret_cast<const f32x2 *>(ds + q * kTileRows + s);
      }
#pragma unroll
      for (int u = 0; u < kPairs; ++u) g[u] = d[0][u] * f32x2{w3r[0], w3r[0]};
#pragma unroll
      for (int q = 1; q < KOUT; ++q)
#pragma unroll
        for (int u = 0; u < kPairs; ++u) g[u] = __builtin_elementwise_fma(d[q][u], f32x2{w3r[q], w3r[q]}, g[u]);
#pragma unroll
      for (int q = 0; q < KOUT; ++q)
#pragma unroll
        for (int u = 0; u < kPairs; ++u) dw3[q][u] = __builtin_elementwise_fma(d[q][u], hv[u], dw3[q][u]);
      __builtin_amdgcn_sched_barrier(0);
      f32x2 dz[kPairs];
      {
        unsigned long long gate[kPairs][2];
#pragma unroll
        for (int u = 0; u < kPairs; ++u) {
          gate[u][0] = positive_mask(hv[u].x);
          gate[u][1] = positive_mask(hv[u].y);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kPairs; ++u)
          dz[u] = f32x2{select_or_zero(gate[u][0], g[u].x), select_or_zero(gate[u][1], g[u].y)};
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kPairs; ++u) db2[u] += dz[u];
#pragma unroll
      for (int u = 0; u < kPairs; ++u) {
        const int s = s0 + 2 * u;
        zt[s * kLdsStride + tid] = dz[u].x;
        zt[(s + 1) * kLdsStride + tid] = dz[u].y;
        buffer_store_f32(dz[u].x, dz2rsrc, tid * 4, s * (kHidden * 4));
        buffer_store_f32(dz[u].y, dz2rsrc, tid * 4, (s + 1) * (kHidden * 4));
      }
    }
    __syncthreads();
    // Phase 2 (MFMA): dH1 = dZ2 x W2.
    f32x16 acc[2][2];
    gemm.run(zt, acc);
    __syncthreads();  // every wave is done with the dZ2 tile: the next h2 tile may land
    if (tile + gridDim.x < tiles) request_tile(tile + gridDim.x);
    fetch_h1(1);
    // Phase 3: dZ1 = dH1 * (h1 > 0), the two columns of a lane as one pair; db1 sums and the dZ1 stores.
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int q0 = 0; q0 < 16; q0 += kSets) {
        f32x2 dz[kSets];
        {
          unsigned long long gate[kSets][2];
#pragma unroll
          for (int u = 0; u < kSets; ++u) {
            gate[u][0] = positive_mask(h1a[mt][0][q0 + u]);
            gate[u][1] = positive_mask(h1a[mt][1][q0 + u]);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < kSets; ++u)
            dz[u] = f32x2{select_or_zero(gate[u][0], acc[mt][0][q0 + u]),
                          select_or_zero(gate[u][1], acc[mt][1][q0 + u])};
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kSets; ++u) db1[u] += dz[u];
#pragma unroll
        for (int u = 0; u < kSets; ++u) {
          const int r = q0 + u;
          const int sr = 32 * mt + (r & 3) + 8 * (r >> 2);  // + 4*hh
          const int voff = (4 * hh * kHidden + 64 * wave + (lane & 31)) * 4;
          buffer_store_f32(dz[u].x, dz1rsrc, voff, sr * (kHidden * 4));
          buffer_store_f32(dz[u].y, dz1rsrc, voff + 32 * 4, sr * (kHidden * 4));
        }
      }
  }
  // Workgroup partial row.
  float *row = partials + (int64_t)blockIdx.x * partial_stride;
  const int off_db2 = kHidden, off_dw3 = 2 * kHidden, off_db3 = off_dw3 + n_out * kHidden;
  // fold the accumulator sets (fixed order)
  f32x2 db1s = db1[0], db2s = db2[0];
#pragma unroll
  for (int c = 1; c < kSets; ++c) db1s += db1[c];
#pragma unroll
  for (int u = 1; u < kPairs; ++u) db2s += db2[u];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int i = 64 * wave + 32 * nt + (lane & 31);
    const float b = db1s[nt] + __shfl_xor(db1s[nt], 32, kWave);
    if (hh == 0) row[i] = b;
  }
  row[off_db2 + tid] = db2s.x + db2s.y;
#pragma unroll
  for (int q = 0; q < KOUT; ++q) {
    f32x2 ws = dw3[q][0];
#pragma unroll
    for (int u = 1; u < kPairs; ++u) ws += dw3[q][u];
    if (q < n_out) row[off_dw3 + q * kHidden + tid] = ws.x + ws.y;
  }
  // db3: thread t holds a share of output t % KOUT; fold through LDS.
  __syncthreads();
  ds0[tid] = db3;
  __syncthreads();
  if (tid < n_out) {
    float sum = 0.0f;
    for (int t = tid; t < kBlock; t += KOUT) sum += ds0[t];
    row[off_db3 + tid] = sum;
  }
}

// dW1[j][c] = sum_s dZ1[s][j] * x[s][c]: a [256 x M] x [M x d_in] product with the reduction over SAMPLES.  Every
// workgroup owns the whole output (8 waves x CT accumulator tiles: wave w the rows 32 w .., all CT column tiles) and a
// strided share of the 32-row tiles.  dZ1 rows go HBM -> LDS by direct-to-LDS loads (one 1-KiB row per instruction), x
// rows (d_in floats: no alignment to build on) through registers; both double-buffered, so the next tile lands during
// the matrix loop of the current one.  The partial sum is left in a workspace slab that a second kernel adds up in slab
// order (bitwise reproducible; no atomics).
constexpr int kWgradThreads = 512;
constexpr int kWgradRows = 32;      // rows per staged tile
// Row strides of 16 n floats, and the rows with bit 2 set -- the rows the upper half-wave reads -- shifted by 32
// floats: the two half-waves of an operand read fall on disjoint banks.
constexpr int kWgradZStride = 320;
constexpr int kWgradZTile = kWgradRows * kWgradZStride;
template <int CT>
struct WgradGeo {
  static constexpr int KX = 32 * CT;             // columns of the x tile
  static constexpr int XS = KX + 32;             // its row stride
  static constexpr int kXTile = kWgradRows * XS;
  static constexpr int kBuffer = kWgradZTile + kXTile;  // floats per buffer
  static constexpr size_t kLdsBytes = sizeof(float) * 2 * kBuffer;
};

template <int CT>
__global__ __launch_bounds__(kWgradThreads, 1) void mlp_wide_in_wgrad_kernel(
    const float *__restrict__ dz1, const float *__restrict__ x, int64_t m, int d_in, float *__restrict__ slabs) {
  using G = WgradGeo<CT>;
  extern __shared__ float lds[];  // [2 buffers][dZ1 tile | x tile]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jl = lane & 31, kh = lane >> 5;
  f32x16 acc[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

  const int64_t tiles = (m + kWgradRows - 1) / kWgradRows;
  constexpr int kXPerThread = kWgradRows * G::KX / kWgradThreads;  // 2 CT
  float xreg[kXPerThread];
  // Wave w fetches rows w, w+8, w+16, w+24 of dZ1; rows past the end of the data are out of range of the descriptor
  // and arrive as zeros, as do the rows and columns of x past m and d_in.
  auto fetch = [&](int64_t tile, int buffer) {
    const int64_t r0 = tile * kWgradRows;
    const int rows = (int)((m - r0) < kWgradRows ? (m - r0) : kWgradRows);
    const __amdgpu_buffer_rsrc_t zr = buffer_rsrc(dz1 + r0 * kHidden, rows * kHidden * 4);
    float *zb = lds + buffer * G::kBuffer;
#pragma unroll
    for (int u = 0; u < kWgradRows / 8; ++u) {
      const int row = wave + 8 * u;  // bit 2 of the row = bit 2 of the wave
      const int off = row * kWgradZStride + ((wave & 4) ? 32 : 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(zr, zb + off, 16, lane * 16, row * (kHidden * 4), 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kXPerThread; ++u) {
      const int idx = tid + u * kWgradThreads, s = idx / G::KX, c = idx % G::KX;
      xreg[u] = (c < d_in && r0 + s < m) ? x[(r0 + s) * d_in + c] : 0.0f;
    }
  };
  auto stage_x = [&](int buffer) {
    float *xb = lds + buffer * G::kBuffer + kWgradZTile;
#pragma unroll
    for (int u = 0; u < kXPerThread; ++u) {
      const int idx = tid + u * kWgradThreads, s = idx / G::KX, c = idx % G::KX;
      xb[s * G::XS + ((s & 4) ? 32 : 0) + c] = xreg[u];
    }
  };
  // One barrier per tile: behind it this tile's operands are in LDS (the x rows written just above it, the dZ1 rows
  // landed) and every wave is done with the other buffer, which the next tile then streams into.
  const int64_t t0 = blockIdx.x, stride = gridDim.x;
  if (t0 < tiles) fetch(t0, 0);
  int buffer = 0;
  for (int64_t tile = t0; tile < tiles; tile += stride, buffer ^= 1) {
    stage_x(buffer);
    wait_vmcnt0();
    __syncthreads();
    if (tile + stride < tiles) fetch(tile + stride, buffer ^ 1);
    // this lane's rows of k-group g are 8g + 4 kh + e: bit 2 of the row is kh
    const float *za = lds + buffer * G::kBuffer + kh * (4 * kWgradZStride + 32) + 32 * wave + jl;
    const float *xa = lds + buffer * G::kBuffer + kWgradZTile + kh * (4 * G::XS + 32) + jl;
#pragma unroll
    for (int g = 0; g < kWgradRows / 8; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = za[(8 * g + e) * kWgradZStride];
#pragma unroll
        for (int t = 0; t < CT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xa[(8 * g + e) * G::XS + 32 * t], acc[t], 0, 0, 0);
      }
  }
  // Partial slab of this workgroup: slab[j][c], the gradient's own layout.
  float *slab = slabs + (int64_t)blockIdx.x * kHidden * d_in;
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * kh;
      const int c = 32 * t + jl;
      if (c < d_in) slab[j * d_in + c] = acc[t][r];
    }
}

// out[idx] (+)= sum over slabs, in slab order.
__global__ __launch_bounds__(kBlock) void mlp_wide_in_wgrad_reduce_kernel(const float *__restrict__ slabs, int rows, int n,
                                                                          float *__restrict__ out, int accumulate) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n) return;
  float sum = accumulate ? out[idx] : 0.0f;
  for (int r = 0; r < rows; ++r) sum += slabs[(int64_t)r * n + idx];
  out[idx] = sum;
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// d_in rounded up to the fetch width of a forward variant; n_out to the width of a head variant.
using InWidths = Widths<32, 64, 128>;
using OutWidths = Widths<2, 4, 8>;
inline int in_class(int d_in) { return d_in <= 32 ? 32 : d_in <= 64 ? 64 : 128; }

template <int KIN, int KOUT, bool SAVE>
static int launch_forward(int grid, hipStream_t s, const float *x, int64_t m, int d_in, const float *w1p, const float *b1,
                          const float4 *w2p, const float *b2, const float *w3, const float *b3, int n_out, float *out,
                          float *save_h1, float *save_h2) {
  if (const int e = allow_dynamic_lds<&mlp_wide_in_forward_kernel<KIN, KOUT, SAVE>>()) return e;
  mlp_wide_in_forward_kernel<KIN, KOUT, SAVE><<<grid, kBlock, forward_lds_bytes(), s>>>(
      x, m, d_in, w1p, b1, w2p, b2, w3, b3, n_out, out, save_h1, save_h2);
  return launch_status();
}

template <int KOUT>
static int launch_backward(int grid, hipStream_t s, const float *h1, const float *h2, const float *dout, int64_t m,
                           const float4 *w2tp, const float *w3, int n_out, float *dz1, float *dz2, float *partials,
                           int stride) {
  if (const int e = allow_dynamic_lds<&mlp_wide_in_backward_kernel<KOUT>>()) return e;
  mlp_wide_in_backward_kernel<KOUT><<<grid, kBlock, backward_lds_bytes(), s>>>(h1, h2, dout, m, w2tp, w3, n_out, dz1, dz2,
                                                                              partials, stride);
  return launch_status();
}

template <int CT>
static int launch_wgrad(int grid, hipStream_t s, const float *dz1, const float *x, int64_t m, int d_in, float *slabs) {
  if (const int e = allow_dynamic_lds<&mlp_wide_in_wgrad_kernel<CT>>()) return e;
  mlp_wide_in_wgrad_kernel<CT><<<grid, kWgradThreads, WgradGeo<CT>::kLdsBytes, s>>>(dz1, x, m, d_in, slabs);
  return launch_status();
}

}  // namespace wide_in
}  // namespace rl8

using namespace rl8;
using namespace rl8::wide_in;

RL8_API int rl8_mlp_wide_in_supports(int d_in, int n_out) { return supports(d_in, n_out) ? 1 : 0; }

// Dynamic LDS of a launch: kernel 0 the forward (either variant), 1 the data gradient, 2 the weight gradient at d_in.
RL8_API int64_t rl8_mlp_wide_in_lds_bytes(int kernel, int d_in) {
  if (kernel < 0 || kernel > 2 || d_in < kMinIn || d_in > kMaxWideIn) return RL8_ESIZE;
  if (kernel == 0) return (int64_t)forward_lds_bytes();
  if (kernel == 1) return (int64_t)backward_lds_bytes();
  const int ct = (d_in + 31) / 32;
  return (int64_t)sizeof(float) * 2 * (kWgradZTile + kWgradRows * (32 * ct + 32));
}

RL8_API int64_t rl8_mlp_wide_in_pack_floats(int d_in) {
  if (d_in < kMinIn || d_in > kMaxWideIn) return RL8_ESIZE;
  return (int64_t)kHidden * 8 * k_groups(d_in);
}

RL8_API int rl8_mlp_wide_in_pack_w1_f32(const float *w1, int d_in, float *w1_packed, void *stream) {
  if (!w1 || !w1_packed) return RL8_ENULL;
  if (d_in < kMinIn || d_in > kMaxWideIn) return RL8_ESIZE;
  if (!aligned4(w1) || !aligned16(w1_packed)) return RL8_EALIGN;
  const int kg = k_groups(d_in);
  mlp_wide_in_pack_w1_kernel<<<kHidden * 8 * kg / kBlock, kBlock, 0, (hipStream_t)stream>>>(w1, d_in, kg, w1_packed);
  return launch_status();
}

RL8_API int rl8_mlp_wide_in_forward_f32(const float *x, int64_t m, int d_in, const float *w1_packed, const float *b1,
                                        const float *w2_packed, const float *b2, const float *w3, const float *b3,
                                        int n_out, float *out, float *save_h1, float *save_h2, void *stream) {
  if (!x || !w1_packed || !b1 || !w2_packed || !b2 || !w3 || !b3 || !out) return RL8_ENULL;
  if ((save_h1 == nullptr) != (save_h2 == nullptr)) return RL8_ENULL;
  if (m < 1 || !supports(d_in, n_out)) return RL8_ESIZE;
  if (!aligned16(w1_packed) || !aligned16(w2_packed) || (save_h1 && (!aligned16(save_h1) || !aligned16(save_h2))))
    return RL8_EALIGN;
  if (!aligned4(x) || !aligned4(b1) || !aligned4(b2) || !aligned4(w3) || !aligned4(b3) || !aligned4(out)) return RL8_EALIGN;
  const int grid = tower_grid(m, kTileRows);
  const float4 *w2p = reinterpret_cast<const float4 *>(w2_packed);
  hipStream_t s = (hipStream_t)stream;
  return variant_status(dispatch_width(in_class(d_in), InWidths{}, [&](auto d) {
    return dispatch_width(pad_out(n_out < 2 ? 2 : n_out), OutWidths{}, [&](auto n) {
      return save_h1 ? launch_forward<d(), n(), true>(grid, s, x, m, d_in, w1_packed, b1, w2p, b2, w3, b3, n_out, out, save_h1, save_h2)
                     : launch_forward<d(), n(), false>(grid, s, x, m, d_in, w1_packed, b1, w2p, b2, w3, b3, n_out, out, save_h1, save_h2);
    });
  }));
}

RL8_API int64_t rl8_mlp_wide_in_partial_floats(int n_out) {
  if (n_out < 1 || n_out > kMaxOut) return RL8_ESIZE;
  return 2 * kHidden + (int64_t)n_out * kHidden + n_out;
}

RL8_API int rl8_mlp_wide_in_max_rows(void) { return 2 * kCUs; }

RL8_API int rl8_mlp_wide_in_backward_f32(const float *h1, const float *h2, const float *dout, int64_t m,
                                         const float *w2t_packed, const float *w3, int n_out, float *dz1_out,
                                         float *dz2_out, float *partials, int *partial_rows_out, void *stream) {
  if (!h1 || !h2 || !dout || !w2t_packed || !w3 || !dz1_out || !dz2_out || !partials || !partial_rows_out) return RL8_ENULL;
  if (m < 1 || n_out < 1 || n_out > kMaxOut) return RL8_ESIZE;
  if (!aligned16(h1) || !aligned16(h2) || !aligned16(dz1_out) || !aligned16(dz2_out) || !aligned16(w2t_packed))
    return RL8_EALIGN;
  if (!aligned4(dout) || !aligned4(w3) || !aligned4(partials)) return RL8_EALIGN;
  const int grid = grid_for(m, kTileRows, 2 * kCUs);  // (rl8_mlp_wide_in_max_rows() partial rows: a function of m alone)
  *partial_rows_out = grid;
  const float4 *w2tp = reinterpret_cast<const float4 *>(w2t_packed);
  const int stride = (int)rl8_mlp_wide_in_partial_floats(n_out);
  hipStream_t s = (hipStream_t)stream;
  return variant_status(dispatch_width(pad_out(n_out < 2 ? 2 : n_out), OutWidths{}, [&](auto n) {
    return launch_backward<n()>(grid, s, h1, h2, dout, m, w2tp, w3, n_out, dz1_out, dz2_out, partials, stride);
  }));
}

RL8_API int64_t rl8_mlp_wide_in_workspace_bytes(int d_in) {
  if (d_in < kMinIn || d_in > kMaxWideIn) return RL8_ESIZE;
  return (int64_t)kCUs * kHidden * d_in * (int64_t)sizeof(float);  // one [256][d_in] slab per CU
}

RL8_API int rl8_mlp_wide_in_wgrad_f32(const float *dz1, const float *x, int64_t m, int d_in, float *workspace,
                                      float *dw1_out, int accumulate, void *stream) {
  if (!dz1 || !x || !workspace || !dw1_out) return RL8_ENULL;
  if (m < 1 || d_in < kMinIn || d_in > kMaxWideIn) return RL8_ESIZE;
  if (!aligned16(dz1) || !aligned4(x) || !aligned4(workspace) || !aligned4(dw1_out)) return RL8_EALIGN;
  const int grid = grid_for(m, kWgradRows, kCUs);
  hipStream_t s = (hipStream_t)stream;
  const int st = variant_status(dispatch_width((d_in + 31) / 32, Widths<1, 2, 3, 4>{}, [&](auto ct) {
    return launch_wgrad<ct()>(grid, s, dz1, x, m, d_in, workspace);
  }));
  if (st != RL8_OK) return st;
  const int n = kHidden * d_in;
  mlp_wide_in_wgrad_reduce_kernel<<<(n + kBlock - 1) / kBlock, kBlock, 0, s>>>(workspace, grid, n, dw1_out, accumulate);
  return launch_status();
}
