// N1, "wide head" family: Linear(d_in, 256) ReLU Linear(256, 256) ReLU Linear(256, n_out) with biased layers,
// 1 <= d_in <= 128, 9 <= n_out <= 128 (summed over a tower's heads), in fp32 throughout on v_mfma_f32_32x32x2_f32 (exact
// fp32 fma chains).  Every other tower family forms the head as a VALU dot per row with n_out accumulators per thread:
// past 8 outputs that neither fits nor pays.  Here the head, and its gradients, are matrix products as well.  The family
// grows out of mlp_wide_in_kernels.hip: the same [64][257] LDS tile, the same layer-1 k-loop from a fragment-ordered W1
// pack (for any d_in >= 1, zero-padded to the k-granule of 8), the same TileGemm over rl8_mlp_pack_w2_f32's packing.
//
// Forward (one launch): a workgroup (4 waves) walks 64-row tiles: x -> tile, layer 1, h1 -> tile, layer 2, h2 -> tile,
// then  out[64][n_out] = h2 W3^T + b3  with the A operand read from the h2 tile and the B operand from a
// fragment-ordered, zero-padded W3 pack (n_out padded to 32-column tiles, 32 k-groups of 8 over the 256 units) through
// L2, as the W1 fragments are: at most 128 KiB, no LDS.  The 2 x ceil(n_out / 32) output blocks of 32 x 32 go round the
// four waves.  The training variant stores h1 and h2; the rollout variant stores neither and computes the same bits.
//
// Data gradient (one launch per row segment): the dOut tile goes into the LDS tile whole, zero-padded to the k-granule,
// as x does in the forward;  dH2 = dOut W3  is a k-loop over ceil(n_out / 8) groups from a second W3 pack (transposed);
// dZ2 = dH2 . [h2 > 0]  is the accumulator epilogue (h2 fetched in accumulator layout) and takes the tile;
// dZ1 = (dZ2 W2) . [h1 > 0]  as in mlp_wide_in_backward_kernel.  dZ1 and dZ2 are stored [rows][256]; one partial row
// per workgroup [db1 (256) | db2 (256) | db3 (n_out)].  No dW3 here (n_out x 256 running sums do not fit a thread): it is
// a product over the rows like dW1.  ReLU'(0) = 0.
//
// Weight gradients over the rows: C [256][c] (+)= A^T B with A [m][256], B [m][c], 1 <= c <= 128: the structure of
// mlp_wide_in_wgrad_kernel (8 waves, 32-row tiles, double-buffered, one slab per workgroup, slabs summed in slab order,
// grid a function of m alone).  dW1 = dZ1^T x (c = d_in) and dW3^T = h2^T dOut (c = n_out; the slab reduction
// writes the transpose).  dW2 stays with rl8_mlp_wgrad_*.
//
// LDS (dynamic) and workgroups per CU (160 KiB):
//   forward, both variants : tile [64][257]                                   = 65 792 B, 2 per CU
//   data gradient          : tile [64][257]                                   = 65 792 B, 2 per CU
//   weight gradient        : 2 x (A [32][320] + B [32][32 CT + 32]), CT = ceil(c / 32) column tiles
//                            = 98 304 / 106 496 / 114 688 / 122 880 B for CT = 1..4, 1 per CU (8 waves)
#include "mfma_tile.hip.h"
#include "tower_launch.hip.h"

namespace rl8 {
namespace wide_out {

constexpr int kMinHead = kMaxOut + 1;  // the VALU heads end at kMaxOut
constexpr int kMaxHead = 128;
constexpr int kMaxWideIn = 128;

inline bool supports(int d_in, int n_out) {
  return d_in >= 1 && d_in <= kMaxWideIn && n_out >= kMinHead && n_out <= kMaxHead;
}
__host__ __device__ constexpr int k_groups(int k) { return (k + 7) / 8; }
__host__ __device__ constexpr int col_tiles(int n) { return (n + 31) / 32; }

// The B operand of a product, B[k][r], in fragment order with kg k-groups per 32-column tile, zeros outside w:
//   packed[((n*kg + g)*4 + e)*64 + l] = B[8g + 4(l>>5) + e][32n + (l&31)]
// B[k][r] = w[r][k] (w [rows_w][cols_w] row-major: a torch Linear weight as the forward uses it), or, `transposed`,
// B[k][r] = w[k][r] (the same weight as the data gradient uses it).
__global__ __launch_bounds__(kBlock) void mlp_wide_out_pack_kernel(const float *__restrict__ w, int rows_w, int cols_w,
                                                                   int transposed, int kg, int total,
                                                                   float *__restrict__ packed) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int l = idx & 63, e = (idx >> 6) & 3, ng = idx >> 8, g = ng % kg, n = ng / kg;
  const int r = 32 * n + (l & 31), k = 8 * g + 4 * (l >> 5) + e;
  float v = 0.0f;
  if (transposed) {
    if (k < rows_w && r < cols_w) v = w[k * cols_w + r];
  } else {
    if (r < rows_w && k < cols_w) v = w[r * cols_w + k];
  }
  packed[idx] = v;
}

constexpr size_t tile_lds_bytes() { return sizeof(float) * kTileRows * kLdsStride; }

// KIN: d_in rounded up to 32, 64 or 128 (how many floats of a row a thread block fetches; the k-loop itself runs
// ceil(d_in / 8) groups).  SAVE: also store h1 / h2 ([m][256] each).  The head's width is a run-time value: it only
// bounds loops over whole 32 x 32 output blocks.
template <int KIN, bool SAVE>
__global__ __launch_bounds__(kBlock, 2) void mlp_wide_out_forward_kernel(
    const float *__restrict__ x, int64_t m, int d_in, const float *__restrict__ w1p, const float *__restrict__ b1,
    const float4 *__restrict__ w2p, const float *__restrict__ b2, const float *__restrict__ w3p,
    const float *__restrict__ b3, int n_out, float *__restrict__ out, float *__restrict__ save_h1,
    float *__restrict__ save_h2) {
  extern __shared__ float lds[];
  float *ht = lds;  // [64][257]: x (columns < 8 kg), then h1, then h2
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5;
  const int kg = k_groups(d_in);
  const int blocks = 2 * col_tiles(n_out);  // 32 x 32 blocks of the head's output tile

  float b1r[2], b2r[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    b1r[nt] = b1[64 * wave + 32 * nt + (lane & 31)];
    b2r[nt] = b2[64 * wave + 32 * nt + (lane & 31)];
  }
  TileGemm gemm(buffer_rsrc(w2p, kHidden * kHidden * 4), wave, lane);
  // W1 fragments: the wave's two column tiles 2 wave + nt, k-group g at g * 1 KiB (a uniform offset)
  const __amdgpu_buffer_rsrc_t w1rsrc = buffer_rsrc(w1p, kHidden * 8 * kg * 4);
  const int w1voff = (2 * wave) * kg * (kWave * 16) + lane * 4, w1tile = kg * (kWave * 16);
  // W3 fragments: column tile ct at ct * 32 KiB
  const __amdgpu_buffer_rsrc_t w3rsrc = buffer_rsrc(w3p, col_tiles(n_out) * 32 * kHidden * 4);
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
    __syncthreads();  // the previous tile's head has read h2
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
    // Head (MFMA): block b = (column tile b / 2, row tile b % 2) of out = b3 + h2 W3^T goes to wave b mod 4; the 32
    // k-groups over the units with two operand sets, as layer 1.
    __builtin_amdgcn_s_setprio(0);
#pragma unroll 1
    for (int block = wave; block < blocks; block += kWavesPerBlock) {
      const int mt = block & 1, ct = block >> 1;
      const int col = 32 * ct + (lane & 31);
      const float bias = col < n_out ? b3[col] : 0.0f;
      f32x16 o;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = bias;
      const float *ap = ht + 32 * mt * kLdsStride + a_off;
      const int w3voff = ct * (kGroups * kWave * 16) + lane * 4;
      float fa[2][4], fb[2][4];
      auto load = [&](int set, int g) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          fa[set][e] = ap[8 * g + e];
          fb[set][e] = buffer_load_f32(w3rsrc, w3voff + e * (kWave * 4), g * (kWave * 16));
        }
      };
      auto mma = [&](int set) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][e], fb[set][e], o, 0, 0, 0);
      };
      load(0, 0);
#pragma unroll 1
      for (int g = 0; g < kGroups; g += 2) {
        load(1, g + 1);
        mma(0);
        load(0, g + 2 < kGroups ? g + 2 : kGroups - 1);
        mma(1);
      }
      if (col < n_out) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int s = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh;
          if (s < rows) out[(r0 + s) * n_out + col] = o[r];
        }
      }
    }
    __builtin_amdgcn_s_setprio(kValuPhasePriority);
  }
}

// Data gradient over m rows:
//   dH2 = dOut x W3                         MFMA, k over the zero-padded n_out (W3 packed transposed)
//   dZ2 = dH2 * (h2 > 0)                    accumulator epilogue
//   dH1 = dZ2 x W2                          MFMA (W2 packed transposed)
//   dZ1 = dH1 * (h1 > 0)                    accumulator epilogue
// dZ1 and dZ2 are stored ([m][256] each) for dW1 = dZ1^T x and dW2 = dZ2^T h1; db3, db2 and db1 leave as one row of
// per-workgroup partials [db1 | db2 | db3], summed by the caller in a fixed order.
// KOUT: n_out rounded up to 32, 64 or 128 (how many floats of a dOut row a thread block fetches).
template <int KOUT>
__global__ __launch_bounds__(kBlock, 2) void mlp_wide_out_backward_kernel(
    const float *__restrict__ h1, const float *__restrict__ h2, const float *__restrict__ dout, int64_t m,
    const float4 *__restrict__ w2tp, const float *__restrict__ w3tp, int n_out, float *__restrict__ dz1_out,
    float *__restrict__ dz2_out, float *__restrict__ partials, int partial_stride) {
  extern __shared__ float lds[];
  float *zt = lds;  // [64][257]: dOut (columns < 8 kg), then dZ2
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5;
  const int kg = k_groups(n_out);

  constexpr int kSets = 4;  // accumulator sets of the two epilogues
  f32x2 db1[kSets], db2[kSets];  // columns 64*wave + 32*nt + (lane&31), this half's rows
#pragma unroll
  for (int c = 0; c < kSets; ++c) db1[c] = db2[c] = f32x2{0.0f, 0.0f};
  float db3 = 0.0f;  // output tid (tid < n_out)
  TileGemm gemm(buffer_rsrc(w2tp, kHidden * kHidden * 4), wave, lane);
  const __amdgpu_buffer_rsrc_t w3rsrc = buffer_rsrc(w3tp, kHidden * 8 * kg * 4);
  const int w3voff = (2 * wave) * kg * (kWave * 16) + lane * 4, w3tile = kg * (kWave * 16);
  const int a_off = (lane & 31) * kLdsStride + 4 * hh;
  __builtin_amdgcn_s_setprio(kValuPhasePriority);

  const int64_t tiles = (m + kTileRows - 1) / kTileRows;
  // dOut tile: element (row idx / KOUT, column idx % KOUT) is owned by thread idx (+256, ...): one column and every
  // (256 / KOUT)-th row per thread, so one lane offset and uniform row offsets behind a descriptor sized to the tile's
  // valid rows.  Rows past m are out of its range and arrive as zeros; so do the columns past n_out, whose lane offset
  // is out of every range.
  constexpr int kDPerThread = kTileRows * KOUT / kBlock, kDRowStep = kBlock / KOUT;
  float dreg[kDPerThread];
  const int dvoff = tid % KOUT < n_out ? ((tid / KOUT) * n_out + tid % KOUT) * 4 : 0x40000000;
  auto fetch_d = [&](int64_t tile) {
    const int64_t r0 = tile * kTileRows;
    const int rows = (int)((m - r0) < kTileRows ? (m - r0) : kTileRows);
    const __amdgpu_buffer_rsrc_t drsrc = buffer_rsrc(dout + r0 * n_out, rows * n_out * 4);
#pragma unroll
    for (int u = 0; u < kDPerThread; ++u) dreg[u] = buffer_load_f32(drsrc, dvoff, u * kDRowStep * n_out * 4);
  };
  if ((int64_t)blockIdx.x < tiles) fetch_d(blockIdx.x);

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kTileRows;
    const int rows = (int)((m - r0) < kTileRows ? (m - r0) : kTileRows);
    const __amdgpu_buffer_rsrc_t h1rsrc = buffer_rsrc(h1 + r0 * kHidden, rows * kHidden * 4);
    const __amdgpu_buffer_rsrc_t h2rsrc = buffer_rsrc(h2 + r0 * kHidden, rows * kHidden * 4);
    const __amdgpu_buffer_rsrc_t dz2rsrc = buffer_rsrc(dz2_out + r0 * kHidden, rows * kHidden * 4);
    const __amdgpu_buffer_rsrc_t dz1rsrc = buffer_rsrc(dz1_out + r0 * kHidden, rows * kHidden * 4);
    // (the previous tile's matrix loop ended behind a barrier: the tile is free)
#pragma unroll
    for (int u = 0; u < kDPerThread; ++u) {
      const int idx = tid + u * kBlock;
      zt[(idx / KOUT) * kLdsStride + idx % KOUT] = dreg[u];
    }
    __syncthreads();
    // h1 / h2 in accumulator layout (their signs are the ReLU masks), requested right ahead of the epilogue that
    // reads them.  Rows past the end arrive as zeros.
    float ha[2][2][16];
    auto fetch_h = [&](__amdgpu_buffer_rsrc_t rsrc, int mt) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int sr = 32 * mt + (r & 3) + 8 * (r >> 2);
          ha[mt][nt][r] = buffer_load_f32(rsrc, (4 * hh * kHidden + 64 * wave + 32 * nt + (lane & 31)) * 4,
                                          sr * (kHidden * 4));
        }
    };
    // db3: the column sums of the dOut tile (rows past m are zeros), rows in order.
    if (tid < n_out) {
#pragma unroll 8
      for (int s = 0; s < kTileRows; ++s) db3 += zt[s * kLdsStride + tid];
    }
    // Phase 1 (MFMA): dH2 = dOut x W3, k-groups of 8 over the zero-padded n_out.
    f32x16 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.0f;
    __builtin_amdgcn_s_setprio(0);
    {
      AFragT<2> fa[2];
      BFrag fb[2];
      auto load = [&](int set, int g) {
        load_a<2, kLdsStride>(fa[set], zt + a_off, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          fb[set].b0[e] = buffer_load_f32(w3rsrc, w3voff + e * (kWave * 4), g * (kWave * 16));
          fb[set].b1[e] = buffer_load_f32(w3rsrc, w3voff + w3tile + e * (kWave * 4), g * (kWave * 16));
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
    __syncthreads();  // every wave has read all of dOut: the tile takes dZ2
    gemm.prefetch();  // first W2^T fragments, requested ahead of this tile's dZ2 stores
    fetch_h(h2rsrc, 0);
    fetch_h(h2rsrc, 1);
    // Phase 2: dZ2 = dH2 * (h2 > 0), the two columns of a lane as one pair; db2 sums, the tile and the dZ2 stores.
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int q0 = 0; q0 < 16; q0 += kSets) {
        f32x2 dz[kSets];
        {
          unsigned long long gate[kSets][2];
#pragma unroll
          for (int u = 0; u < kSets; ++u) {
            gate[u][0] = positive_mask(ha[mt][0][q0 + u]);
            gate[u][1] = positive_mask(ha[mt][1][q0 + u]);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < kSets; ++u)
            dz[u] = f32x2{select_or_zero(gate[u][0], acc[mt][0][q0 + u]), select_or_zero(gate[u][1], acc[mt][1][q0 + u])};
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kSets; ++u) db2[u] += dz[u];
#pragma unroll
        for (int u = 0; u < kSets; ++u) {
          const int r = q0 + u;
          const int sr = 32 * mt + (r & 3) + 8 * (r >> 2);  // + 4*hh
          const int j = 64 * wave + (lane & 31);
          zt[(sr + 4 * hh) * kLdsStride + j] = dz[u].x;
          zt[(sr + 4 * hh) * kLdsStride + j + 32] = dz[u].y;
          const int voff = (4 * hh * kHidden + j) * 4;
          buffer_store_f32(dz[u].x, dz2rsrc, voff, sr * (kHidden * 4));
          buffer_store_f32(dz[u].y, dz2rsrc, voff + 32 * 4, sr * (kHidden * 4));
        }
      }
    __syncthreads();
    // Phase 3 (MFMA): dH1 = dZ2 x W2.
    gemm.run(zt, acc);
    __syncthreads();  // every wave is done with the dZ2 tile: the next dOut tile may be written
    // (h1 is requested here, not ahead of the matrix loop: a half of it beside the loop's operand sets spills)
    fetch_h(h1rsrc, 0);
    fetch_h(h1rsrc, 1);
    // Phase 4: dZ1 = dH1 * (h1 > 0); db1 sums and the dZ1 stores.
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int q0 = 0; q0 < 16; q0 += kSets) {
        f32x2 dz[kSets];
        {
          unsigned long long gate[kSets][2];
#pragma unroll
          for (int u = 0; u < kSets; ++u) {
            gate[u][0] = positive_mask(ha[mt][0][q0 + u]);
            gate[u][1] = positive_mask(ha[mt][1][q0 + u]);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < kSets; ++u)
            dz[u] = f32x2{select_or_zero(gate[u][0], acc[mt][0][q0 + u]), select_or_zero(gate[u][1], acc[mt][1][q0 + u])};
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
    // (requested here and not ahead of phase 4: beside both halves of h1 and the accumulators, 32 more registers at
    // 128 outputs do not fit two workgroups per CU; the other workgroup's matrix loop covers the wait)
    if (tile + gridDim.x < tiles) fetch_d(tile + gridDim.x);
  }
  // Workgroup partial row; the accumulator sets fold in a fixed order.
  float *row = partials + (int64_t)blockIdx.x * partial_stride;
  f32x2 db1s = db1[0], db2s = db2[0];
#pragma unroll
  for (int c = 1; c < kSets; ++c) {
    db1s += db1[c];
    db2s += db2[c];
  }
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int i = 64 * wave + 32 * nt + (lane & 31);
    const float u = db1s[nt] + __shfl_xor(db1s[nt], 32, kWave);
    const float v = db2s[nt] + __shfl_xor(db2s[nt], 32, kWave);
    if (hh == 0) {
      row[i] = u;
      row[kHidden + i] = v;
    }
  }
  if (tid < n_out) row[2 * kHidden + tid] = db3;
}

// C[j][q] = sum_s A[s][j] * B[s][q]: a [256 x M] x [M x c] product with the reduction over SAMPLES.  Every workgroup
// owns the whole output (8 waves x CT accumulator tiles: wave w the rows 32 w .., all CT column tiles) and a strided
// share of the 32-row tiles.  A rows go HBM -> LDS by direct-to-LDS loads (one 1-KiB row per instruction), B rows (c
// floats: no alignment to build on) through registers; both double-buffered, so the next tile lands during the matrix
// loop of the current one.  The partial sum is left in a workspace slab that a second kernel adds up in slab order
// (bitwise reproducible; no atomics).
constexpr int kWgradThreads = 512;
constexpr int kWgradRows = 32;      // rows per staged tile
// Row strides of 16 n floats, and the rows with bit 2 set -- the rows the upper half-wave reads -- shifted by 32
// floats: the two half-waves of an operand read fall on disjoint banks.
constexpr int kWgradAStride = 320;
constexpr int kWgradATile = kWgradRows * kWgradAStride;
template <int CT>
struct WgradGeo {
  static constexpr int KB = 32 * CT;             // columns of the B tile
  static constexpr int BS = KB + 32;             // its row stride
  static constexpr int kBTile = kWgradRows * BS;
  static constexpr int kBuffer = kWgradATile + kBTile;  // floats per buffer
  static constexpr size_t kLdsBytes = sizeof(float) * 2 * kBuffer;
};

template <int CT>
__global__ __launch_bounds__(kWgradThreads, 1) void mlp_wide_out_wgrad_kernel(
    const float *__restrict__ a, const float *__restrict__ b, int64_t m, int c, float *__restrict__ slabs) {
  using G = WgradGeo<CT>;
  extern __shared__ float lds[];  // [2 buffers][A tile | B tile]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jl = lane & 31, kh = lane >> 5;
  f32x16 acc[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

  const int64_t tiles = (m + kWgradRows - 1) / kWgradRows;
  constexpr int kBPerThread = kWgradRows * G::KB / kWgradThreads;  // 2 CT
  float breg[kBPerThread];
  // Wave w fetches rows w, w+8, w+16, w+24 of A; rows past the end of the data are out of range of the descriptor
  // and arrive as zeros, as do the rows and columns of B past m and c.
  auto fetch = [&](int64_t tile, int buffer) {
    const int64_t r0 = tile * kWgradRows;
    const int rows = (int)((m - r0) < kWgradRows ? (m - r0) : kWgradRows);
    const __amdgpu_buffer_rsrc_t ar = buffer_rsrc(a + r0 * kHidden, rows * kHidden * 4);
    float *ab = lds + buffer * G::kBuffer;
#pragma unroll
    for (int u = 0; u < kWgradRows / 8; ++u) {
      const int row = wave + 8 * u;  // bit 2 of the row = bit 2 of the wave
      const int off = row * kWgradAStride + ((wave & 4) ? 32 : 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ar, ab + off, 16, lane * 16, row * (kHidden * 4), 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kBPerThread; ++u) {
      const int idx = tid + u * kWgradThreads, s = idx / G::KB, q = idx % G::KB;
      breg[u] = (q < c && r0 + s < m) ? b[(r0 + s) * c + q] : 0.0f;
    }
  };
  auto stage_b = [&](int buffer) {
    float *bb = lds + buffer * G::kBuffer + kWgradATile;
#pragma unroll
    for (int u = 0; u < kBPerThread; ++u) {
      const int idx = tid + u * kWgradThreads, s = idx / G::KB, q = idx % G::KB;
      bb[s * G::BS + ((s & 4) ? 32 : 0) + q] = breg[u];
    }
  };
  // One barrier per tile: behind it this tile's operands are in LDS (the B rows written just above it, the A rows
  // landed) and every wave is done with the other buffer, which the next tile then streams into.
  const int64_t t0 = blockIdx.x, stride = gridDim.x;
  if (t0 < tiles) fetch(t0, 0);
  int buffer = 0;
  for (int64_t tile = t0; tile < tiles; tile += stride, buffer ^= 1) {
    stage_b(buffer);
    wait_vmcnt0();
    __syncthreads();
    if (tile + stride < tiles) fetch(tile + stride, buffer ^ 1);
    // this lane's rows of k-group g are 8g + 4 kh + e: bit 2 of the row is kh
    const float *aa = lds + buffer * G::kBuffer + kh * (4 * kWgradAStride + 32) + 32 * wave + jl;
    const float *ba = lds + buffer * G::kBuffer + kWgradATile + kh * (4 * G::BS + 32) + jl;
#pragma unroll
    for (int g = 0; g < kWgradRows / 8; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float av = aa[(8 * g + e) * kWgradAStride];
#pragma unroll
        for (int t = 0; t < CT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ba[(8 * g + e) * G::BS + 32 * t], acc[t], 0, 0, 0);
      }
  }
  // Partial slab of this workgroup: slab[j][q].
  float *slab = slabs + (int64_t)blockIdx.x * kHidden * c;
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * kh;
      const int q = 32 * t + jl;
      if (q < c) slab[j * c + q] = acc[t][r];
    }
}

// out (+)= the sum over the slabs ([256][c] each), in slab order; `transpose`: out is [c][256].
__global__ __launch_bounds__(kBlock) void mlp_wide_out_wgrad_reduce_kernel(const float *__restrict__ slabs, int rows, int c,
                                                                           float *__restrict__ out, int accumulate,
                                                                           int transpose) {
  const int idx = blockIdx.x * kBlock + threadIdx.x, n = kHidden * c;
  if (idx >= n) return;
  const int at = transpose ? (idx % c) * kHidden + idx / c : idx;
  float sum = accumulate ? out[at] : 0.0f;
  for (int r = 0; r < rows; ++r) sum += slabs[(int64_t)r * n + idx];
  out[at] = sum;
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// d_in / n_out rounded up to the fetch width of a variant.
using FetchWidths = Widths<32, 64, 128>;
inline int fetch_class(int n) { return n <= 32 ? 32 : n <= 64 ? 64 : 128; }

template <int KIN, bool SAVE>
static int launch_forward(int grid, hipStream_t s, const float *x, int64_t m, int d_in, const float *w1p, const float *b1,
                          const float4 *w2p, const float *b2, const float *w3p, const float *b3, int n_out, float *out,
                          float *save_h1, float *save_h2) {
  if (const int e = allow_dynamic_lds<&mlp_wide_out_forward_kernel<KIN, SAVE>>()) return e;
  mlp_wide_out_forward_kernel<KIN, SAVE><<<grid, kBlock, tile_lds_bytes(), s>>>(x, m, d_in, w1p, b1, w2p, b2, w3p, b3, n_out,
                                                                               out, save_h1, save_h2);
  return launch_status();
}

template <int KOUT>
static int launch_backward(int grid, hipStream_t s, const float *h1, const float *h2, const float *dout, int64_t m,
                           const float4 *w2tp, const float *w3tp, int n_out, float *dz1, float *dz2, float *partials,
                           int stride) {
  if (const int e = allow_dynamic_lds<&mlp_wide_out_backward_kernel<KOUT>>()) return e;
  mlp_wide_out_backward_kernel<KOUT><<<grid, kBlock, tile_lds_bytes(), s>>>(h1, h2, dout, m, w2tp, w3tp, n_out, dz1, dz2,
                                                                           partials, stride);
  return launch_status();
}

template <int CT>
static int launch_wgrad(int grid, hipStream_t s, const float *a, const float *b, int64_t m, int c, float *slabs) {
  if (const int e = allow_dynamic_lds<&mlp_wide_out_wgrad_kernel<CT>>()) return e;
  mlp_wide_out_wgrad_kernel<CT><<<grid, kWgradThreads, WgradGeo<CT>::kLdsBytes, s>>>(a, b, m, c, slabs);
  return launch_status();
}

// Floats of a pack, or RL8_ESIZE: matrix 0 = W1 [256][n] (n = d_in), 1 = W3 [n][256] for the forward (n = n_out),
// 2 = W3 [n][256] for the data gradient.
inline int64_t pack_floats(int matrix, int n) {
  if (matrix == 0) return n >= 1 && n <= kMaxWideIn ? (int64_t)kHidden * 8 * k_groups(n) : RL8_ESIZE;
  if (n < kMinHead || n > kMaxHead) return RL8_ESIZE;
  if (matrix == 1) return (int64_t)col_tiles(n) * 32 * kHidden;
  if (matrix == 2) return (int64_t)kHidden * 8 * k_groups(n);
  return RL8_ESIZE;
}

}  // namespace wide_out
}  // namespace rl8

using namespace rl8;
using namespace rl8::wide_out;

RL8_API int rl8_mlp_wide_out_supports(int d_in, int n_out) { return supports(d_in, n_out) ? 1 : 0; }

// Dynamic LDS of a launch: kernel 0 the forward (either variant), 1 the data gradient, 2 the weight gradient at c columns.
RL8_API int64_t rl8_mlp_wide_out_lds_bytes(int kernel, int c) {
  if (kernel < 0 || kernel > 2 || c < 1 || c > 128) return RL8_ESIZE;
  if (kernel < 2) return (int64_t)tile_lds_bytes();
  return (int64_t)sizeof(float) * 2 * (kWgradATile + kWgradRows * (32 * col_tiles(c) + 32));
}

RL8_API int64_t rl8_mlp_wide_out_pack_floats(int matrix, int n) { return pack_floats(matrix, n); }

RL8_API int rl8_mlp_wide_out_pack_f32(const float *w, int matrix, int n, float *packed, void *stream) {
  if (!w || !packed) return RL8_ENULL;
  const int64_t total = pack_floats(matrix, n);
  if (total < 0) return RL8_ESIZE;
  if (!aligned4(w) || !aligned16(packed)) return RL8_EALIGN;
  const int rows_w = matrix == 0 ? kHidden : n, cols_w = matrix == 0 ? n : kHidden;
  const int kg = matrix == 1 ? kGroups : k_groups(n);
  mlp_wide_out_pack_kernel<<<(int)(total / kBlock), kBlock, 0, (hipStream_t)stream>>>(w, rows_w, cols_w, matrix == 2, kg,
                                                                                     (int)total, packed);
  return launch_status();
}

RL8_API int rl8_mlp_wide_out_forward_f32(const float *x, int64_t m, int d_in, const float *w1_packed, const float *b1,
                                         const float *w2_packed, const float *b2, const float *w3_packed, const float *b3,
                                         int n_out, float *out, float *save_h1, float *save_h2, void *stream) {
  if (!x || !w1_packed || !b1 || !w2_packed || !b2 || !w3_packed || !b3 || !out) return RL8_ENULL;
  if ((save_h1 == nullptr) != (save_h2 == nullptr)) return RL8_ENULL;
  if (m < 1 || !supports(d_in, n_out)) return RL8_ESIZE;
  if (!aligned16(w1_packed) || !aligned16(w2_packed) || !aligned16(w3_packed) ||
      (save_h1 && (!aligned16(save_h1) || !aligned16(save_h2))))
    return RL8_EALIGN;
  if (!aligned4(x) || !aligned4(b1) || !aligned4(b2) || !aligned4(b3) || !aligned4(out)) return RL8_EALIGN;
  const int grid = tower_grid(m, kTileRows);
  const float4 *w2p = reinterpret_cast<const float4 *>(w2_packed);
  hipStream_t s = (hipStream_t)stream;
  return variant_status(dispatch_width(fetch_class(d_in), FetchWidths{}, [&](auto d) {
    return save_h1 ? launch_forward<d(), true>(grid, s, x, m, d_in, w1_packed, b1, w2p, b2, w3_packed, b3, n_out, out, save_h1, save_h2)
                   : launch_forward<d(), false>(grid, s, x, m, d_in, w1_packed, b1, w2p, b2, w3_packed, b3, n_out, out, save_h1, save_h2);
  }));
}

RL8_API int64_t rl8_mlp_wide_out_partial_floats(int n_out) {
  if (n_out < kMinHead || n_out > kMaxHead) return RL8_ESIZE;
  return 2 * kHidden + n_out;
}

RL8_API int rl8_mlp_wide_out_max_rows(void) { return 2 * kCUs; }

RL8_API int rl8_mlp_wide_out_backward_f32(const float *h1, const float *h2, const float *dout, int64_t m,
                                          const float *w2t_packed, const float *w3t_packed, int n_out, float *dz1_out,
                                          float *dz2_out, float *partials, int *partial_rows_out, void *stream) {
  if (!h1 || !h2 || !dout || !w2t_packed || !w3t_packed || !dz1_out || !dz2_out || !partials || !partial_rows_out)
    return RL8_ENULL;
  if (m < 1 || n_out < kMinHead || n_out > kMaxHead) return RL8_ESIZE;
  if (!aligned16(h1) || !aligned16(h2) || !aligned16(dz1_out) || !aligned16(dz2_out) || !aligned16(w2t_packed) ||
      !aligned16(w3t_packed))
    return RL8_EALIGN;
  if (!aligned4(dout) || !aligned4(partials)) return RL8_EALIGN;
  const int grid = grid_for(m, kTileRows, 2 * kCUs);  // (rl8_mlp_wide_out_max_rows() partial rows: a function of m alone)
  *partial_rows_out = grid;
  const float4 *w2tp = reinterpret_cast<const float4 *>(w2t_packed);
  const int stride = (int)rl8_mlp_wide_out_partial_floats(n_out);
  hipStream_t s = (hipStream_t)stream;
  return variant_status(dispatch_width(fetch_class(n_out), FetchWidths{}, [&](auto n) {
    return launch_backward<n()>(grid, s, h1, h2, dout, m, w2tp, w3t_packed, n_out, dz1_out, dz2_out, partials, stride);
  }));
}

RL8_API int64_t rl8_mlp_wide_out_workspace_bytes(int c) {
  if (c < 1 || c > 128) return RL8_ESIZE;
  return (int64_t)kCUs * kHidden * c * (int64_t)sizeof(float);  // one [256][c] slab per CU
}

RL8_API int rl8_mlp_wide_out_wgrad_f32(const float *a, const float *b, int64_t m, int c, float *workspace, float *out,
                                       int accumulate, int transpose, void *stream) {
  if (!a || !b || !workspace || !out) return RL8_ENULL;
  if (m < 1 || c < 1 || c > 128) return RL8_ESIZE;
  if (!aligned16(a) || !aligned4(b) || !aligned4(workspace) || !aligned4(out)) return RL8_EALIGN;
  const int grid = grid_for(m, kWgradRows, kCUs);
  hipStream_t s = (hipStream_t)stream;
  const int st = variant_status(dispatch_width(col_tiles(c), Widths<1, 2, 3, 4>{}, [&](auto ct) {
    return launch_wgrad<ct()>(grid, s, a, b, m, c, workspace);
  }));
  if (st != RL8_OK) return st;
  const int n = kHidden * c;
  mlp_wide_out_wgrad_reduce_kernel<<<(n + kBlock - 1) / kBlock, kBlock, 0, s>>>(workspace, grid, c, out, accumulate != 0,
                                                                               transpose != 0);
  return launch_status();
}
