// a-9, "stack256" family: the layers ABOVE the first of a width-256 LSTM stack (num_layers >= 2), in fp32 throughout on
// v_mfma_f32_32x32x2_f32.  Such a layer's input row is the 256 floats the layer below left in hs[b][t]; layer 0 runs on
// the kernels of its own input width (lstm_kernels.hip, lstm_split_kernels.hip, lstm_wide_in_kernels.hip).
//
// Forward: lstm_wide_in.hip.h's forward at d_in = 256 -- the operand row [h_{t-1} (256) | x_t (256) | 1 | 0..],
// K = 256 + 8 * 33 = 520, 65 k-groups, the class of 33 extra groups.  The input product stays inside the time loop: the
// weights are streamed from L2 either way (no W_hh in registers as at 64 / 128), the MFMA work is the same, and a
// projection array would cost 4 KiB written and 4 KiB read per row-step.  x_t, a dense 1-KiB row, goes HBM -> LDS by the
// direct row load h0 uses, between a step's two barriers (32 floats per thread held over the products spilled).  Gate
// order and the save layouts are rl8_lstm_forward_f32's.
//
// Input and bias gradient: dx [M][256] = dG [M][1024] x W_ih [1024][256] -- the dL/dhs of the layer below -- and
// db [1024] = the column sums of dG, from ONE read of dG.  The product is lstm_backward_kernel's
// dh_{t-1} = sum_q dG_q W_hh[q] with W_ih in W_hh's place (the same pack, rl8_mlp_pack_w2_f32(transposed) per gate, the
// same TileGemmT<1> products accumulating over the four gates), but over all M = B L rows at once: a workgroup walks
// 32-row tiles, each as four [32][257] quarter tiles (one gate's columns) that go HBM -> LDS by direct-to-LDS loads, one
// 1-KiB row per instruction, into two buffers: quarter s + 1 streams in while quarter s is multiplied.  Thread c sums
// column c of every quarter tile (32 rows in row order, then onto its running sum, tiles in order) and leaves the
// workgroup's 1024 partial sums in its slab; a second kernel adds the slabs in slab order in fp64.  Grids are functions
// of M alone, nothing is atomic: bitwise reproducible.
//
// LDS (dynamic) and workgroups per CU (160 KiB):
//   forward : [32][256 + 8 * 33 + 1] = 66 688 B, 2 per CU
//   dx / db : 2 x [32][257]          = 65 792 B, 2 per CU
#include "lstm_wide_in.hip.h"

namespace rl8 {
namespace lstm_stack256 {

using namespace rl8::lstm_wide_in;

constexpr int kIn = kHidden;  // the layer below's outputs
constexpr int kXgClass = 33;
constexpr int kKGroups = k_groups(kIn);  // 65
static_assert(extra_groups(kIn) == kXgClass && class_max_in(kXgClass) == kIn, "the class of a 256-float input");

// lstm_wide_in_pack_kernel's layout at d_in = 256: per gate q, Wcat[j] = [w_hh[j] (256) | w_ih[j] (256) | b_ih[j] +
// b_hh[j] | 0 x 7]:  packed[(((q*8 + n)*65 + g)*4 + e)*64 + l] = Wcat[256q + 32n + (l&31)][8g + 4(l>>5) + e].
__global__ __launch_bounds__(kBlock) void lstm_stack256_pack_kernel(const float *__restrict__ w_ih,
                                                                    const float *__restrict__ w_hh,
                                                                    const float *__restrict__ b_ih,
                                                                    const float *__restrict__ b_hh,
                                                                    float *__restrict__ packed) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= 4 * 8 * kKGroups * 4 * kWave) return;
  const int l = idx & 63, e = (idx >> 6) & 3, gn = idx >> 8;
  const int g = gn % kKGroups, qn = gn / kKGroups;  // qn = q*8 + n
  const int j = 32 * qn + (l & 31), k = 8 * g + 4 * (l >> 5) + e;
  float v = 0.0f;
  if (k < kHidden)
    v = w_hh[j * kHidden + k];
  else if (k < kHidden + kIn)
    v = w_ih[j * kIn + (k - kHidden)];
  else if (k == kHidden + kIn)
    v = b_ih[j] + b_hh[j];
  packed[idx] = v;
}

constexpr int kDxRows = 32;                         // rows per tile
constexpr int kDxTile = kDxRows * kLdsStride;       // one quarter tile: a gate's 256 columns of 32 rows
constexpr size_t kDxLdsBytes = sizeof(float) * 2 * kDxTile;
inline int dx_grid(int64_t m) { return grid_for(m, kDxRows, 2 * kCUs); }

// dx rows and this workgroup's slab of column sums; wiht_packed: W_ih^T per gate as lstm_backward_kernel reads W_hh^T.
__global__ __launch_bounds__(kBlock, 2) void lstm_stack256_dx_kernel(const float *__restrict__ dgates, int64_t m,
                                                                     const float *__restrict__ wiht_packed,
                                                                     float *__restrict__ dx, float *__restrict__ slabs) {
  extern __shared__ float lds[];  // [2 buffers][32][257]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5, l31 = lane & 31;

  __amdgpu_buffer_rsrc_t wrsrc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) wrsrc[q] = buffer_rsrc(wiht_packed + q * kHidden * kHidden, kHidden * kHidden * 4);
  TileGemmT<1> gemm(wrsrc[0], wave, lane);
  __builtin_amdgcn_s_setprio(kValuPhasePriority);
  const int v_out = (4 * hh * kHidden + 64 * wave + l31) * 4;  // accumulator slot (nt, r): lstm_backward_kernel's

  // Quarter q of the tile at row r0 -> buffer: wave w fetches rows w, w + 4, ..; rows past the end of the data are out
  // of range of the descriptor and arrive as zeros.
  auto fetch = [&](int64_t tile, int q, int buffer) {
    const int64_t r0 = tile * kDxRows;
    const int rows = (int)((m - r0) < kDxRows ? (m - r0) : kDxRows);
    const __amdgpu_buffer_rsrc_t zr =
        buffer_rsrc(dgates + r0 * (4 * kHidden) + q * kHidden, ((rows - 1) * 4 * kHidden + kHidden) * 4);
    float *zb = lds + buffer * kDxTile;
#pragma unroll
    for (int u = 0; u < kDxRows / 4; ++u) {
      const int row = wave + 4 * u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(zr, zb + row * kLdsStride, 16, lane * 16, row * (4 * kHidden * 4), 0, 0);
    }
  };

  float colsum[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // column 256 q + tid
  const int64_t tiles = (m + kDxRows - 1) / kDxRows;
  if ((int64_t)blockIdx.x < tiles) fetch(blockIdx.x, 0, 0);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kDxRows;
    const int rows = (int)((m - r0) < kDxRows ? (m - r0) : kDxRows);
    f32x16 acc[1][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float *zb = lds + (q & 1) * kDxTile;
      gemm.bp = wrsrc[q];
      gemm.prefetch();
      wait_vmcnt0();
      __syncthreads();  // this quarter is in LDS and every wave is done with the other buffer, which the next streams into
      if (q < 3)
        fetch(tile, q + 1, (q + 1) & 1);
      else if (tile + gridDim.x < tiles)
        fetch(tile + gridDim.x, 0, 0);
      float sum = 0.0f;
#pragma unroll
      for (int row = 0; row < kDxRows; ++row) sum += zb[row * kLdsStride + tid];
      colsum[q] += sum;
      if (q == 0)
        gemm.run<false>(zb, acc);
      else
        gemm.run<true>(zb, acc);
    }
    const __amdgpu_buffer_rsrc_t dxr = buffer_rsrc(dx + r0 * kHidden, rows * kHidden * 4);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        buffer_store_f32(acc[0][nt][r], dxr, v_out + nt * 128, ((r & 3) + 8 * (r >> 2)) * (kHidden * 4));
  }
  float *slab = slabs + (int64_t)blockIdx.x * (4 * kHidden);
#pragma unroll
  for (int q = 0; q < 4; ++q) slab[q * kHidden + tid] = colsum[q];
}

// db[j] = the sum of the slabs' entry j, in slab order, in fp64.
__global__ __launch_bounds__(kBlock) void lstm_stack256_db_reduce_kernel(const float *__restrict__ slabs, int slab_count,
                                                                         float *__restrict__ db) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  double sum = 0.0;
  for (int r = 0; r < slab_count; ++r) sum += (double)slabs[(int64_t)r * (4 * kHidden) + j];
  db[j] = (float)sum;
}

}  // namespace lstm_stack256
}  // namespace rl8

using namespace rl8;
using namespace rl8::lstm_stack256;

// 1: this build has the upper-layer kernels of a width-256 stack (host only).
RL8_API int rl8_lstm_stack256_supports(void) { return 1; }

// Dynamic LDS of a launch: kernel 0 the forward (either variant), 1 the input / bias gradient.
RL8_API int64_t rl8_lstm_stack256_lds_bytes(int kernel) {
  if (kernel < 0 || kernel > 1) return RL8_ESIZE;
  return kernel == 0 ? (int64_t)forward_lds_bytes(kXgClass) : (int64_t)kDxLdsBytes;
}

RL8_API int64_t rl8_lstm_stack256_pack_floats(void) { return (int64_t)4 * kHidden * 8 * kKGroups; }

RL8_API int rl8_lstm_stack256_pack_f32(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                       float *packed, void *stream) {
  if (!w_ih || !w_hh || !b_ih || !b_hh || !packed) return RL8_ENULL;
  if (!aligned16(packed)) return RL8_EALIGN;
  if (!aligned4(w_ih) || !aligned4(w_hh) || !aligned4(b_ih) || !aligned4(b_hh)) return RL8_EALIGN;
  lstm_stack256_pack_kernel<<<4 * 8 * kKGroups * 4 * kWave / kBlock, kBlock, 0, (hipStream_t)stream>>>(w_ih, w_hh, b_ih,
                                                                                                      b_hh, packed);
  return launch_status();
}

RL8_API int rl8_lstm_stack256_forward_f32(const float *x, int64_t b, int l, const float *h0, const float *c0,
                                          const float *w_packed, float *hs, float *hn, float *cn, float *save_gates,
                                          float *save_c, void *stream) {
  if (!x || !h0 || !c0 || !w_packed || !hs || !hn || !cn) return RL8_ENULL;
  if ((save_gates == nullptr) != (save_c == nullptr)) return RL8_ENULL;
  if (b <= 0 || l <= 0) return RL8_ESIZE;
  // buffer descriptors address one tile's rows with 32-bit offsets
  if ((int64_t)kRows * l * 4 * kHidden * 4 >= (int64_t)1 << 31) return RL8_ESIZE;
  if (!aligned16(w_packed) || !aligned16(h0) || !aligned16(x)) return RL8_EALIGN;  // (rows that go HBM -> LDS)
  if (!aligned4(c0) || !aligned4(hs) || !aligned4(hn) || !aligned4(cn) || !aligned4(save_gates) ||
      !aligned4(save_c))
    return RL8_EALIGN;
  const int64_t tiles = (b + kRows - 1) / kRows;
  const int grid = (int)(tiles < 2 * kCUs ? tiles : 2 * kCUs);
  hipStream_t s = (hipStream_t)stream;
  return save_gates
             ? launch_forward<kXgClass, true>(grid, s, x, b, l, kIn, h0, c0, w_packed, hs, hn, cn, save_gates, save_c)
             : launch_forward<kXgClass, false>(grid, s, x, b, l, kIn, h0, c0, w_packed, hs, hn, cn, save_gates, save_c);
}

// One [1024] slab of column sums per workgroup of the dx launch over m rows.
RL8_API int64_t rl8_lstm_stack256_workspace_bytes(int64_t m) {
  if (m < 1) return RL8_ESIZE;
  return (int64_t)dx_grid(m) * 4 * kHidden * (int64_t)sizeof(float);
}

RL8_API int rl8_lstm_stack256_dx_f32(const float *dgates, int64_t m, const float *wiht_packed, float *workspace,
                                     float *dx_out, float *db_out, void *stream) {
  if (!dgates || !wiht_packed || !workspace || !dx_out || !db_out) return RL8_ENULL;
  if (m < 1) return RL8_ESIZE;
  if (!aligned16(dgates) || !aligned16(wiht_packed)) return RL8_EALIGN;
  if (!aligned4(workspace) || !aligned4(dx_out) || !aligned4(db_out)) return RL8_EALIGN;
  if (const int e = allow_dynamic_lds<&lstm_stack256_dx_kernel>()) return e;
  const int grid = dx_grid(m);  // a function of m alone
  hipStream_t s = (hipStream_t)stream;
  lstm_stack256_dx_kernel<<<grid, kBlock, kDxLdsBytes, s>>>(dgates, m, wiht_packed, dx_out, workspace);
  if (const int st = launch_status()) return st;
  lstm_stack256_db_reduce_kernel<<<4 * kHidden / kBlock, kBlock, 0, s>>>(workspace, grid, db_out);
  return launch_status();
}
