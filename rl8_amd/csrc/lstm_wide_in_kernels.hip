// a-9, "wide input" family: the default recurrent models' one-layer, 256-wide LSTM behind observations of 8 to 128
// floats, in fp32 throughout on v_mfma_f32_32x32x2_f32.  lstm_kernels.hip folds [w_ih | bias] into ONE extra k-group of
// the recurrent product, which ends at d_in = 7; here the operand row [h_{t-1} (256) | x_t (d_in) | 1 | 0..] takes
// xg = ceil((d_in + 1) / 8) extra k-groups, 2 to 17, and everything else is that kernel's design: 32 sequences per
// workgroup, the time loop inside the kernel, h_t handed on through LDS, gates and cell update on the accumulators.
// Gate order and the save layouts are those of rl8_lstm_forward_f32, so the backward kernels (lstm_backward_kernel,
// rl8_lstm_rows_backward[_heads]_f32) and the W_hh weight gradients read them as they are.
//
// Forward: compiled per CLASS of xg (2, 4, 8, 17 extra groups: the LDS row pitch 256 + 8 XG + 1, odd, and the shape of
// the x fetch); the k-loop runs the exact 32 + xg groups of the packed weights, so a 24-float observation pays for four
// extra groups whatever its class.  The x tile: thread (row = tid / 8, tid % 8) owns columns tid % 8 + 8 u of its row,
// fetched through a descriptor sized to the tile's valid rows (rows past the end arrive as zeros) one step ahead, behind
// the products; only columns < d_in are written to LDS, so the ones column and the zero padding stay what the prologue
// made them.
//
// Input-weight and bias gradient: dW_ih [1024][d_in] = dG^T x and db [1024] = the column sums of dG, in one launch over
// all M = B L rows, after mlp_wide_in_wgrad_kernel: 8 waves, wave w owns the 32 rows 32 w .. of a gate's [256][d_in + 1]
// block and all ceil((d_in + 1) / 32) column tiles; the x tile in LDS carries a ones column at d_in, so db is column d_in
// of the same product.  Workgroup 4 s + q walks the 32-row tiles s, s + S, .. of gate q (S slabs, a function of M
// alone); slabs are summed in slab order by a second kernel: bitwise reproducible, no atomics.
//
// LDS (dynamic) and workgroups per CU (160 KiB):
//   forward         : [32][256 + 8 XG + 1]                       = 34 944 / 36 992 / 41 088 / 50 304 B, 2 per CU
//   weight gradient : 2 x (dG [32][320] + x [32][32 CT + 32])    = 98 304 .. 131 072 B for CT = 1..5, 1 per CU (8 waves)
//
// The forward template and its tile product live in lstm_wide_in.hip.h, which lstm_stack256_kernels.hip instantiates at
// an input of 256 floats; this unit instantiates the four classes above.
#include "lstm_wide_in.hip.h"

namespace rl8 {
namespace lstm_wide_in {

constexpr int kMinIn = 8;  // lstm_kernels.hip ends at 7
constexpr int kMaxWideIn = 128;

inline bool supports(int d_in) { return d_in >= kMinIn && d_in <= kMaxWideIn; }
inline int group_class(int d_in) {
  const int xg = extra_groups(d_in);
  return xg <= 2 ? 2 : xg <= 4 ? 4 : xg <= 8 ? 8 : 17;
}

// Per gate q, Wcat[j][k] = w_hh[j][k] (k < 256), w_ih[j][k - 256] (k < 256 + d), b_ih[j] + b_hh[j] (k = 256 + d), 0
// beyond, K = 8 kg:  packed[(((q*8 + n)*kg + g)*4 + e)*64 + l] = Wcat[256q + 32n + (l&31)][8g + 4(l>>5) + e]
// (lstm_pack_kernel's scheme with kg - 32 extra k-groups).
__global__ __launch_bounds__(kBlock) void lstm_wide_in_pack_kernel(const float *__restrict__ w_ih,
                                                                   const float *__restrict__ w_hh,
                                                                   const float *__restrict__ b_ih,
                                                                   const float *__restrict__ b_hh, int d_in, int kg,
                                                                   float *__restrict__ packed) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= 4 * 8 * kg * 4 * kWave) return;
  const int l = idx & 63, e = (idx >> 6) & 3, gn = idx >> 8;
  const int g = gn % kg, qn = gn / kg;  // qn = q*8 + n
  const int j = 32 * qn + (l & 31), k = 8 * g + 4 * (l >> 5) + e;
  float v = 0.0f;
  if (k < kHidden)
    v = w_hh[j * kHidden + k];
  else if (k < kHidden + d_in)
    v = w_ih[j * d_in + (k - kHidden)];
  else if (k == kHidden + d_in)
    v = b_ih[j] + b_hh[j];
  packed[idx] = v;
}

// [dW_ih | db] of gate q = blockIdx.x & 3: out[j][c] = sum_s dG[s][256 q + j] * xo[s][c], xo = [x | 1], c <= d_in; the
// reduction over SAMPLES.  mlp_wide_in_wgrad_kernel's tiling with dG rows at a pitch of 1024 floats and the ones column:
// dG rows go HBM -> LDS by direct-to-LDS loads (one 1-KiB row per instruction), x rows through registers; both
// double-buffered, one barrier per tile.  The partial sum is left in slab (blockIdx.x >> 2) of the gate's workspace.
constexpr int kWgradThreads = 512;
constexpr int kWgradRows = 32;  // rows per staged tile
constexpr int kWgradSlabs = kCUs / 4;  // per gate
// Row strides of 16 n floats, and the rows with bit 2 set -- the rows the upper half-wave reads -- shifted by 32 floats:
// the two half-waves of an operand read fall on disjoint banks.
constexpr int kWgradZStride = 320;
constexpr int kWgradZTile = kWgradRows * kWgradZStride;
constexpr int wgrad_column_tiles(int d_in) { return (d_in + 1 + 31) / 32; }
constexpr size_t wgrad_lds_bytes(int ct) { return sizeof(float) * 2 * (kWgradZTile + kWgradRows * (32 * ct + 32)); }

template <int CT>
__global__ __launch_bounds__(kWgradThreads, 1) void lstm_wide_in_wgrad_kernel(const float *__restrict__ dgates,
                                                                              const float *__restrict__ x, int64_t m,
                                                                              int d_in, float *__restrict__ slabs) {
  constexpr int KX = 32 * CT, XS = KX + 32, kBuffer = kWgradZTile + kWgradRows * XS;
  extern __shared__ float lds[];  // [2 buffers][dG tile | x tile]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jl = lane & 31, kh = lane >> 5;
  const int q = blockIdx.x & 3, slab_id = blockIdx.x >> 2, slab_count = gridDim.x >> 2;
  f32x16 acc[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

  const int64_t tiles = (m + kWgradRows - 1) / kWgradRows;
  constexpr int kXPerThread = kWgradRows * KX / kWgradThreads;  // 2 CT
  float xreg[kXPerThread];
  // Wave w fetches rows w, w+8, w+16, w+24 of the gate's dG columns; rows past the end of the data are out of range of
  // the descriptor and arrive as zeros, as do the rows of [x | 1] past m and its columns past d_in.
  auto fetch = [&](int64_t tile, int buffer) {
    const int64_t r0 = tile * kWgradRows;
    const int rows = (int)((m - r0) < kWgradRows ? (m - r0) : kWgradRows);
    const __amdgpu_buffer_rsrc_t zr =
        buffer_rsrc(dgates + r0 * (4 * kHidden) + q * kHidden, ((rows - 1) * 4 * kHidden + kHidden) * 4);
    float *zb = lds + buffer * kBuffer;
#pragma unroll
    for (int u = 0; u < kWgradRows / 8; ++u) {
      const int row = wave + 8 * u;  // bit 2 of the row = bit 2 of the wave
      const int off = row * kWgradZStride + ((wave & 4) ? 32 : 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(zr, zb + off, 16, lane * 16, row * (4 * kHidden * 4), 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kXPerThread; ++u) {
      const int idx = tid + u * kWgradThreads, s = idx / KX, c = idx % KX;
      const bool row_ok = r0 + s < m;
      xreg[u] = (c < d_in && row_ok) ? x[(r0 + s) * d_in + c] : (c == d_in && row_ok) ? 1.0f : 0.0f;
    }
  };
  auto stage_x = [&](int buffer) {
    float *xb = lds + buffer * kBuffer + kWgradZTile;
#pragma unroll
    for (int u = 0; u < kXPerThread; ++u) {
      const int idx = tid + u * kWgradThreads, s = idx / KX, c = idx % KX;
      xb[s * XS + ((s & 4) ? 32 : 0) + c] = xreg[u];
    }
  };
  // One barrier per tile: behind it this tile's operands are in LDS and every wave is done with the other buffer, which
  // the next tile then streams into.
  const int64_t t0 = slab_id, stride = slab_count;
  if (t0 < tiles) fetch(t0, 0);
  int buffer = 0;
  for (int64_t tile = t0; tile < tiles; tile += stride, buffer ^= 1) {
    stage_x(buffer);
    wait_vmcnt0();
    __syncthreads();
    if (tile + stride < tiles) fetch(tile + stride, buffer ^ 1);
    // this lane's rows of k-group g are 8g + 4 kh + e: bit 2 of the row is kh
    const float *za = lds + buffer * kBuffer + kh * (4 * kWgradZStride + 32) + 32 * wave + jl;
    const float *xa = lds + buffer * kBuffer + kWgradZTile + kh * (4 * XS + 32) + jl;
#pragma unroll
    for (int g = 0; g < kWgradRows / 8; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = za[(8 * g + e) * kWgradZStride];
#pragma unroll
        for (int t = 0; t < CT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xa[(8 * g + e) * XS + 32 * t], acc[t], 0, 0, 0);
      }
  }
  // Partial slab of this workgroup: slab[j][c], c <= d_in.
  const int width = d_in + 1;
  float *slab = slabs + ((int64_t)q * slab_count + slab_id) * kHidden * width;
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * kh;
      const int c = 32 * t + jl;
      if (c < width) slab[j * width + c] = acc[t][r];
    }
}

// dw_ih[256 q + j][c] / db[256 q + j] = the sum over the gate's slabs, in slab order; idx = (256 q + j) * (d_in + 1) + c.
__global__ __launch_bounds__(kBlock) void lstm_wide_in_wgrad_reduce_kernel(const float *__restrict__ slabs, int slab_count,
                                                                           int d_in, float *__restrict__ dw_ih,
                                                                           float *__restrict__ db) {
  const int width = d_in + 1, per_gate = kHidden * width;
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= 4 * per_gate) return;
  const int q = idx / per_gate, rest = idx - q * per_gate;
  const float *first = slabs + (int64_t)q * slab_count * per_gate + rest;
  float sum = 0.0f;
  for (int r = 0; r < slab_count; ++r) sum += first[(int64_t)r * per_gate];
  const int row = idx / width, c = idx - row * width;
  if (c < d_in)
    dw_ih[row * d_in + c] = sum;
  else
    db[row] = sum;
}

template <int CT>
static int launch_wgrad(int grid, hipStream_t s, const float *dgates, const float *x, int64_t m, int d_in, float *slabs) {
  if (const int e = allow_dynamic_lds<&lstm_wide_in_wgrad_kernel<CT>>()) return e;
  lstm_wide_in_wgrad_kernel<CT><<<grid, kWgradThreads, wgrad_lds_bytes(CT), s>>>(dgates, x, m, d_in, slabs);
  return launch_status();
}

}  // namespace lstm_wide_in
}  // namespace rl8

using namespace rl8;
using namespace rl8::lstm_wide_in;

RL8_API int rl8_lstm_wide_in_supports(int d_in) { return supports(d_in) ? 1 : 0; }

// Dynamic LDS of a launch: kernel 0 the forward (either variant), 1 the weight gradient, at d_in.
RL8_API int64_t rl8_lstm_wide_in_lds_bytes(int kernel, int d_in) {
  if (kernel < 0 || kernel > 1 || !supports(d_in)) return RL8_ESIZE;
  if (kernel == 0) return (int64_t)forward_lds_bytes(group_class(d_in));
  return (int64_t)wgrad_lds_bytes(wgrad_column_tiles(d_in));
}

RL8_API int64_t rl8_lstm_wide_in_pack_floats(int d_in) {
  if (!supports(d_in)) return RL8_ESIZE;
  return (int64_t)4 * kHidden * 8 * k_groups(d_in);
}

RL8_API int rl8_lstm_wide_in_pack_f32(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, int d_in,
                                      float *packed, void *stream) {
  if (!w_ih || !w_hh || !b_ih || !b_hh || !packed) return RL8_ENULL;
  if (!supports(d_in)) return RL8_ESIZE;
  if (!aligned16(packed)) return RL8_EALIGN;
  if (!aligned4(w_ih) || !aligned4(w_hh) || !aligned4(b_ih) || !aligned4(b_hh)) return RL8_EALIGN;
  const int kg = k_groups(d_in);
  lstm_wide_in_pack_kernel<<<4 * 8 * kg * 4 * kWave / kBlock, kBlock, 0, (hipStream_t)stream>>>(w_ih, w_hh, b_ih, b_hh,
                                                                                                d_in, kg, packed);
  return launch_status();
}

RL8_API int rl8_lstm_wide_in_forward_f32(const float *x, int64_t b, int l, int d_in, const float *h0, const float *c0,
                                         const float *w_packed, float *hs, float *hn, float *cn, float *save_gates,
                                         float *save_c, void *stream) {
  if (!x || !h0 || !c0 || !w_packed || !hs || !hn || !cn) return RL8_ENULL;
  if ((save_gates == nullptr) != (save_c == nullptr)) return RL8_ENULL;
  if (b <= 0 || l <= 0) return RL8_ESIZE;
  if (!supports(d_in)) return RL8_ESIZE;
  // buffer descriptors address one tile's rows with 32-bit offsets
  if ((int64_t)kRows * l * 4 * kHidden * 4 >= (int64_t)1 << 31) return RL8_ESIZE;
  if (!aligned16(w_packed) || !aligned16(h0)) return RL8_EALIGN;
  if (!aligned4(x) || !aligned4(c0) || !aligned4(hs) || !aligned4(hn) || !aligned4(cn) || !aligned4(save_gates) ||
      !aligned4(save_c))
    return RL8_EALIGN;
  const int64_t tiles = (b + kRows - 1) / kRows;
  const int grid = (int)(tiles < 2 * kCUs ? tiles : 2 * kCUs);
  hipStream_t s = (hipStream_t)stream;
  return variant_status(dispatch_width(group_class(d_in), Widths<2, 4, 8, 17>{}, [&](auto xg) {
    return save_gates ? launch_forward<xg(), true>(grid, s, x, b, l, d_in, h0, c0, w_packed, hs, hn, cn, save_gates, save_c)
                      : launch_forward<xg(), false>(grid, s, x, b, l, d_in, h0, c0, w_packed, hs, hn, cn, save_gates, save_c);
  }));
}

RL8_API int64_t rl8_lstm_wide_in_workspace_bytes(int d_in) {
  if (!supports(d_in)) return RL8_ESIZE;
  return (int64_t)4 * kWgradSlabs * kHidden * (d_in + 1) * (int64_t)sizeof(float);  // [gate][slab][256][d_in + 1]
}

RL8_API int rl8_lstm_wide_in_wgrad_f32(const float *dgates, const float *x, int64_t m, int d_in, float *workspace,
                                       float *dw_ih_out, float *db_out, void *stream) {
  if (!dgates || !x || !workspace || !dw_ih_out || !db_out) return RL8_ENULL;
  if (m < 1 || !supports(d_in)) return RL8_ESIZE;
  if (!aligned16(dgates) || !aligned4(x) || !aligned4(workspace) || !aligned4(dw_ih_out) || !aligned4(db_out))
    return RL8_EALIGN;
  const int slab_count = grid_for(m, kWgradRows, kWgradSlabs);  // a function of m alone
  hipStream_t s = (hipStream_t)stream;
  const int st = variant_status(dispatch_width(wgrad_column_tiles(d_in), Widths<1, 2, 3, 4, 5>{}, [&](auto ct) {
    return launch_wgrad<ct()>(4 * slab_count, s, dgates, x, m, d_in, workspace);
  }));
  if (st != RL8_OK) return st;
  const int n = 4 * kHidden * (d_in + 1);
  lstm_wide_in_wgrad_reduce_kernel<<<(n + kBlock - 1) / kBlock, kBlock, 0, s>>>(workspace, slab_count, d_in, dw_ih_out,
                                                                                db_out);
  return launch_status();
}
