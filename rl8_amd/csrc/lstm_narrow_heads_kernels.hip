// The output heads of the narrow recurrent models: a few Linear(H, n) layers on the outputs of an LSTM of hidden width
// H = 64 or 128 (lstm_narrow_kernels.hip), evaluated together: out [M][n] = h [M][H] x W^T + b, n <= 8.  The width-256
// heads are lstm_kernels.hip's; a library GEMM with N = 1..3 runs far below HBM speed at these shapes.
//
// Forward: one pass over h (4 H bytes per row), four lanes per row (lstm_narrow_heads.hip.h), the single and the pair
// form (two layers that stay separate arrays) through the same per-row arithmetic: bit-identical.
//
// Backward: thread = input unit j, 256 / H rows in flight per workgroup, a workgroup walks a contiguous slice of the
// rows: dh[s][j] = sum_q dout[s][q] w[q][j] (optional), dW[q][j] += dout[s][q] h[s][j], db[q] += dout[s][q] in fp32;
// the workgroup's row groups are added in fp64 in a fixed order into one slab [dW (n H) | db (n)], and
// linear_heads_narrow_reduce_kernel adds the slabs in fp64 in a fixed order.  The grid is a function of M alone and
// there are no float atomics, so the gradients repeat bit for bit.
#include "lstm_narrow_heads.hip.h"

namespace rl8 {
namespace narrow_heads {

struct ForwardArgs {
  const float *w, *bias;
  float *out;
  int n_a;
  const float *w_b, *bias_b;
  float *out_b;
};

template <int H, int NOUT>
__global__ __launch_bounds__(kBlock) void linear_heads_narrow_forward_kernel(const float4 *__restrict__ h, int64_t m,
                                                                             ForwardArgs a) {
  __shared__ float4 ws[NOUT * H / 4];
  const int n_a = a.n_a, n_b = NOUT - n_a;
  stage_weights<H>(ws, NOUT, a.w, n_a, a.w_b);
  __syncthreads();
  const int q4 = threadIdx.x & 3;
  const int64_t stride = (int64_t)gridDim.x * (kBlock / 4);
  for (int64_t row = (int64_t)blockIdx.x * (kBlock / 4) + (threadIdx.x >> 2); row < m; row += stride) {
    float o[NOUT];
    row_dots<H, NOUT>(h + row * (H / 4), ws, q4, o);
    if (q4 != 0) continue;
#pragma unroll
    for (int q = 0; q < NOUT; ++q) {
      if (q < n_a) a.out[row * n_a + q] = o[q] + a.bias[q];
      else a.out_b[row * n_b + (q - n_a)] = o[q] + a.bias_b[q - n_a];
    }
  }
}

constexpr int kSlabCap = 1024;     // most workgroups (slabs) of the backward
constexpr int kMinRowsPerSlab = 64;

// Rows per workgroup and the workgroup count: functions of m alone.
inline void slabs_for(int64_t m, int64_t *per, int *count) {
  int64_t want = (m + kMinRowsPerSlab - 1) / kMinRowsPerSlab;
  if (want > kSlabCap) want = kSlabCap;
  *per = (m + want - 1) / want;
  *count = (int)((m + *per - 1) / *per);
}

__host__ __device__ inline int slab_floats(int hidden, int n_out) { return n_out * hidden + n_out; }

template <int H, int NOUT>
__global__ __launch_bounds__(kBlock) void linear_heads_narrow_backward_kernel(
    const float *__restrict__ h, const float *__restrict__ dout, int64_t m, const float *__restrict__ w,
    float *__restrict__ dh, int64_t per_block, float *__restrict__ slabs) {
  constexpr int RG = kBlock / H;  // row groups: rows in flight
  __shared__ float red[RG * NOUT * H];
  __shared__ float red_b[RG * NOUT];
  const int j = threadIdx.x % H, rg = threadIdx.x / H;
  float wr[NOUT], dw[NOUT], db[NOUT];
#pragma unroll
  for (int q = 0; q < NOUT; ++q) {
    wr[q] = w[q * H + j];
    dw[q] = db[q] = 0.0f;
  }
  const int64_t r0 = blockIdx.x * per_block;
  const int64_t r1 = r0 + per_block < m ? r0 + per_block : m;
#pragma unroll 4
  for (int64_t s = r0 + rg; s < r1; s += RG) {
    const float hv = h[s * H + j];
    float g = 0.0f;
#pragma unroll
    for (int q = 0; q < NOUT; ++q) {
      const float d = dout[s * NOUT + q];
      g = __builtin_fmaf(d, wr[q], g);
      dw[q] = __builtin_fmaf(d, hv, dw[q]);
      db[q] += d;
    }
    if (dh) dh[s * H + j] = g;  // (null: parameter gradients only -- the caller forms dh where it is used)
  }
#pragma unroll
  for (int q = 0; q < NOUT; ++q) {
    red[(rg * NOUT + q) * H + j] = dw[q];
    if (j == 0) red_b[rg * NOUT + q] = db[q];
  }
  __syncthreads();
  if (rg != 0) return;
  float *slab = slabs + (int64_t)blockIdx.x * slab_floats(H, NOUT);
#pragma unroll
  for (int q = 0; q < NOUT; ++q) {
    double sw = 0.0, sb = 0.0;
#pragma unroll
    for (int g = 0; g < RG; ++g) {
      sw += (double)red[(g * NOUT + q) * H + j];
      sb += (double)red_b[g * NOUT + q];
    }
    slab[q * H + j] = (float)sw;
    if (j == 0) slab[NOUT * H + q] = (float)sb;
  }
}

// grads[e] = sum over the slabs in fp64, in a fixed order: workgroup = element e; thread t adds slabs t, t + 256, ..
// in that order, and the 256 partial sums are added pairwise in a fixed tree.  (One thread per element walking every
// slab took longer than the backward kernel itself at 1024 slabs.)
__global__ __launch_bounds__(kBlock) void linear_heads_narrow_reduce_kernel(const float *__restrict__ slabs,
                                                                            int slab_count, int floats,
                                                                            float *__restrict__ grads) {
  __shared__ double part[kBlock];
  const int e = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  for (int g = t; g < slab_count; g += kBlock) s += (double)slabs[(int64_t)g * floats + e];
  part[t] = s;
  __syncthreads();
#pragma unroll
  for (int half = kBlock / 2; half > 0; half >>= 1) {
    if (t < half) part[t] += part[t + half];
    __syncthreads();
  }
  if (t == 0) grads[e] = (float)part[0];
}

template <int H, int NOUT>
void launch_forward(int grid, hipStream_t s, const float4 *h, int64_t m, const ForwardArgs &a) {
  linear_heads_narrow_forward_kernel<H, NOUT><<<grid, kBlock, 0, s>>>(h, m, a);
}

template <int H>
int forward(const float *h, int64_t m, const ForwardArgs &a, int n_out, void *stream) {
  const int grid = grid_for(m, kBlock / 4);
  hipStream_t s = (hipStream_t)stream;
  const float4 *h4 = reinterpret_cast<const float4 *>(h);
  switch (n_out) {
    case 1: launch_forward<H, 1>(grid, s, h4, m, a); break;
    case 2: launch_forward<H, 2>(grid, s, h4, m, a); break;
    case 3: launch_forward<H, 3>(grid, s, h4, m, a); break;
    case 4: launch_forward<H, 4>(grid, s, h4, m, a); break;
    case 5: launch_forward<H, 5>(grid, s, h4, m, a); break;
    case 6: launch_forward<H, 6>(grid, s, h4, m, a); break;
    case 7: launch_forward<H, 7>(grid, s, h4, m, a); break;
    default: launch_forward<H, 8>(grid, s, h4, m, a); break;
  }
  return launch_status();
}

template <int H, int NOUT>
void launch_backward(int grid, hipStream_t s, const float *h, const float *dout, int64_t m, const float *w, float *dh,
                     int64_t per, float *slabs) {
  linear_heads_narrow_backward_kernel<H, NOUT><<<grid, kBlock, 0, s>>>(h, dout, m, w, dh, per, slabs);
}

template <int H>
int backward(const float *h, const float *dout, int64_t m, const float *w, int n_out, float *dh, float *slabs,
             float *grads, void *stream) {
  int64_t per = 0;
  int count = 0;
  slabs_for(m, &per, &count);
  hipStream_t s = (hipStream_t)stream;
  switch (n_out) {
    case 1: launch_backward<H, 1>(count, s, h, dout, m, w, dh, per, slabs); break;
    case 2: launch_backward<H, 2>(count, s, h, dout, m, w, dh, per, slabs); break;
    case 3: launch_backward<H, 3>(count, s, h, dout, m, w, dh, per, slabs); break;
    case 4: launch_backward<H, 4>(count, s, h, dout, m, w, dh, per, slabs); break;
    case 5: launch_backward<H, 5>(count, s, h, dout, m, w, dh, per, slabs); break;
    case 6: launch_backward<H, 6>(count, s, h, dout, m, w, dh, per, slabs); break;
    case 7: launch_backward<H, 7>(count, s, h, dout, m, w, dh, per, slabs); break;
    default: launch_backward<H, 8>(count, s, h, dout, m, w, dh, per, slabs); break;
  }
  if (const int st = launch_status()) return st;
  const int floats = slab_floats(H, n_out);
  linear_heads_narrow_reduce_kernel<<<floats, kBlock, 0, s>>>(slabs, count, floats, grads);
  return launch_status();
}

inline bool width_ok(int hidden) { return hidden == 64 || hidden == 128; }
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace narrow_heads
}  // namespace rl8

using namespace rl8;

RL8_API int64_t rl8_linear_heads_narrow_workspace_bytes(int64_t m, int hidden, int n_out) {
  if (m <= 0 || m >= ((int64_t)1 << 40) || !narrow_heads::width_ok(hidden) || n_out <= 0 ||
      n_out > narrow_heads::kMaxOut)
    return RL8_ESIZE;
  int64_t per = 0;
  int count = 0;
  narrow_heads::slabs_for(m, &per, &count);
  return (int64_t)count * narrow_heads::slab_floats(hidden, n_out) * (int64_t)sizeof(float);
}

RL8_API int rl8_linear_heads_narrow_forward_f32(const float *h, int64_t m, int hidden, const float *w, const float *b,
                                                int n_out, float *out, void *stream) {
  if (!h || !w || !b || !out) return RL8_ENULL;
  if (m <= 0 || m >= ((int64_t)1 << 40) || !narrow_heads::width_ok(hidden) || n_out <= 0 ||
      n_out > narrow_heads::kMaxOut)
    return RL8_ESIZE;
  if (!aligned16(h) || !aligned16(w) || !narrow_heads::aligned4(b) || !narrow_heads::aligned4(out)) return RL8_EALIGN;
  const narrow_heads::ForwardArgs a{w, b, out, n_out, nullptr, nullptr, nullptr};
  return hidden == 64 ? narrow_heads::forward<64>(h, m, a, n_out, stream)
                      : narrow_heads::forward<128>(h, m, a, n_out, stream);
}

RL8_API int rl8_linear_heads_narrow_forward_pair_f32(const float *h, int64_t m, int hidden, const float *w_a,
                                                     const float *b_a, int n_a, float *out_a, const float *w_b,
                                                     const float *b_b, int n_b, float *out_b, void *stream) {
  if (!h || !w_a || !b_a || !out_a || !w_b || !b_b || !out_b) return RL8_ENULL;
  if (m <= 0 || m >= ((int64_t)1 << 40) || !narrow_heads::width_ok(hidden) || n_a <= 0 || n_b <= 0 ||
      n_a + n_b > narrow_heads::kMaxOut)
    return RL8_ESIZE;
  if (!aligned16(h) || !aligned16(w_a) || !aligned16(w_b)) return RL8_EALIGN;
  for (const void *p : {(const void *)b_a, (const void *)out_a, (const void *)b_b, (const void *)out_b})
    if (!narrow_heads::aligned4(p)) return RL8_EALIGN;
  const narrow_heads::ForwardArgs a{w_a, b_a, out_a, n_a, w_b, b_b, out_b};
  return hidden == 64 ? narrow_heads::forward<64>(h, m, a, n_a + n_b, stream)
                      : narrow_heads::forward<128>(h, m, a, n_a + n_b, stream);
}

RL8_API int rl8_linear_heads_narrow_backward_f32(const float *h, const float *dout, int64_t m, int hidden,
                                                 const float *w, int n_out, float *dh_out, float *workspace,
                                                 float *grads_out, void *stream) {
  if (!h || !dout || !w || !workspace || !grads_out) return RL8_ENULL;  // (dh_out may be null)
  if (m <= 0 || m >= ((int64_t)1 << 40) || !narrow_heads::width_ok(hidden) || n_out <= 0 ||
      n_out > narrow_heads::kMaxOut)
    return RL8_ESIZE;
  for (const void *p : {(const void *)h, (const void *)dout, (const void *)w, (const void *)dh_out,
                        (const void *)workspace, (const void *)grads_out})
    if (!narrow_heads::aligned4(p)) return RL8_EALIGN;
  return hidden == 64 ? narrow_heads::backward<64>(h, dout, m, w, n_out, dh_out, workspace, grads_out, stream)
                      : narrow_heads::backward<128>(h, dout, m, w, n_out, dh_out, workspace, grads_out, stream);
}
