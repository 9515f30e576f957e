// The core of multihead attention over short sequences, softmax(q k^T scale + masks) v, forward and backward, under
// rl8_amd.nn's SelfAttention / CrossAttention (rl8_amd/nn/fused_attention.py).  Tq, Tk <= 64, head width D <= 16, fp32.
// Compiled with -ffp-contract=off.
//
// q rows [B][Tq] and k, v rows [B][Tk] each have a base pointer and a row stride in floats, head h of a row being the D
// floats at h D: a packed [B][T][3E] or [B][Tk][2E] projection is read, and its gradient written, in place.
// `key_padding` [B][Tk] bytes, NONZERO = PADDED (torch's key_padding_mask, what rl8_window_last / rl8_gather_windows
// write -- the opposite of the rl8_masked_* kernels' mask); `bias` [Tq][Tk] is added to the scaled scores and may hold
// -inf.  A query without an admissible key has P = 0: out = 0, lse = +inf, and exp(s - lse) = 0 carries that through
// both backward kernels without a case of its own.
//
// One lane holds one (b, q, h) -- forward and dQ -- or one (b, t, h) -- dK, dV -- with the loop over the other sequence
// inside it and D a template parameter, so that a head's q, k, v, dout and accumulators are registers.  No LDS, no
// scratch, no atomics and no reduction across lanes: gradients are the same bits on every run.  The scores are formed
// again where they are needed (twice in the forward: the maximum, then the sums) instead of being kept; a row's k and v
// come out of L1 across the Tq H lanes that share them.
#include <math.h>

#include "common.hip.h"

namespace rl8 {
namespace {

constexpr int kMaxT = 64;
constexpr int kMaxD = 16;

// Lanes run over flattened (b, x, h), consecutive lanes consecutive in that order (a wave's stores of out / dq / dk / dv
// are runs of E floats); the 32-bit divisions where the count allows, as for_each_pair of masked_kernels.hip.
template <class F>
__device__ __forceinline__ void for_each_head_row(int64_t b, int t, int heads, F &&f) {
  const int64_t rows = b * t;
  const int64_t total = rows * heads;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const bool narrow = total <= 0x7fffffff;  // (wave-uniform)
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
    const int64_t row = narrow ? (int64_t)((uint32_t)i / (uint32_t)heads) : i / heads;
    const int64_t batch = narrow ? (int64_t)((uint32_t)row / (uint32_t)t) : row / t;
    f(batch, (int)(row - batch * t), (int)(i - row * heads), row);
  }
}

template <int D>
__device__ __forceinline__ void load_head(const float *p, float (&x)[D]) {
#pragma unroll
  for (int c = 0; c < D; ++c) x[c] = p[c];
}

template <int D>
__device__ __forceinline__ float dot_head(const float (&a)[D], const float *b) {
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < D; ++c) s = s + a[c] * b[c];
  return s;
}

// s[q, t] = scale (q . k_t) + bias[q, t], -inf at a padded key.
struct Scores {
  const uint8_t *padded;  // the batch row's [Tk] bytes, or NULL
  const float *bias;      // the query's [Tk] floats, or NULL
  float scale;
  __device__ __forceinline__ float operator()(float qk, int t) const {
    float s = scale * qk;
    if (bias) s = s + bias[t];
    return (padded && padded[t]) ? -INFINITY : s;
  }
};

template <int D>
__global__ __launch_bounds__(kBlock) void attention_forward_kernel(
    const float *__restrict__ q, int64_t q_stride, const float *__restrict__ k, const float *__restrict__ v,
    int64_t kv_stride, const uint8_t *__restrict__ key_padding, const float *__restrict__ bias, int64_t b, int tq, int tk,
    int heads, float scale, float *__restrict__ out, float *__restrict__ lse) {
  for_each_head_row(b, tq, heads, [&](int64_t batch, int qi, int h, int64_t row) {
    float qr[D], acc[D];
    load_head(q + row * q_stride + h * D, qr);
    const float *kr = k + batch * tk * kv_stride + h * D;
    const float *vr = v + batch * tk * kv_stride + h * D;
    const Scores score{key_padding ? key_padding + batch * tk : nullptr, bias ? bias + (int64_t)qi * tk : nullptr, scale};
    float mx = -INFINITY;
    for (int t = 0; t < tk; ++t) {
      const float s = score(dot_head(qr, kr + t * kv_stride), t);
      mx = s > mx ? s : mx;
    }
    float sum = 0.0f;
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.0f;
    if (mx > -INFINITY) {
      for (int t = 0; t < tk; ++t) {
        const float p = expf(score(dot_head(qr, kr + t * kv_stride), t) - mx);
        sum = sum + p;
#pragma unroll
        for (int c = 0; c < D; ++c) acc[c] = acc[c] + p * vr[t * kv_stride + c];
      }
    }
    const bool dead = !(mx > -INFINITY);  // no admissible key
    float *o = out + (row * heads + h) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) o[c] = dead ? 0.0f : acc[c] / sum;
    if (lse) lse[(batch * heads + h) * tq + qi] = dead ? INFINITY : mx + logf(sum);
  });
}

// dq[q] = scale sum_t dS[q, t] k[t], dS = P (dout . v_t - delta), P = exp(s - lse); delta[b][h][q] = dout . out is left for
// the dK, dV kernel.
template <int D>
__global__ __launch_bounds__(kBlock) void attention_backward_q_kernel(
    const float *__restrict__ q, int64_t q_stride, const float *__restrict__ k, const float *__restrict__ v,
    int64_t kv_stride, const uint8_t *__restrict__ key_padding, const float *__restrict__ bias,
    const float *__restrict__ out, const float *__restrict__ lse, const float *__restrict__ dout, int64_t b, int tq, int tk,
    int heads, float scale, float *__restrict__ dq, int64_t dq_stride, float *__restrict__ delta) {
  for_each_head_row(b, tq, heads, [&](int64_t batch, int qi, int h, int64_t row) {
    float qr[D], g[D], acc[D];
    load_head(q + row * q_stride + h * D, qr);
    load_head(dout + (row * heads + h) * D, g);
    const float dl = dot_head(g, out + (row * heads + h) * D);
    const int64_t at = (batch * heads + h) * tq + qi;
    const float l = lse[at];
    delta[at] = dl;
    const float *kr = k + batch * tk * kv_stride + h * D;
    const float *vr = v + batch * tk * kv_stride + h * D;
    const Scores score{key_padding ? key_padding + batch * tk : nullptr, bias ? bias + (int64_t)qi * tk : nullptr, scale};
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.0f;
    for (int t = 0; t < tk; ++t) {
      const float p = expf(score(dot_head(qr, kr + t * kv_stride), t) - l);
      const float ds = p * (dot_head(g, vr + t * kv_stride) - dl);
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = acc[c] + ds * kr[t * kv_stride + c];
    }
    float *o = dq + row * dq_stride + h * D;
#pragma unroll
    for (int c = 0; c < D; ++c) o[c] = scale * acc[c];
  });
}

// dv[t] = sum_q P[q, t] dout[q], dk[t] = scale sum_q dS[q, t] q[q]: one lane per (b, t, h), the queries in ascending order.
template <int D>
__global__ __launch_bounds__(kBlock) void attention_backward_kv_kernel(
    const float *__restrict__ q, int64_t q_stride, const float *__restrict__ k, const float *__restrict__ v,
    int64_t kv_stride, const uint8_t *__restrict__ key_padding, const float *__restrict__ bias,
    const float *__restrict__ lse, const float *__restrict__ delta, const float *__restrict__ dout, int64_t b, int tq, int tk,
    int heads, float scale, float *__restrict__ dk, float *__restrict__ dv, int64_t dkv_stride) {
  for_each_head_row(b, tk, heads, [&](int64_t batch, int ti, int h, int64_t row) {
    float kr[D], vr[D], dka[D], dva[D];
    load_head(k + row * kv_stride + h * D, kr);
    load_head(v + row * kv_stride + h * D, vr);
    const bool padded = key_padding && key_padding[row];
    const float *qr = q + batch * tq * q_stride + h * D;
    const float *gr = dout + (batch * tq * heads + h) * D;
    const float *lr = lse + (batch * heads + h) * tq;
    const float *dr = delta + (batch * heads + h) * tq;
#pragma unroll
    for (int c = 0; c < D; ++c) dka[c] = dva[c] = 0.0f;
    for (int qi = 0; qi < tq; ++qi) {
      const float *qq = qr + qi * q_stride;
      const float *g = gr + (int64_t)qi * heads * D;
      float s = scale * dot_head(kr, qq);
      if (bias) s = s + bias[(int64_t)qi * tk + ti];
      const float p = expf((padded ? -INFINITY : s) - lr[qi]);
      const float ds = p * (dot_head(vr, g) - dr[qi]);
#pragma unroll
      for (int c = 0; c < D; ++c) {
        dva[c] = dva[c] + p * g[c];
        dka[c] = dka[c] + ds * qq[c];
      }
    }
    float *ok = dk + row * dkv_stride + h * D;
    float *ov = dv + row * dkv_stride + h * D;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      ok[c] = scale * dka[c];
      ov[c] = dva[c];
    }
  });
}

inline bool aligned_to(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// One instantiation per head width: f.template operator()<D>().
template <class F>
inline void with_head_width(int d, F &&f) {
  switch (d) {
#define RL8_HEAD_WIDTH(D) \
  case D:                 \
    f.template operator()<D>(); \
    break;
    RL8_HEAD_WIDTH(1) RL8_HEAD_WIDTH(2) RL8_HEAD_WIDTH(3) RL8_HEAD_WIDTH(4) RL8_HEAD_WIDTH(5) RL8_HEAD_WIDTH(6)
    RL8_HEAD_WIDTH(7) RL8_HEAD_WIDTH(8) RL8_HEAD_WIDTH(9) RL8_HEAD_WIDTH(10) RL8_HEAD_WIDTH(11) RL8_HEAD_WIDTH(12)
    RL8_HEAD_WIDTH(13) RL8_HEAD_WIDTH(14) RL8_HEAD_WIDTH(15) RL8_HEAD_WIDTH(16)
#undef RL8_HEAD_WIDTH
  }
}

struct ForwardLaunch {
  const float *q;
  int64_t q_stride;
  const float *k, *v;
  int64_t kv_stride;
  const uint8_t *key_padding;
  const float *bias;
  int64_t b;
  int tq, tk, heads;
  float scale;
  float *out, *lse;
  hipStream_t stream;
  template <int D>
  void operator()() const {
    attention_forward_kernel<D><<<grid_for(b * tq * heads, kBlock), kBlock, 0, stream>>>(
        q, q_stride, k, v, kv_stride, key_padding, bias, b, tq, tk, heads, scale, out, lse);
  }
};

struct BackwardLaunch {
  const float *q;
  int64_t q_stride;
  const float *k, *v;
  int64_t kv_stride;
  const uint8_t *key_padding;
  const float *bias, *out, *lse, *dout;
  int64_t b;
  int tq, tk, heads;
  float scale;
  float *dq;
  int64_t dq_stride;
  float *dk, *dv;
  int64_t dkv_stride;
  float *delta;
  hipStream_t stream;
  template <int D>
  void operator()() const {
    attention_backward_q_kernel<D><<<grid_for(b * tq * heads, kBlock), kBlock, 0, stream>>>(
        q, q_stride, k, v, kv_stride, key_padding, bias, out, lse, dout, b, tq, tk, heads, scale, dq, dq_stride, delta);
    attention_backward_kv_kernel<D><<<grid_for(b * tk * heads, kBlock), kBlock, 0, stream>>>(
        q, q_stride, k, v, kv_stride, key_padding, bias, lse, delta, dout, b, tq, tk, heads, scale, dk, dv, dkv_stride);
  }
};

}  // namespace
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_attention_supports(int tq, int tk, int heads, int d) {
  if (tq < 1 || tk < 1 || heads < 1 || d < 1) return RL8_ESIZE;
  return tq <= kMaxT && tk <= kMaxT && d <= kMaxD ? 1 : 0;
}

RL8_API int rl8_attention_f32(const float *q, int64_t q_stride, const float *k, const float *v, int64_t kv_stride,
                              const uint8_t *key_padding, const float *bias, int64_t b, int tq, int tk, int heads, int d,
                              float *out, float *lse, void *stream) {
  if (!q || !k || !v || !out) return RL8_ENULL;
  if (b < 1 || tq < 1 || tk < 1 || heads < 1 || d < 1) return RL8_ESIZE;
  if (q_stride < (int64_t)heads * d || kv_stride < (int64_t)heads * d) return RL8_ESIZE;
  if (!aligned_to(q, 4) || !aligned_to(k, 4) || !aligned_to(v, 4) || !aligned_to(bias, 4) || !aligned_to(out, 4) ||
      !aligned_to(lse, 4))
    return RL8_EALIGN;
  if (rl8_attention_supports(tq, tk, heads, d) != 1) return RL8_ECONFIG;
  with_head_width(d, ForwardLaunch{q, q_stride, k, v, kv_stride, key_padding, bias, b, tq, tk, heads,
                                   1.0f / sqrtf((float)d), out, lse, (hipStream_t)stream});
  return launch_status();
}

RL8_API int rl8_attention_backward_f32(const float *q, int64_t q_stride, const float *k, const float *v,
                                       int64_t kv_stride, const uint8_t *key_padding, const float *bias, const float *out,
                                       const float *lse, const float *dout, int64_t b, int tq, int tk, int heads, int d,
                                       float *dq, int64_t dq_stride, float *dk, float *dv, int64_t dkv_stride,
                                       float *delta_workspace, void *stream) {
  if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || !delta_workspace) return RL8_ENULL;
  if (b < 1 || tq < 1 || tk < 1 || heads < 1 || d < 1) return RL8_ESIZE;
  const int64_t e = (int64_t)heads * d;
  if (q_stride < e || kv_stride < e || dq_stride < e || dkv_stride < e) return RL8_ESIZE;
  if (!aligned_to(q, 4) || !aligned_to(k, 4) || !aligned_to(v, 4) || !aligned_to(bias, 4) || !aligned_to(out, 4) ||
      !aligned_to(lse, 4) || !aligned_to(dout, 4) || !aligned_to(dq, 4) || !aligned_to(dk, 4) || !aligned_to(dv, 4) ||
      !aligned_to(delta_workspace, 4))
    return RL8_EALIGN;
  if (rl8_attention_supports(tq, tk, heads, d) != 1) return RL8_ECONFIG;
  with_head_width(d, BackwardLaunch{q, q_stride, k, v, kv_stride, key_padding, bias, out, lse, dout, b, tq, tk, heads,
                                    1.0f / sqrtf((float)d), dq, dq_stride, dk, dv, dkv_stride, delta_workspace,
                                    (hipStream_t)stream});
  return launch_status();
}
