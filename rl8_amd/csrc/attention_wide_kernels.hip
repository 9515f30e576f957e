// Multihead attention's core on the matrix cores for what attention_kernels.hip leaves: 1 <= Tq, Tk <= 128 cells and
// heads of 1 <= D <= 64 floats, fp32, forward and backward.  Compiled with -ffp-contract=off.
//
// The operand contract is attention_kernels.hip's, clause for clause.  q rows [B][Tq] and k, v rows [B][Tk] each have a
// base pointer and a row stride in floats, head h of a row being the D floats at h D: a packed [B][T][3E] or
// [B][Tk][2E] projection is read, and its gradient written, in place.  Pointers are 4-byte aligned and no more (16-byte
// loads only behind a wave-uniform check of base, stride and D).  `key_padding` [B][Tk] bytes, NONZERO = PADDED;
// `bias` [Tq][Tk] is added to the scaled scores and may hold -inf; `out` [B][Tq][H][D] dense; `lse`, `delta`
// [B][H][Tq].  A query without an admissible key has P = 0: out = 0, lse = +inf, and exp(s - lse) = 0 carries that
// through both backward kernels, so it adds exactly nothing to dk and dv.
//
// The tile helpers (and the matrix instruction's operand layout) are in attention_tiles.hip.h, shared with
// attention_long_kernels.hip.
//
// Split.  One workgroup per (b, h, group of up to four 16-row strips), one wave per strip; the workgroup stages the
// head's other sequence into LDS once (forward and dQ: K and V, strips of queries; dK/dV: Q and dO, strips of keys), rows
// padded to a multiple of 16 and columns to 16 NF = the next multiple of 16 with zeros, NF a template parameter.  Row
// pitch 16 NF + 4 floats: pitch / 4 is odd, so both access patterns below touch 64 different banks.
//
// No transpose of P.  A wave forms the TRANSPOSED score tile S^T = K Q^T, keys along the accumulator's rows: lane l
// holds keys 16 tile + 4 (l / 16) + r of query l % 16.  Scale, bias, padding and the rows >= Tk are applied on the
// accumulators; a query's maximum and sum are reduced over r and the tiles in the lane, then over the four 16-lane
// groups by two xor exchanges (every lane of a query ends with the same bits: a + b is commutative).  Accumulator
// register r of a tile IS the B operand of O^T = V^T P^T for the four keys {16 tile + 4 g + r : g}, so the A operand is
// read from LDS in that permuted key order and the probabilities never leave the registers.  The backward kernels use
// the same trick: dQ^T = K^T dS^T from S^T and dP^T = V dO^T; dV^T = dO^T P and dK^T = Q^T dS from S = Q K^T.
//
// Every sum runs inside one wave in a fixed order: no atomics, no reduction across workgroups, the same bits on every
// run.
#include "attention_tiles.hip.h"

namespace rl8 {
namespace {

using namespace attention_tiles;

constexpr int kWideMaxT = 128;
constexpr int kWideMaxD = 64;
constexpr int kMaxTiles = kWideMaxT / kStrip;
constexpr int kMaxGridWide = 1 << 20;

// Floats of LDS of a kernel that stages two [t][16 NF] operands and 2 t words beside them (the forward and dQ use a
// quarter of the words: the padding bytes; dK/dV all of them: lse and delta).
inline int lds_bytes(int t, int nf) {
  const int tp = (t + kStrip - 1) / kStrip * kStrip;
  return (2 * tp * pitch_of(nf) + 2 * tp) * (int)sizeof(float);
}

template <int NF>
__global__ __launch_bounds__(kBlock) void attention_wide_forward_kernel(
    const float *__restrict__ q, int64_t q_stride, const float *__restrict__ k, const float *__restrict__ v,
    int64_t kv_stride, const uint8_t *__restrict__ key_padding, const float *__restrict__ bias, int64_t total, int groups,
    int tq, int tk, int heads, int d, float scale, float *__restrict__ out, float *__restrict__ lse) {
  constexpr int kPitch = pitch_of(NF);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, col = lane & 15, grp = lane >> 4;
  const int nt = (tk + kStrip - 1) / kStrip, tkp = nt * kStrip;
  float *ks = lds, *vs = lds + tkp * kPitch;
  uint32_t *pad = reinterpret_cast<uint32_t *>(vs + tkp * kPitch);
  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    const Item at(item, heads, groups);
    const int64_t kv0 = at.batch * tk * kv_stride + at.h * d;
    stage_rows<NF>(ks, k + kv0, kv_stride, tk, tkp, d);
    stage_rows<NF>(vs, v + kv0, kv_stride, tk, tkp, d);
    stage_padding(pad, key_padding ? key_padding + at.batch * tk : nullptr, tk, tkp);
    __syncthreads();
    const int qi = (at.first_strip + wave) * kStrip + col;
    if (qi - col < tq) {  // (wave-uniform: the strip exists)
      const bool live = qi < tq;
      const int64_t row = at.batch * tq + (live ? qi : 0);
      float qf[4 * NF];
      load_fragment<NF>(q + row * q_stride + at.h * d, live, grp, d, qf);
      const float *bias_row = bias ? bias + (int64_t)(live ? qi : 0) * tk : nullptr;
      f32x4 s[kMaxTiles];
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < kMaxTiles; ++t) {
        if (t < nt) {
          s[t] = finish_scores(rows_times_fragment<NF>(ks + (16 * t + col) * kPitch + grp, qf), scale, bias_row, live,
                               16 * t + 4 * grp, tk, pad[4 * t + grp]);
#pragma unroll
          for (int r = 0; r < 4; ++r) mx = s[t][r] > mx ? s[t][r] : mx;
        }
      }
      mx = across_groups_max(mx);
      const bool dead = !(mx > -INFINITY);  // no admissible key: never (-inf) - (-inf)
      const float base = dead ? 0.0f : mx;
      float sum = 0.0f;
      f32x4 o[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) o[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < kMaxTiles; ++t) {
        if (t < nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            s[t][r] = expf(s[t][r] - base);
            sum = sum + s[t][r];
          }
          transposed_times_tile<NF>(vs + (16 * t + 4 * grp) * kPitch + col, s[t], o);
        }
      }
      sum = across_groups_sum(sum);
      if (live) {
        float *orow = out + (row * heads + at.h) * d;
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = 16 * f + 4 * grp + r;
            if (c < d) orow[c] = dead ? 0.0f : o[f][r] / sum;
          }
        if (lse && grp == 0) lse[(at.batch * heads + at.h) * tq + qi] = dead ? INFINITY : mx + logf(sum);
      }
    }
    __syncthreads();  // (the next item stages over what this one reads)
  }
}

// dq[q] = scale sum_t dS[q, t] k[t], dS = P (dout . v_t - delta), P = exp(s - lse); delta[b][h][q] = dout . out is left for
// the dK, dV kernel.  One key tile at a time: S^T and dP^T of the tile, dS^T, and dQ^T += K^T dS^T.
template <int NF>
__global__ __launch_bounds__(kBlock) void attention_wide_backward_q_kernel(
    const float *__restrict__ q, int64_t q_stride, const float *__restrict__ k, const float *__restrict__ v,
    int64_t kv_stride, const uint8_t *__restrict__ key_padding, const float *__restrict__ bias,
    const float *__restrict__ out, const float *__restrict__ lse, const float *__restrict__ dout, int64_t total, int groups,
    int tq, int tk, int heads, int d, float scale, float *__restrict__ dq, int64_t dq_stride, float *__restrict__ delta) {
  constexpr int kPitch = pitch_of(NF);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, col = lane & 15, grp = lane >> 4;
  const int nt = (tk + kStrip - 1) / kStrip, tkp = nt * kStrip;
  float *ks = lds, *vs = lds + tkp * kPitch;
  uint32_t *pad = reinterpret_cast<uint32_t *>(vs + tkp * kPitch);
  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    const Item at(item, heads, groups);
    const int64_t kv0 = at.batch * tk * kv_stride + at.h * d;
    stage_rows<NF>(ks, k + kv0, kv_stride, tk, tkp, d);
    stage_rows<NF>(vs, v + kv0, kv_stride, tk, tkp, d);
    stage_padding(pad, key_padding ? key_padding + at.batch * tk : nullptr, tk, tkp);
    __syncthreads();
    const int qi = (at.first_strip + wave) * kStrip + col;
    if (qi - col < tq) {
      const bool live = qi < tq;
      const int64_t row = at.batch * tq + (live ? qi : 0);
      float qf[4 * NF], gf[4 * NF];
      load_fragment<NF>(q + row * q_stride + at.h * d, live, grp, d, qf);
      load_fragment<NF>(dout + (row * heads + at.h) * d, live, grp, d, gf);
      // delta = dout . out on the matrix cores too: see diagonal_dot().
      float of[4 * NF];
      load_fragment<NF>(out + (row * heads + at.h) * d, live, grp, d, of);
      const float dl = diagonal_dot<NF>(of, gf, col);
      const int64_t stat = (at.batch * heads + at.h) * tq + qi;
      const float l = live ? lse[stat] : INFINITY;  // (a column past Tq: P = 0)
      if (live && grp == 0) delta[stat] = dl;
      const float *bias_row = bias ? bias + (int64_t)(live ? qi : 0) * tk : nullptr;
      f32x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      for (int t = 0; t < nt; ++t) {
        const int lane_row = (16 * t + col) * kPitch + grp;
        const f32x4 s = finish_scores(rows_times_fragment<NF>(ks + lane_row, qf), scale, bias_row, live, 16 * t + 4 * grp,
                                      tk, pad[4 * t + grp]);
        const f32x4 dp = rows_times_fragment<NF>(vs + lane_row, gf);
        f32x4 ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) ds[r] = expf(s[r] - l) * (dp[r] - dl);
        transposed_times_tile<NF>(ks + (16 * t + 4 * grp) * kPitch + col, ds, acc);
      }
      if (live) {
        float *orow = dq + row * dq_stride + at.h * d;
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = 16 * f + 4 * grp + r;
            if (c < d) orow[c] = scale * acc[f][r];
          }
      }
    }
    __syncthreads();
  }
}

// dv[t] = sum_q P[q, t] dout[q], dk[t] = scale sum_q dS[q, t] q[q]: strips of KEYS, Q and dO (and lse, delta) in LDS, one
// query tile at a time with the queries along the accumulator's rows: S = Q K^T, dP = dO V^T, then dV^T += dO^T P and
// dK^T += Q^T dS.  Rows >= Tq have lse = +inf, so P = 0 there.
template <int NF>
__global__ __launch_bounds__(kBlock) void attention_wide_backward_kv_kernel(
    const float *__restrict__ q, int64_t q_stride, const float *__restrict__ k, const float *__restrict__ v,
    int64_t kv_stride, const uint8_t *__restrict__ key_padding, const float *__restrict__ bias,
    const float *__restrict__ lse, const float *__restrict__ delta, const float *__restrict__ dout, int64_t total,
    int groups, int tq, int tk, int heads, int d, float scale, float *__restrict__ dk, float *__restrict__ dv,
    int64_t dkv_stride) {
  constexpr int kPitch = pitch_of(NF);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, col = lane & 15, grp = lane >> 4;
  const int nt = (tq + kStrip - 1) / kStrip, tqp = nt * kStrip;
  float *qs = lds, *gs = lds + tqp * kPitch, *ls = gs + tqp * kPitch, *ds_ = ls + tqp;
  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    const Item at(item, heads, groups);
    stage_rows<NF>(qs, q + at.batch * tq * q_stride + at.h * d, q_stride, tq, tqp, d);
    stage_rows<NF>(gs, dout + (at.batch * tq * heads + at.h) * d, (int64_t)heads * d, tq, tqp, d);
    for (int i = threadIdx.x; i < tqp; i += blockDim.x) {
      const int64_t stat = (at.batch * heads + at.h) * tq + i;
      ls[i] = i < tq ? lse[stat] : INFINITY;
      ds_[i] = i < tq ? delta[stat] : 0.0f;
    }
    __syncthreads();
    const int ki = (at.first_strip + wave) * kStrip + col;
    if (ki - col < tk) {
      const bool live = ki < tk;
      const int64_t row = at.batch * tk + (live ? ki : 0);
      float kf[4 * NF], vf[4 * NF];
      load_fragment<NF>(k + row * kv_stride + at.h * d, live, grp, d, kf);
      load_fragment<NF>(v + row * kv_stride + at.h * d, live, grp, d, vf);
      const bool padded = !live || (key_padding && key_padding[row]);
      f32x4 dka[NF], dva[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) dka[f] = dva[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      for (int t = 0; t < nt; ++t) {
        const int lane_row = (16 * t + col) * kPitch + grp;
        const f32x4 s = rows_times_fragment<NF>(qs + lane_row, kf);
        const f32x4 dp = rows_times_fragment<NF>(gs + lane_row, vf);
        f32x4 p, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qi = 16 * t + 4 * grp + r;
          float x = scale * s[r];
          if (bias) x = x + ((live && qi < tq) ? bias[(int64_t)qi * tk + ki] : 0.0f);
          p[r] = expf((padded ? -INFINITY : x) - ls[qi]);
          ds[r] = p[r] * (dp[r] - ds_[qi]);
        }
        const int perm = (16 * t + 4 * grp) * kPitch + col;
        transposed_times_tile<NF>(gs + perm, p, dva);
        transposed_times_tile<NF>(qs + perm, ds, dka);
      }
      if (live) {
        float *ok = dk + row * dkv_stride + at.h * d;
        float *ov = dv + row * dkv_stride + at.h * d;
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = 16 * f + 4 * grp + r;
            if (c < d) {
              ok[c] = scale * dka[f][r];
              ov[c] = dva[f][r];
            }
          }
      }
    }
    __syncthreads();
  }
}

// Workgroups and their size over strips of `t` rows: groups of up to four strips, one wave per strip.
struct Split {
  int groups, block;
  int64_t total;
  int grid;
  Split(int64_t b, int heads, int t) {
    const int strips = (t + kStrip - 1) / kStrip;
    groups = (strips + 3) / 4;
    block = kWave * (strips < 4 ? strips : 4);
    total = b * heads * groups;
    grid = (int)(total < kMaxGridWide ? total : kMaxGridWide);
  }
};

struct WideForwardLaunch {
  const float *q;
  int64_t q_stride;
  const float *k, *v;
  int64_t kv_stride;
  const uint8_t *key_padding;
  const float *bias;
  int64_t b;
  int tq, tk, heads, d;
  float scale;
  float *out, *lse;
  hipStream_t stream;
  template <int NF>
  int operator()() const {
    const int bytes = lds_bytes(tk, NF);
    if (const int e = allow_dynamic_lds<&attention_wide_forward_kernel<NF>>(lds_bytes(kWideMaxT, NF))) return e;
    const Split s(b, heads, tq);
    attention_wide_forward_kernel<NF><<<s.grid, s.block, bytes, stream>>>(
        q, q_stride, k, v, kv_stride, key_padding, bias, s.total, s.groups, tq, tk, heads, d, scale, out, lse);
    return launch_status();
  }
};

struct WideBackwardLaunch {
  const float *q;
  int64_t q_stride;
  const float *k, *v;
  int64_t kv_stride;
  const uint8_t *key_padding;
  const float *bias, *out, *lse, *dout;
  int64_t b;
  int tq, tk, heads, d;
  float scale;
  float *dq;
  int64_t dq_stride;
  float *dk, *dv;
  int64_t dkv_stride;
  float *delta;
  hipStream_t stream;
  template <int NF>
  int operator()() const {
    if (const int e = allow_dynamic_lds<&attention_wide_backward_q_kernel<NF>>(lds_bytes(kWideMaxT, NF))) return e;
    if (const int e = allow_dynamic_lds<&attention_wide_backward_kv_kernel<NF>>(lds_bytes(kWideMaxT, NF))) return e;
    const Split sq(b, heads, tq), sk(b, heads, tk);
    attention_wide_backward_q_kernel<NF><<<sq.grid, sq.block, lds_bytes(tk, NF), stream>>>(
        q, q_stride, k, v, kv_stride, key_padding, bias, out, lse, dout, sq.total, sq.groups, tq, tk, heads, d, scale, dq,
        dq_stride, delta);
    attention_wide_backward_kv_kernel<NF><<<sk.grid, sk.block, lds_bytes(tq, NF), stream>>>(
        q, q_stride, k, v, kv_stride, key_padding, bias, lse, delta, dout, sk.total, sk.groups, tq, tk, heads, d, scale,
        dk, dv, dkv_stride);
    return launch_status();
  }
};

}  // namespace
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_attention_wide_supports(int tq, int tk, int heads, int d) {
  if (tq < 1 || tk < 1 || heads < 1 || d < 1) return RL8_ESIZE;
  return tq <= kWideMaxT && tk <= kWideMaxT && d <= kWideMaxD ? 1 : 0;
}

RL8_API int rl8_attention_wide_f32(const float *q, int64_t q_stride, const float *k, const float *v, int64_t kv_stride,
                                   const uint8_t *key_padding, const float *bias, int64_t b, int tq, int tk, int heads,
                                   int d, float *out, float *lse, void *stream) {
  if (!q || !k || !v || !out) return RL8_ENULL;
  if (b < 1 || tq < 1 || tk < 1 || heads < 1 || d < 1) return RL8_ESIZE;
  if (q_stride < (int64_t)heads * d || kv_stride < (int64_t)heads * d) return RL8_ESIZE;
  if (!aligned_to(q, 4) || !aligned_to(k, 4) || !aligned_to(v, 4) || !aligned_to(bias, 4) || !aligned_to(out, 4) ||
      !aligned_to(lse, 4))
    return RL8_EALIGN;
  if (rl8_attention_wide_supports(tq, tk, heads, d) != 1) return RL8_ECONFIG;
  return with_feature_tiles(d, WideForwardLaunch{q, q_stride, k, v, kv_stride, key_padding, bias, b, tq, tk, heads, d,
                                                 1.0f / sqrtf((float)d), out, lse, (hipStream_t)stream});
}

RL8_API int rl8_attention_wide_backward_f32(const float *q, int64_t q_stride, const float *k, const float *v,
                                            int64_t kv_stride, const uint8_t *key_padding, const float *bias,
                                            const float *out, const float *lse, const float *dout, int64_t b, int tq,
                                            int tk, int heads, int d, float *dq, int64_t dq_stride, float *dk, float *dv,
                                            int64_t dkv_stride, float *delta_workspace, void *stream) {
  if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || !delta_workspace) return RL8_ENULL;
  if (b < 1 || tq < 1 || tk < 1 || heads < 1 || d < 1) return RL8_ESIZE;
  const int64_t e = (int64_t)heads * d;
  if (q_stride < e || kv_stride < e || dq_stride < e || dkv_stride < e) return RL8_ESIZE;
  if (!aligned_to(q, 4) || !aligned_to(k, 4) || !aligned_to(v, 4) || !aligned_to(bias, 4) || !aligned_to(out, 4) ||
      !aligned_to(lse, 4) || !aligned_to(dout, 4) || !aligned_to(dq, 4) || !aligned_to(dk, 4) || !aligned_to(dv, 4) ||
      !aligned_to(delta_workspace, 4))
    return RL8_EALIGN;
  if (rl8_attention_wide_supports(tq, tk, heads, d) != 1) return RL8_ECONFIG;
  return with_feature_tiles(d, WideBackwardLaunch{q, q_stride, k, v, kv_stride, key_padding, bias, out, lse, dout, b, tq,
                                                  tk, heads, d, 1.0f / sqrtf((float)d), dq, dq_stride, dk, dv,
                                                  dkv_stride, delta_workspace, (hipStream_t)stream});
}
