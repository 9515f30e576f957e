// Multihead attention's core on the matrix cores for long sequences: 1 <= Tq, Tk <= 2048 cells and heads of
// 1 <= D <= 64 floats, fp32, forward and backward.  Compiled with -ffp-contract=off.
//
// The operand contract is attention_wide_kernels.hip's, clause for clause (strides, 4-byte alignment, `key_padding`
// NONZERO = PADDED, `bias` with -inf, `out` dense, `lse` and `delta` [B][H][Tq], a query without an admissible key:
// out = 0, lse = +inf, gradient 0 and exactly nothing added to dk and dv).  The tile helpers, the transposed-score
// layout (S^T = K Q^T, lane l owning query l % 16, a tile's accumulators being the B operand of the second product) and
// the LDS row pitch 16 NF + 4 are attention_tiles.hip.h's.
//
// What differs is that nothing of size Tq Tk or T is held.  The OTHER sequence of a head streams through LDS in chunks
// of 64 rows = four 16-row tiles, two buffers per operand: the global loads of chunk c + 1 are issued into registers
// before the products of chunk c and written to the other buffer after them, one barrier per chunk.  LDS use is
// (256 (16 NF + 4) + 256) floats whatever the lengths: 70656 bytes at NF = 4.
//
// Forward.  One workgroup of four waves per (b, h, group of query strips); a wave keeps its query column's running
// maximum m, the lane's part of the running sum l, and O^T in NF accumulators.  Every accumulator element of a lane
// belongs to the lane's query, so the rescale by exp(m_old - m_new) is one multiply per register.  The exponent's base
// is m_new where that is finite and 0 where it is still -inf: (-inf) - (-inf) never forms, a chunk, a first chunk or
// every chunk without an admissible key leaves m = -inf, l = 0, O = 0.
//
// Few strips.  The four waves are S strips x (4 / S) key lanes, S = 1, 2 or 4 from the count of strips.  Key lane j
// takes tiles j, j + 4 / S, ... of every chunk (not whole chunks: the stream and the LDS stay those of one chunk, and
// the lanes meet every barrier with equal work).  The lanes' partial (m, l, O^T) are merged through LDS by lane 0 in
// lane order; a lane that saw only dead keys has m = -inf and its weight exp(-inf - base) = 0.
//
// dQ: the same split and stream, no running softmax (lse is known), dQ^T in accumulators across all chunks, the lanes'
// parts added by lane 0 in lane order; delta = dout . out by diagonal_dot().  dK/dV: strips of KEYS, chunks of 64
// queries of Q, dO, lse and delta; dK^T and dV^T in accumulators, the same lane split over the query tiles.
//
// Every sum runs in a fixed order inside one workgroup: no atomics, the same bits on every run.
#include "attention_tiles.hip.h"

namespace rl8 {
namespace {

using namespace attention_tiles;

constexpr int kLongMaxT = 2048;
constexpr int kLongMaxD = 64;
constexpr int kChunk = 64;  // rows of the streamed sequence per LDS buffer: four tiles
constexpr int kMaxGridLong = 1 << 20;

// Two operands x two buffers of a chunk, and 2 x 128 words beside them (padding words; lse and delta).
constexpr int lds_floats(int nf) { return 4 * kChunk * pitch_of(nf) + 4 * kChunk; }

// A workgroup's part of one chunk of an operand in registers: slot i of thread t is the four floats at row
// (t + 256 i) / (4 NF), column 4 ((t + 256 i) % (4 NF)); zeros past `rows` and `d`.
template <int NF>
__device__ __forceinline__ void fetch_chunk(f32x4 (&x)[NF], const float *__restrict__ src, int64_t stride, int rows, int d,
                                            bool vec) {
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int idx = (int)threadIdx.x + kBlock * i, r = idx / (4 * NF), c = 4 * (idx - r * (4 * NF));
    x[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (r < rows) {
      const float *p = src + r * stride + c;
      if (vec) {
        if (c < d) x[i] = *reinterpret_cast<const f32x4 *>(p);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c + j < d) x[i][j] = p[j];
      }
    }
  }
}

template <int NF>
__device__ __forceinline__ void store_chunk(float *__restrict__ dst, const f32x4 (&x)[NF]) {
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int idx = (int)threadIdx.x + kBlock * i, r = idx / (4 * NF), c = 4 * (idx - r * (4 * NF));
    *reinterpret_cast<f32x4 *>(dst + r * pitch_of(NF) + c) = x[i];
  }
}

// Whether a base pointer, its row stride and D allow 16-byte loads (wave-uniform).
__device__ __forceinline__ bool vector_rows(const float *p, int64_t stride, int d) {
  return aligned16_dev(p) && (stride & 3) == 0 && (d & 3) == 0;
}

// The waves of a workgroup as `split` strips x 4 / split lanes over the tiles of a chunk.
struct Waves {
  int lanes, strip, lane;
  __device__ __forceinline__ Waves(int wave, int split) : lanes(4 / split), strip(wave % split), lane(wave / split) {}
  __device__ __forceinline__ bool takes(int tile) const { return (tile & (lanes - 1)) == lane; }
};

// Where wave `wave` (of a key lane > 0) leaves value i of its lanes for the merge: behind each other per lane.
__device__ __forceinline__ int merge_slot(int wave, int split, int values, int i, int lane) {
  return ((wave - split) * values + i) * kWave + lane;
}

template <int NF>
__global__ __launch_bounds__(kBlock) void attention_long_forward_kernel(
    const float *__restrict__ q, int64_t q_stride, const float *__restrict__ k, const float *__restrict__ v,
    int64_t kv_stride, const uint8_t *__restrict__ key_padding, const float *__restrict__ bias, int64_t total, int groups,
    int split, int tq, int tk, int heads, int d, float scale, float *__restrict__ out, float *__restrict__ lse) {
  constexpr int kPitch = pitch_of(NF), kBuf = kChunk * kPitch, kValues = 2 + 4 * NF;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, col = lane & 15, grp = lane >> 4;
  const Waves my(wave, split);
  float *kbuf = lds, *vbuf = lds + 2 * kBuf;
  uint32_t *pad = reinterpret_cast<uint32_t *>(lds + 4 * kBuf);  // [2][16]
  const int nc = (tk + kChunk - 1) / kChunk;
  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    const Item at(item, heads, groups, split);
    const float *kbase = k + at.batch * tk * kv_stride + at.h * d, *vbase = v + at.batch * tk * kv_stride + at.h * d;
    const uint8_t *padded = key_padding ? key_padding + at.batch * tk : nullptr;
    const bool vec = vector_rows(kbase, kv_stride, d) && aligned16_dev(vbase);
    f32x4 kx[NF], vx[NF];
    uint32_t pw = 0;
    fetch_chunk<NF>(kx, kbase, kv_stride, tk, d, vec);
    fetch_chunk<NF>(vx, vbase, kv_stride, tk, d, vec);
    if (threadIdx.x < 16) pw = padding_word(padded, threadIdx.x, tk);
    store_chunk<NF>(kbuf, kx);
    store_chunk<NF>(vbuf, vx);
    if (threadIdx.x < 16) pad[threadIdx.x] = pw;
    __syncthreads();
    const int qi = (at.first_strip + my.strip) * kStrip + col;
    const bool active = qi - col < tq, live = qi < tq;  // (active: wave-uniform, the strip exists)
    const int64_t row = at.batch * tq + (live ? qi : 0);
    float qf[4 * NF];
    load_fragment<NF>(q + row * q_stride + at.h * d, live, grp, d, qf);
    const float *bias_row = bias ? bias + (int64_t)(live ? qi : 0) * tk : nullptr;
    float m = -INFINITY, l = 0.0f;
    f32x4 o[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) o[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < nc; ++c) {
      const bool more = c + 1 < nc;
      const int key1 = kChunk * (c + 1);
      if (more) {
        fetch_chunk<NF>(kx, kbase + key1 * kv_stride, kv_stride, tk - key1, d, vec);
        fetch_chunk<NF>(vx, vbase + key1 * kv_stride, kv_stride, tk - key1, d, vec);
        if (threadIdx.x < 16) pw = padding_word(padded, key1 / 4 + threadIdx.x, tk);
      }
      if (active) {
        const float *kb = kbuf + (c & 1) * kBuf, *vb = vbuf + (c & 1) * kBuf;
        const uint32_t *pb = pad + (c & 1) * 16;
        f32x4 s[4];
        float cm = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (my.takes(t) && kChunk * c + 16 * t < tk) {
            s[t] = finish_scores(rows_times_fragment<NF>(kb + (16 * t + col) * kPitch + grp, qf), scale, bias_row, live,
                                 kChunk * c + 16 * t + 4 * grp, tk, pb[4 * t + grp]);
#pragma unroll
            for (int r = 0; r < 4; ++r) cm = s[t][r] > cm ? s[t][r] : cm;
          }
        }
        cm = across_groups_max(cm);
        const float m_new = cm > m ? cm : m;
        const float base = m_new > -INFINITY ? m_new : 0.0f;  // finite: never (-inf) - (-inf)
        const float alpha = expf(m - base);
        m = m_new;
        l = l * alpha;
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) o[f][r] = o[f][r] * alpha;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (my.takes(t) && kChunk * c + 16 * t < tk) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              s[t][r] = expf(s[t][r] - base);
              l = l + s[t][r];
            }
            transposed_times_tile<NF>(vb + (16 * t + 4 * grp) * kPitch + col, s[t], o);
          }
        }
      }
      if (more) {
        store_chunk<NF>(kbuf + ((c + 1) & 1) * kBuf, kx);
        store_chunk<NF>(vbuf + ((c + 1) & 1) * kBuf, vx);
        if (threadIdx.x < 16) pad[((c + 1) & 1) * 16 + threadIdx.x] = pw;
      }
      __syncthreads();
    }
    l = across_groups_sum(l);
    if (my.lanes > 1) {  // (workgroup-uniform) the key lanes' parts, merged by lane 0 in lane order over the K buffers
      if (my.lane > 0) {
        lds[merge_slot(wave, split, kValues, 0, lane)] = m;
        lds[merge_slot(wave, split, kValues, 1, lane)] = l;
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) lds[merge_slot(wave, split, kValues, 2 + 4 * f + r, lane)] = o[f][r];
      }
      __syncthreads();
      if (my.lane == 0) {
        for (int j = 1; j < my.lanes; ++j) {
          const int from = j * split + my.strip;
          const float mj = lds[merge_slot(from, split, kValues, 0, lane)];
          const float lj = lds[merge_slot(from, split, kValues, 1, lane)];
          const float m_new = mj > m ? mj : m;
          const float base = m_new > -INFINITY ? m_new : 0.0f;
          const float a = expf(m - base), bj = expf(mj - base);
          m = m_new;
          l = l * a + lj * bj;
#pragma unroll
          for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              o[f][r] = o[f][r] * a + lds[merge_slot(from, split, kValues, 2 + 4 * f + r, lane)] * bj;
        }
      }
      __syncthreads();  // (the next item stages over what lane 0 reads)
    }
    if (active && live && my.lane == 0) {
      const bool dead = !(m > -INFINITY);
      float *orow = out + (row * heads + at.h) * d;
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int cc = 16 * f + 4 * grp + r;
          if (cc < d) orow[cc] = dead ? 0.0f : o[f][r] / l;
        }
      if (lse && grp == 0) lse[(at.batch * heads + at.h) * tq + qi] = dead ? INFINITY : m + logf(l);
    }
  }
}

// dq[q] = scale sum_t dS[q, t] k[t], dS = P (dout . v_t - delta), P = exp(s - lse); delta[b][h][q] = dout . out is left for
// the dK, dV kernel.
template <int NF>
__global__ __launch_bounds__(kBlock) void attention_long_backward_q_kernel(
    const float *__restrict__ q, int64_t q_stride, const float *__restrict__ k, const float *__restrict__ v,
    int64_t kv_stride, const uint8_t *__restrict__ key_padding, const float *__restrict__ bias,
    const float *__restrict__ out, const float *__restrict__ lse, const float *__restrict__ dout, int64_t total, int groups,
    int split, int tq, int tk, int heads, int d, float scale, float *__restrict__ dq, int64_t dq_stride,
    float *__restrict__ delta) {
  constexpr int kPitch = pitch_of(NF), kBuf = kChunk * kPitch, kValues = 4 * NF;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, col = lane & 15, grp = lane >> 4;
  const Waves my(wave, split);
  float *kbuf = lds, *vbuf = lds + 2 * kBuf;
  uint32_t *pad = reinterpret_cast<uint32_t *>(lds + 4 * kBuf);
  const int nc = (tk + kChunk - 1) / kChunk;
  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    const Item at(item, heads, groups, split);
    const float *kbase = k + at.batch * tk * kv_stride + at.h * d, *vbase = v + at.batch * tk * kv_stride + at.h * d;
    const uint8_t *padded = key_padding ? key_padding + at.batch * tk : nullptr;
    const bool vec = vector_rows(kbase, kv_stride, d) && aligned16_dev(vbase);
    f32x4 kx[NF], vx[NF];
    uint32_t pw = 0;
    fetch_chunk<NF>(kx, kbase, kv_stride, tk, d, vec);
    fetch_chunk<NF>(vx, vbase, kv_stride, tk, d, vec);
    if (threadIdx.x < 16) pw = padding_word(padded, threadIdx.x, tk);
    store_chunk<NF>(kbuf, kx);
    store_chunk<NF>(vbuf, vx);
    if (threadIdx.x < 16) pad[threadIdx.x] = pw;
    __syncthreads();
    const int qi = (at.first_strip + my.strip) * kStrip + col;
    const bool active = qi - col < tq, live = qi < tq;
    const int64_t row = at.batch * tq + (live ? qi : 0);
    float qf[4 * NF], gf[4 * NF];
    load_fragment<NF>(q + row * q_stride + at.h * d, live, grp, d, qf);
    load_fragment<NF>(dout + (row * heads + at.h) * d, live, grp, d, gf);
    float dl;
    {
      float of[4 * NF];
      load_fragment<NF>(out + (row * heads + at.h) * d, live, grp, d, of);
      dl = diagonal_dot<NF>(of, gf, col);
    }
    const int64_t stat = (at.batch * heads + at.h) * tq + (live ? qi : 0);
    const float ls = live ? lse[stat] : INFINITY;  // (a column past Tq: P = 0)
    if (active && live && my.lane == 0 && grp == 0) delta[stat] = dl;
    const float *bias_row = bias ? bias + (int64_t)(live ? qi : 0) * tk : nullptr;
    f32x4 acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < nc; ++c) {
      const bool more = c + 1 < nc;
      const int key1 = kChunk * (c + 1);
      if (more) {
        fetch_chunk<NF>(kx, kbase + key1 * kv_stride, kv_stride, tk - key1, d, vec);
        fetch_chunk<NF>(vx, vbase + key1 * kv_stride, kv_stride, tk - key1, d, vec);
        if (threadIdx.x < 16) pw = padding_word(padded, key1 / 4 + threadIdx.x, tk);
      }
      if (active) {
        const float *kb = kbuf + (c & 1) * kBuf, *vb = vbuf + (c & 1) * kBuf;
        const uint32_t *pb = pad + (c & 1) * 16;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (my.takes(t) && kChunk * c + 16 * t < tk) {
            const int lane_row = (16 * t + col) * kPitch + grp;
            const f32x4 s = finish_scores(rows_times_fragment<NF>(kb + lane_row, qf), scale, bias_row, live,
                                          kChunk * c + 16 * t + 4 * grp, tk, pb[4 * t + grp]);
            const f32x4 dp = rows_times_fragment<NF>(vb + lane_row, gf);
            f32x4 ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) ds[r] = expf(s[r] - ls) * (dp[r] - dl);
            transposed_times_tile<NF>(kb + (16 * t + 4 * grp) * kPitch + col, ds, acc);
          }
        }
      }
      if (more) {
        store_chunk<NF>(kbuf + ((c + 1) & 1) * kBuf, kx);
        store_chunk<NF>(vbuf + ((c + 1) & 1) * kBuf, vx);
        if (threadIdx.x < 16) pad[((c + 1) & 1) * 16 + threadIdx.x] = pw;
      }
      __syncthreads();
    }
    if (my.lanes > 1) {
      if (my.lane > 0) {
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) lds[merge_slot(wave, split, kValues, 4 * f + r, lane)] = acc[f][r];
      }
      __syncthreads();
      if (my.lane == 0) {
        for (int j = 1; j < my.lanes; ++j)
#pragma unroll
          for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              acc[f][r] = acc[f][r] + lds[merge_slot(j * split + my.strip, split, kValues, 4 * f + r, lane)];
      }
      __syncthreads();
    }
    if (active && live && my.lane == 0) {
      float *orow = dq + row * dq_stride + at.h * d;
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int cc = 16 * f + 4 * grp + r;
          if (cc < d) orow[cc] = scale * acc[f][r];
        }
    }
  }
}

// dv[t] = sum_q P[q, t] dout[q], dk[t] = scale sum_q dS[q, t] q[q]: strips of KEYS; Q, dO, lse and delta stream through
// LDS in chunks of 64 queries, the queries along the accumulator's rows: S = Q K^T, dP = dO V^T, then dV^T += dO^T P and
// dK^T += Q^T dS.  Rows >= Tq are staged with lse = +inf, so P = 0 there.
template <int NF>
__global__ __launch_bounds__(kBlock) void attention_long_backward_kv_kernel(
    const float *__restrict__ q, int64_t q_stride, const float *__restrict__ k, const float *__restrict__ v,
    int64_t kv_stride, const uint8_t *__restrict__ key_padding, const float *__restrict__ bias,
    const float *__restrict__ lse, const float *__restrict__ delta, const float *__restrict__ dout, int64_t total,
    int groups, int split, int tq, int tk, int heads, int d, float scale, float *__restrict__ dk, float *__restrict__ dv,
    int64_t dkv_stride) {
  constexpr int kPitch = pitch_of(NF), kBuf = kChunk * kPitch, kValues = 8 * NF;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, col = lane & 15, grp = lane >> 4;
  const Waves my(wave, split);
  float *qbuf = lds, *gbuf = lds + 2 * kBuf, *stats = lds + 4 * kBuf;  // stats [2][lse 64 | delta 64]
  const int nc = (tq + kChunk - 1) / kChunk;
  const int64_t g_stride = (int64_t)heads * d;
  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    const Item at(item, heads, groups, split);
    const float *qbase = q + at.batch * tq * q_stride + at.h * d, *gbase = dout + (at.batch * tq * heads + at.h) * d;
    const float *stat_base = (threadIdx.x < kChunk ? lse : delta) + (at.batch * heads + at.h) * tq;
    const int stat_row = threadIdx.x & (kChunk - 1);
    const float stat_dead = threadIdx.x < kChunk ? INFINITY : 0.0f;
    const bool qvec = vector_rows(qbase, q_stride, d), gvec = vector_rows(gbase, g_stride, d);
    f32x4 qx[NF], gx[NF];
    float sx = 0.0f;
    fetch_chunk<NF>(qx, qbase, q_stride, tq, d, qvec);
    fetch_chunk<NF>(gx, gbase, g_stride, tq, d, gvec);
    if (threadIdx.x < 2 * kChunk) sx = stat_row < tq ? stat_base[stat_row] : stat_dead;
    store_chunk<NF>(qbuf, qx);
    store_chunk<NF>(gbuf, gx);
    if (threadIdx.x < 2 * kChunk) stats[threadIdx.x] = sx;
    __syncthreads();
    const int ki = (at.first_strip + my.strip) * kStrip + col;
    const bool active = ki - col < tk, live = ki < tk;
    const int64_t row = at.batch * tk + (live ? ki : 0);
    float kf[4 * NF], vf[4 * NF];
    load_fragment<NF>(k + row * kv_stride + at.h * d, live, grp, d, kf);
    load_fragment<NF>(v + row * kv_stride + at.h * d, live, grp, d, vf);
    const bool padded = !live || (key_padding && key_padding[row]);
    f32x4 dka[NF], dva[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) dka[f] = dva[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < nc; ++c) {
      const bool more = c + 1 < nc;
      const int q1 = kChunk * (c + 1);
      if (more) {
        fetch_chunk<NF>(qx, qbase + q1 * q_stride, q_stride, tq - q1, d, qvec);
        fetch_chunk<NF>(gx, gbase + q1 * g_stride, g_stride, tq - q1, d, gvec);
        if (threadIdx.x < 2 * kChunk) sx = q1 + stat_row < tq ? stat_base[q1 + stat_row] : stat_dead;
      }
      if (active) {
        const float *qb = qbuf + (c & 1) * kBuf, *gb = gbuf + (c & 1) * kBuf;
        const float *lsb = stats + (c & 1) * 2 * kChunk, *dlb = lsb + kChunk;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (my.takes(t) && kChunk * c + 16 * t < tq) {
            const int lane_row = (16 * t + col) * kPitch + grp;
            const f32x4 s = rows_times_fragment<NF>(qb + lane_row, kf);
            const f32x4 dp = rows_times_fragment<NF>(gb + lane_row, vf);
            f32x4 p, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int in_chunk = 16 * t + 4 * grp + r, qi = kChunk * c + in_chunk;
              float x = scale * s[r];
              if (bias) x = x + ((live && qi < tq) ? bias[(int64_t)qi * tk + ki] : 0.0f);
              p[r] = expf((padded ? -INFINITY : x) - lsb[in_chunk]);
              ds[r] = p[r] * (dp[r] - dlb[in_chunk]);
            }
            const int perm = (16 * t + 4 * grp) * kPitch + col;
            transposed_times_tile<NF>(gb + perm, p, dva);
            transposed_times_tile<NF>(qb + perm, ds, dka);
          }
        }
      }
      if (more) {
        store_chunk<NF>(qbuf + ((c + 1) & 1) * kBuf, qx);
        store_chunk<NF>(gbuf + ((c + 1) & 1) * kBuf, gx);
        if (threadIdx.x < 2 * kChunk) stats[((c + 1) & 1) * 2 * kChunk + threadIdx.x] = sx;
      }
      __syncthreads();
    }
    if (my.lanes > 1) {
      if (my.lane > 0) {
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            lds[merge_slot(wave, split, kValues, 4 * f + r, lane)] = dka[f][r];
            lds[merge_slot(wave, split, kValues, 4 * NF + 4 * f + r, lane)] = dva[f][r];
          }
      }
      __syncthreads();
      if (my.lane == 0) {
        for (int j = 1; j < my.lanes; ++j)
#pragma unroll
          for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int from = j * split + my.strip;
              dka[f][r] = dka[f][r] + lds[merge_slot(from, split, kValues, 4 * f + r, lane)];
              dva[f][r] = dva[f][r] + lds[merge_slot(from, split, kValues, 4 * NF + 4 * f + r, lane)];
            }
      }
      __syncthreads();
    }
    if (active && live && my.lane == 0) {
      float *ok = dk + row * dkv_stride + at.h * d;
      float *ov = dv + row * dkv_stride + at.h * d;
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int cc = 16 * f + 4 * grp + r;
          if (cc < d) {
            ok[cc] = scale * dka[f][r];
            ov[cc] = dva[f][r];
          }
        }
    }
  }
}

// Workgroups over strips of `t` rows: 1, 2 or 4 strips per workgroup, the other waves being lanes over the chunk's
// tiles.
struct Split {
  int per_group, groups;
  int64_t total;
  int grid;
  Split(int64_t b, int heads, int t) {
    const int strips = (t + kStrip - 1) / kStrip;
    per_group = strips >= 3 ? 4 : strips;
    groups = (strips + per_group - 1) / per_group;
    total = b * heads * groups;
    grid = (int)(total < kMaxGridLong ? total : kMaxGridLong);
  }
};

struct LongForwardLaunch {
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
    constexpr int kBytes = lds_floats(NF) * (int)sizeof(float);
    if (const int e = allow_dynamic_lds<&attention_long_forward_kernel<NF>>(kBytes)) return e;
    const Split s(b, heads, tq);
    attention_long_forward_kernel<NF><<<s.grid, kBlock, kBytes, stream>>>(
        q, q_stride, k, v, kv_stride, key_padding, bias, s.total, s.groups, s.per_group, tq, tk, heads, d, scale, out, lse);
    return launch_status();
  }
};

struct LongBackwardLaunch {
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
    constexpr int kBytes = lds_floats(NF) * (int)sizeof(float);
    if (const int e = allow_dynamic_lds<&attention_long_backward_q_kernel<NF>>(kBytes)) return e;
    if (const int e = allow_dynamic_lds<&attention_long_backward_kv_kernel<NF>>(kBytes)) return e;
    const Split sq(b, heads, tq), sk(b, heads, tk);
    attention_long_backward_q_kernel<NF><<<sq.grid, kBlock, kBytes, stream>>>(
        q, q_stride, k, v, kv_stride, key_padding, bias, out, lse, dout, sq.total, sq.groups, sq.per_group, tq, tk, heads,
        d, scale, dq, dq_stride, delta);
    attention_long_backward_kv_kernel<NF><<<sk.grid, kBlock, kBytes, stream>>>(
        q, q_stride, k, v, kv_stride, key_padding, bias, lse, delta, dout, sk.total, sk.groups, sk.per_group, tq, tk, heads,
        d, scale, dk, dv, dkv_stride);
    return launch_status();
  }
};

}  // namespace
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_attention_long_supports(int tq, int tk, int heads, int d) {
  if (tq < 1 || tk < 1 || heads < 1 || d < 1) return RL8_ESIZE;
  return tq <= kLongMaxT && tk <= kLongMaxT && d <= kLongMaxD ? 1 : 0;
}

RL8_API int rl8_attention_long_f32(const float *q, int64_t q_stride, const float *k, const float *v, int64_t kv_stride,
                                   const uint8_t *key_padding, const float *bias, int64_t b, int tq, int tk, int heads,
                                   int d, float *out, float *lse, void *stream) {
  if (!q || !k || !v || !out) return RL8_ENULL;
  if (b < 1 || tq < 1 || tk < 1 || heads < 1 || d < 1) return RL8_ESIZE;
  if (q_stride < (int64_t)heads * d || kv_stride < (int64_t)heads * d) return RL8_ESIZE;
  if (!aligned_to(q, 4) || !aligned_to(k, 4) || !aligned_to(v, 4) || !aligned_to(bias, 4) || !aligned_to(out, 4) ||
      !aligned_to(lse, 4))
    return RL8_EALIGN;
  if (rl8_attention_long_supports(tq, tk, heads, d) != 1) return RL8_ECONFIG;
  return with_feature_tiles(d, LongForwardLaunch{q, q_stride, k, v, kv_stride, key_padding, bias, b, tq, tk, heads, d,
                                                 1.0f / sqrtf((float)d), out, lse, (hipStream_t)stream});
}

RL8_API int rl8_attention_long_backward_f32(const float *q, int64_t q_stride, const float *k, const float *v,
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
  if (rl8_attention_long_supports(tq, tk, heads, d) != 1) return RL8_ECONFIG;
  return with_feature_tiles(d, LongBackwardLaunch{q, q_stride, k, v, kv_stride, key_padding, bias, out, lse, dout, b, tq,
                                                  tk, heads, d, 1.0f / sqrtf((float)d), dq, dq_stride, dk, dv,
                                                  dkv_stride, delta_workspace, (hipStream_t)stream});
}
