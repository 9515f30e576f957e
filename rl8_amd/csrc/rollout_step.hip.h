// One rollout timestep is always: draw an action from the policy's outputs, advance the env, write
// action / logp / value / reward / obs[t+1] into the buffer's columns, carry rdr[t+1] = gamma * rdr[t] + r.
// The pieces every fused per-timestep kernel (and the two scatter kernels) share live here, once; a kernel keeps only
// what is its env's own: where the policy's outputs come from, the *_advance call, the state and obs[t+1] stores.
#pragma once
#include <initializer_list>

#include "common.hip.h"
#include "device_math.hip.h"

namespace rl8 {

// The columns every timestep writes beside action and obs[t+1] (rdr_t / rdr_t1: both or neither).
struct StepColumns {
  float *logp_col, *value_col, *reward_col;
  const float *rdr_t;
  float *rdr_t1;
  float gamma;

  __device__ __forceinline__ void record(int64_t i, float lp, float v, float r) const {
    reward_col[i] = r;
    logp_col[i] = lp;
    value_col[i] = v;
    if (rdr_t1) rdr_t1[i] = gamma * rdr_t[i] + r;
  }
};

// Row i of a dense [N][K] fp32 array, in registers (K = 2: one 8-byte load, so p is 8-byte aligned).
template <int K>
__device__ __forceinline__ void load_row(const float *__restrict__ p, int64_t i, float (&x)[K]) {
  if constexpr (K == 2) {
    const float2 v = *reinterpret_cast<const float2 *>(p + 2 * i);
    x[0] = v.x;
    x[1] = v.y;
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) x[j] = p[K * i + j];
  }
}

// One K-way categorical action from logits already in registers.  The Exp(1) draws are always handed to
// categorical_draw in registers -- the injected ones (noise [N][K]), or the ones it would take from the Philox stream
// itself: a pointer that may be null would put q in the private segment.
template <int K>
__device__ __forceinline__ int draw_categorical_x(const float (&x)[K], const float *__restrict__ noise, int64_t i,
                                                  uint64_t seed, uint64_t row, uint64_t step, bool deterministic,
                                                  float *lp) {
  float q[K];
#pragma unroll
  for (int j = 0; j < K; ++j) q[j] = 1.0f;
  if (!deterministic) {
    if (noise) {
      load_row<K>(noise, i, q);
    } else {
      // (the Philox round keys depend on the seed alone; hoisted out of the env loop they are twenty SGPRs more than
      // these kernels have left and come back through v_readlane: keep them a few scalar adds per env instead)
      asm("" : "+s"(seed) : "v"((uint32_t)i));
#pragma unroll
      for (int j = 0; j < K; ++j) q[j] = rl8_exponential(seed, row, step, (uint32_t)j);
    }
  }
  return categorical_draw<K>(x, q, seed, row, step, 0u, deterministic, lp);
}

// The same from row i of logits [N][K].
template <int K>
__device__ __forceinline__ int draw_categorical(const float *__restrict__ logits, const float *__restrict__ noise,
                                                int64_t i, uint64_t seed, uint64_t row, uint64_t step,
                                                bool deterministic, float *lp) {
  float x[K];
  load_row<K>(logits, i, x);
  return draw_categorical_x<K>(x, noise, i, seed, row, step, deterministic, lp);
}

// One Normal / SquashedNormal action dim from mean[i], log_std[i]; *lp is the log-probability the buffer keeps.
__device__ __forceinline__ float draw_normal(const float *__restrict__ mean, const float *__restrict__ log_std,
                                             const float *__restrict__ noise, int64_t i, uint64_t seed, uint64_t row,
                                             uint64_t step, bool squashed, bool deterministic, float *lp) {
  float e = 0.0f;
  if (!deterministic) e = noise ? noise[i] : rl8_normal(seed, row, step, 0u);
  float l, c;
  const float act = normal_draw(mean[i], log_std[i], e, squashed, deterministic, &l, &c);
  *lp = squashed ? l - c : l;
  return act;
}

// The discrete dummy env's timestep from its two logits x and its value v: draw, step, record.
__device__ __forceinline__ void dummy_discrete_timestep(const float (&x)[2], float v, const float *__restrict__ noise,
                                                        float *__restrict__ state, int64_t *__restrict__ action_col,
                                                        float *__restrict__ obs_col_next, const StepColumns &cols,
                                                        int64_t i, uint64_t seed, uint64_t row, uint64_t step,
                                                        bool deterministic) {
  float lp;
  const int act = draw_categorical_x<2>(x, noise, i, seed, row, step, deterministic, &lp);
  action_col[i] = act;
  const float s = dummy_step_discrete(state[i], act);
  state[i] = s;
  obs_col_next[i] = s;
  cols.record(i, lp, v, -fabsf(s));
}

// ---- host: the argument checks of the rl8_rollout_step_* / rl8_rollout_scatter_* entries --------------------------
struct StepPointer {
  const void *p;
  unsigned align;        // bytes: 4 for a float column, 8 for an int64 one, more where the kernel loads vectors
  bool required = true;  // an optional pointer may be null; when present it is held to its alignment
};

inline bool aligned_to(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// RL8_ENULL for a missing required pointer or an rdr_t / rdr_t1 pair of which one is null, then RL8_ESIZE for n < 1
// (or an entry's own size check, `sizes_ok`), then RL8_EALIGN; 0 when the launch may go ahead.
inline int check_rollout_step_args(std::initializer_list<StepPointer> pointers, const float *rdr_t, const float *rdr_t1,
                                   int64_t n, bool sizes_ok = true) {
  for (const StepPointer &a : pointers)
    if (a.required && !a.p) return RL8_ENULL;
  if ((rdr_t == nullptr) != (rdr_t1 == nullptr)) return RL8_ENULL;
  if (n <= 0 || !sizes_ok) return RL8_ESIZE;
  for (const StepPointer &a : pointers)
    if (!aligned_to(a.p, a.align)) return RL8_EALIGN;
  if (!aligned_to(rdr_t, 4) || !aligned_to(rdr_t1, 4)) return RL8_EALIGN;
  return 0;
}

}  // namespace rl8
