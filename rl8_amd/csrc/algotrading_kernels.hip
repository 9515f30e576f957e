// The reference's fourth example environment, AlgoTrading (examples/algotrading/env.py:23-183), on the template of
// the other built-in envs: struct-of-arrays state [9][N] (invested, position, f, k_cyclic, k_market, t, price and the
// two log-changes, all fp32 -- invested is 0 / 1 and t a small integer, both exact), one lane per env, a standalone
// step / reset pair behind Env.step / Env.reset and a fused per-timestep kernel (three-way categorical draw from the
// masked logits + the advance + rollout-buffer bookkeeping) for Algorithm.collect().
//
// Its observations are a dict of four leaves, so where the other envs write one obs slab these write four:
// action_mask [N][3] bool (one byte each), invested [N] int64, LOG_CHANGE(price) [N] and LOG_CHANGE(price, position)
// [N] fp32.
//
// Traffic per env and timestep, fused kernel: reads logits 12 B, value 4, state 36, rdr 4; writes action 8, logp 4,
// value 4, reward 4, the leaves 3 + 8 + 4 + 4, state 24, rdr 4 = 123 B, beside one sinf and up to five fp64 logs.
#include "common.hip.h"
#include "device_math.hip.h"
#include "rollout_step.hip.h"

namespace rl8 {

__global__ __launch_bounds__(kBlock) void algotrading_reset_kernel(
    float *__restrict__ state, int64_t n, float f_bounds, float k_cyclic_bounds, float k_market_bounds,
    uint64_t seed, uint64_t reset_count, int64_t env_offset, uint8_t *__restrict__ mask,
    int64_t *__restrict__ invested, float *__restrict__ log_change, float *__restrict__ log_change_position) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    uint32_t r[4], r2[4];
    rl8_philox4x32_10(seed, (uint64_t)(i + env_offset), reset_count, rl8_stream_block(RL8_STREAM_RESET, 0), r);
    rl8_philox4x32_10(seed, (uint64_t)(i + env_offset), reset_count, rl8_stream_block(RL8_STREAM_RESET, 1), r2);
    AlgoTradingState s;
    s.invested = 0.0f;
    s.position = 0.0f;
    s.f = rl8_u01_24(r[0]) * (f_bounds - 0.0f) + 0.0f;
    s.k_cyclic = rl8_u01_24(r[1]) * (k_cyclic_bounds - (-k_cyclic_bounds)) + (-k_cyclic_bounds);
    s.k_market = rl8_u01_24(r[2]) * (k_market_bounds - (-k_market_bounds)) + (-k_market_bounds);
    s.t = (float)(r[3] % 10u);
    s.price = rl8_u01_24(r2[0]) * (10000.0f - 100.0f) + 100.0f;
    s.log_change = 0.0f;
    s.log_change_position = 0.0f;
    algotrading_store(state, n, i, s);
    state[2 * n + i] = s.f;
    state[3 * n + i] = s.k_cyclic;
    state[4 * n + i] = s.k_market;
    if (mask) algotrading_write_obs(s, i, mask, invested, log_change, log_change_position);
  }
}

__global__ __launch_bounds__(kBlock) void algotrading_step_kernel(
    float *__restrict__ state, const int64_t *__restrict__ action, uint8_t *__restrict__ mask,
    int64_t *__restrict__ invested, float *__restrict__ log_change, float *__restrict__ log_change_position,
    float *__restrict__ reward, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    AlgoTradingState s = algotrading_load(state, n, i);
    const float r = algotrading_advance(s, action[i]);
    algotrading_store(state, n, i, s);
    algotrading_write_obs(s, i, mask, invested, log_change, log_change_position);
    reward[i] = r;
  }
}

__global__ __launch_bounds__(kBlock) void rollout_step_algotrading_kernel(
    const float *__restrict__ logits, const float *__restrict__ value, const float *__restrict__ noise,
    float *__restrict__ state, int64_t *__restrict__ action_col, float *__restrict__ logp_col,
    float *__restrict__ value_col, float *__restrict__ reward_col, uint8_t *__restrict__ mask_next,
    int64_t *__restrict__ invested_next, float *__restrict__ log_change_next,
    float *__restrict__ log_change_position_next, const float *__restrict__ rdr_t, float *__restrict__ rdr_t1,
    float gamma, int64_t n, uint64_t seed, uint64_t step, int64_t env_offset, int deterministic) {
  const StepColumns cols = {logp_col, value_col, reward_col, rdr_t, rdr_t1, gamma};
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    float lp;
    const int act = draw_categorical<3>(logits, noise, i, seed, (uint64_t)(i + env_offset), step, deterministic != 0, &lp);
    AlgoTradingState s = algotrading_load(state, n, i);
    const float r = algotrading_advance(s, act);
    algotrading_store(state, n, i, s);
    algotrading_write_obs(s, i, mask_next, invested_next, log_change_next, log_change_position_next);
    action_col[i] = act;
    cols.record(i, lp, value[i], r);
  }
}

}  // namespace rl8

using namespace rl8;

RL8_API int rl8_algotrading_reset_f32(float *state, int64_t n, float f_bounds, float k_cyclic_bounds,
                                      float k_market_bounds, uint64_t seed, uint64_t reset_count, int64_t env_offset,
                                      uint8_t *mask_out, int64_t *invested_out, float *log_change_out,
                                      float *log_change_position_out, void *stream) {
  if (!state) return RL8_ENULL;
  const int outs = (mask_out != nullptr) + (invested_out != nullptr) + (log_change_out != nullptr) +
                   (log_change_position_out != nullptr);
  if (outs != 0 && outs != 4) return RL8_ENULL;  // the four observation leaves together, or none
  if (n <= 0) return RL8_ESIZE;
  if (!aligned_to(state, 4) || !aligned_to(invested_out, 8) || !aligned_to(log_change_out, 4) ||
      !aligned_to(log_change_position_out, 4))
    return RL8_EALIGN;
  algotrading_reset_kernel<<<grid_for(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(
      state, n, f_bounds, k_cyclic_bounds, k_market_bounds, seed, reset_count, env_offset, mask_out, invested_out,
      log_change_out, log_change_position_out);
  return launch_status();
}

RL8_API int rl8_algotrading_step_f32(float *state, const int64_t *action, uint8_t *mask_out, int64_t *invested_out,
                                     float *log_change_out, float *log_change_position_out, float *reward_out,
                                     int64_t n, void *stream) {
  if (!state || !action || !mask_out || !invested_out || !log_change_out || !log_change_position_out || !reward_out)
    return RL8_ENULL;
  if (n <= 0) return RL8_ESIZE;
  if (!aligned_to(state, 4) || !aligned_to(action, 8) || !aligned_to(invested_out, 8) ||
      !aligned_to(log_change_out, 4) || !aligned_to(log_change_position_out, 4) || !aligned_to(reward_out, 4))
    return RL8_EALIGN;
  algotrading_step_kernel<<<grid_for(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(
      state, action, mask_out, invested_out, log_change_out, log_change_position_out, reward_out, n);
  return launch_status();
}

RL8_API int rl8_rollout_step_algotrading_f32(const float *logits, const float *value, const float *noise, float *state,
                                             int64_t *action_col, float *logp_col, float *value_col, float *reward_col,
                                             uint8_t *mask_next, int64_t *invested_next, float *log_change_next,
                                             float *log_change_position_next, const float *rdr_t, float *rdr_t1,
                                             float gamma, int64_t n, uint64_t seed, uint64_t step, int64_t env_offset,
                                             int deterministic, void *stream) {
  if (const int bad = check_rollout_step_args(
          {{logits, 4}, {value, 4}, {noise, 4, false}, {state, 4}, {action_col, 8}, {logp_col, 4}, {value_col, 4},
           {reward_col, 4}, {mask_next, 1}, {invested_next, 8}, {log_change_next, 4}, {log_change_position_next, 4}},
          rdr_t, rdr_t1, n))
    return bad;
  rollout_step_algotrading_kernel<<<grid_for(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(
      logits, value, noise, state, action_col, logp_col, value_col, reward_col, mask_next, invested_next,
      log_change_next, log_change_position_next, rdr_t, rdr_t1, gamma, n, seed, step, env_offset, deterministic);
  return launch_status();
}
