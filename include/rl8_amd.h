/*
 * rl8_amd.h -- C ABI of the MI355X (gfx950) PPO hot path.
 *
 * One shared library, librl8_amd.so, built from rl8_amd/csrc with
 * `hipcc --offload-arch=gfx950`. Plain pointers and sizes only; every pointer is
 * a DEVICE pointer owned by the caller (PyTorch in the Python host, hipMalloc in
 * a C host) unless it says "host". Nothing here allocates, frees or
 * synchronises: each call enqueues kernels on `stream` (a hipStream_t passed as
 * void*; NULL = the default stream) and returns.
 *
 * Return value: 0 on success; RL8_E* (negative) when an argument check fails
 * (nothing was launched); a positive hipError_t if the launch itself failed.
 *
 * The reference (theOGognf/rl8) has no FFI on this path: its boundary is Python
 * call signatures. Each entry point below cites the reference function whose
 * arithmetic it replaces (paths relative to the reference checkout);
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Layouts.  N = num_envs, H = horizon, M = samples in a (mini)batch,
 * A = action dims, K = classes per action dim.
 *   "env-major"  buffer leaf: [N][H+1] contiguous  (the reference's [N, H+1, 1])
 *   "time-major" buffer leaf: [H+1][N] contiguous  (rl8_amd's own rollout
 *                buffer; exposed to Python as a transposed [N, H+1, 1] view)
 *
 * Which entry runs where (round 6; every entry is exported, declared here and called by rl8_amd/hip.py --
 * tests/test_host_logic.py checks the three lists against each other; none is dead):
 *   PRODUCT, default path (AlgorithmConfig / RecurrentAlgorithmConfig defaults, built-in envs, default models):
 *     rollout    rl8_rollout_step_{dummy,cartpole,mountain_car,pendulum}_f32, rl8_rollout_step_dummy_heads_f32,
 *                rl8_rollout_scatter_f32 (user envs), rl8_rollout_stats_f32, rl8_*_reset_f32, rl8_*_step_f32 (Env.step()
 *                called by the user), rl8_categorical_sample_logp_f32, rl8_normal_sample_logp_f32 (Distribution.sample())
 *     update     rl8_gae_scan_f32, rl8_advantage_normalise_f32 (their routes: rl8_gae_plan, rl8_advantage_normalise_route),
 *                rl8_ppo_loss_{categorical,normal}_fwd_bwd_f32,
 *                rl8_pack_samples, rl8_gather_packed, rl8_gather_minibatch, rl8_gather_sequences (dict observations)
 *                (their routes: rl8_rollout_stats_plan, rl8_gather_minibatch_plan, rl8_pack_plan)
 *     windows    (feed-forward models with padded rolling-window view requirements on "obs" / ("obs", leaf), and dict
 *                observations; RL8_AMD_WINDOW_KERNELS=0 puts both back on torch ops) rl8_window_last (collect(): the
 *                model's input at every timestep and at the bootstrap value), rl8_gather_windows (step(): the
 *                observation views of every minibatch)
 *     masked     (rl8_amd.nn.functional's masked_avg, masked_max, masked_log_softmax, masked_categorical_sample on dense
 *                f32 HIP tensors; RL8_AMD_MASKED_KERNELS=0 puts them back on torch ops) rl8_masked_pool[_backward]_f32
 *                (TransformerTrader pools its attended window with it), rl8_masked_log_softmax[_backward]_f32,
 *                rl8_masked_categorical_sample_f32 (their route: rl8_masked_rows_route)
 *     attention  (rl8_amd.nn's SelfAttention / CrossAttention on f32 HIP tensors with sequences of at most 64 cells and
 *                heads of at most 16 floats, TransformerTrader among them; RL8_AMD_ATTENTION_KERNELS=0, read on every
 *                call by rl8_amd/nn/fused_attention.py, puts the core back on nn.MultiheadAttention's math backend)
 *                rl8_attention_f32, rl8_attention_backward_f32 (their envelope: rl8_attention_supports)
 *     feedforward (the LayerNorm -> Linear -> ReLU -> Linear block that ends every SelfAttention / CrossAttention, with
 *                its skip connection, on f32 HIP tensors of at most 32 features and 256 hidden units;
 *                opt-in: RL8_AMD_FEEDFORWARD_KERNELS=1, read on every call by rl8_amd/nn/fused_feedforward.py, takes
 *                it off the torch modules) rl8_feedforward_f32, rl8_feedforward_backward_f32 (their envelope:
 *                rl8_feedforward_supports; their sizes: rl8_feedforward_limits, rl8_feedforward_workspace_floats)
 *     towers     rl8_mlp_tower_forward_f16_f32, rl8_mlp_tower_backward_gate_f16_f32, rl8_mlp_tower_backward_f16_f32,
 *                rl8_mlp_wgrad_gate_bits_f32, rl8_mlp_wgrad_fused_split_f32, rl8_mlp_wgrad_fused_pair_f32,
 *                rl8_mlp_pack_w2_f16, rl8_mlp_pack_w2_f16_gate, rl8_mlp_dout_pair_check, the *_supports / *_bytes /
 *                *_floats / *_max_rows queries
 *     towers, hidden width 256 with heads of 9 to 128 outputs in all (RL8_AMD_WIDE_HEAD_TOWERS=0: the torch modules):
 *                rl8_mlp_wide_out_{pack,forward,backward,wgrad}_f32 and their *_supports / *_bytes / *_floats /
 *                *_max_rows queries, with rl8_mlp_pack_w2_f32 and the dW2 entries of the wide-input towers
 *     recurrent  rl8_lstm_pack_split, rl8_lstm_split_state[_bound], rl8_lstm_step_split_f32,
 *                rl8_lstm_rows_backward_pack, rl8_lstm_rows_backward[_heads]_f32, rl8_lstm_wgrad_f16_f32,
 *                rl8_linear_heads_{forward,forward_pair,backward}_f32
 *     recurrent, hidden width 256 behind an observation of 8 to 128 floats (RL8_AMD_WIDE_INPUT_LSTM=0: torch.nn.LSTM):
 *                rl8_lstm_wide_in_{pack,forward,wgrad}_f32, rl8_lstm_backward_dgates_f32 (RL8_AMD_LSTM_BACKWARD_ROWS=0),
 *                with the rows backward and the W_hh weight gradients above
 *     recurrent, hidden width 64 / 128 (model_config={"hidden_size": 64}): rl8_lstm_narrow_{forward,backward,reduce}_f32,
 *                rl8_lstm_narrow_backward_heads_f32 (one layer, heads of <= 4 outputs: the one-node training pass),
 *                rl8_lstm_narrow_input_grad_f32 (dL/dx of layer 0, for models with an encoder in front of the LSTM),
 *                rl8_lstm_stack_* (layers 1..), rl8_linear_heads_narrow_{forward,forward_pair,backward}_f32,
 *                rl8_rollout_step_dummy_heads_narrow_f32 (the lean rollout's last launch of a timestep)
 *   PRODUCT, fallback (shapes outside the plane kernels' envelope -- d_in > 16, n_out > 8, hidden != 256 go to eager --
 *   or a switch: RL8_AMD_TOWER_GEMM=f32, RL8_WGRAD_PLANES=bf16, the LSTM switches below), and THE YARDSTICK the parity
 *   tests hold the plane kernels against beside fp64:
 *     rl8_mlp_tower_forward_f32, rl8_mlp_tower_backward_f32, rl8_mlp_wgrad_f32, rl8_mlp_wgrad_split_f32,
 *     rl8_mlp_pack_w2_f32, rl8_lstm_pack_f32, rl8_lstm_forward_f32, rl8_lstm_backward_f32,
 *     rl8_mlp_wgrad_strided_f32, rl8_mlp_wgrad_split_strided_f32, rl8_mlp_wgrad_f16_strided_f32 (one gate per launch)
 *   OPT-IN prototype (RL8_AMD_TOWERS=piecewise; never the default, never the headline): rl8_pw_*
 * The LSTM switches and where each is read.  rl8_amd/nn/fused_lstm.py reads RL8_AMD_LSTM_GEMM=f32 (the fp32-MFMA step
 * kernel, backward and weight gradient), RL8_AMD_LSTM_BACKWARD_ROWS=0 (the fp32-MFMA backward through time, the bf16-plane
 * weight gradient) and RL8_AMD_LSTM_FUSE_HEADS=0 (LSTM and heads as two autograd nodes) at import, into module attributes;
 * fused_lstm._plan reads those and RL8_AMD_LSTM_WGRAD_PLANES=bf16 (the bf16-plane weight gradient) and
 * RL8_AMD_LSTM_WGRAD_GATES=separate (one weight-gradient launch per gate) on every call, once for a forward and its
 * backward.  RL8_AMD_ROLLOUT_FUSE_HEADS=0 (the lean recurrent rollout's heads in launches of their own) is read by
 * fused_lstm when a rollout is set up; RL8_AMD_LSTM_BACKWARD_PLANES=bf16 (the heads form of the backward through time on
 * three bf16 planes instead of two fp16 ones) by rl8_lstm_rows_backward_heads_f32 itself, on every call.
 */
#ifndef RL8_AMD_H
#define RL8_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RL8_OK 0
#define RL8_ENULL (-1)   /* required pointer is NULL */
#define RL8_ESIZE (-2)   /* size / shape argument out of range */
#define RL8_EALIGN (-3)  /* pointer not aligned as required */
#define RL8_ECONFIG (-4) /* unsupported combination of options */

#define RL8_MAX_CLASSES 64 /* K upper bound for the categorical kernels */
#define RL8_MAX_WIDE_CLASSES 65536 /* K upper bound for the wave-per-row (_wide_) categorical kernels */
#define RL8_MAX_PARTIALS 2048 /* upper bound on per-launch partial rows */

/* ABI / build identification: returns RL8_ABI_VERSION of the library's build; `arch` (host pointer, may be NULL)
 * receives "gfx950".  A binding compares it with the header it was written against (rl8_amd/hip.py refuses a
 * mismatch).  History: 100 rounds 1-2; 103 round 3 (bf16-plane forward / data-gradient entries removed, reduction
 * scratch doubled with two-level tickets -- bump owed since then); 104 round 4 (weight-gradient
 * workspace: guard words and lifetime counters behind the slabs; caller-owned outputs of the forward unchanged);
 * 105 round 4 (rl8_gather_minibatch takes index = NULL: all samples in order); 106 round 6 (no signature changed:
 * rl8_lstm_rows_backward_pack writes the fp16 planes of W_hh^T behind the bf16 ones -- rl8_lstm_rows_backward_pack_bytes
 * grew by 1 MiB + 16, and rl8_lstm_rows_backward_heads_f32 reads them; rl8_mlp_backward_f16_supports and
 * rl8_lstm_split_supports report wider envelopes; the weight-gradient workspace's tail words moved).  Added under 106
 * without a bump (new entries only, nothing existing changed): rl8_rollout_scatter_leaves_f32,
 * rl8_algotrading_reset_f32, rl8_algotrading_step_f32, rl8_rollout_step_algotrading_f32, rl8_gather_windows,
 * rl8_window_last.  107 (no signature changed: min / max of rl8_rollout_stats_f32 are NaN when a reward is, where they
 * used to drop it; rl8_gather_minibatch checks every field before its first launch; new queries
 * rl8_rollout_stats_plan, rl8_gather_minibatch_plan, rl8_pack_plan).  Added under 107 without a bump (new entries
 * only): rl8_masked_rows_route, rl8_masked_pool_f32, rl8_masked_pool_backward_f32, rl8_masked_log_softmax_f32,
 * rl8_masked_log_softmax_backward_f32, rl8_masked_categorical_sample_f32; rl8_attention_supports, rl8_attention_f32,
 * rl8_attention_backward_f32; rl8_feedforward_supports, rl8_feedforward_limits, rl8_feedforward_workspace_floats,
 * rl8_feedforward_f32, rl8_feedforward_backward_f32.  Widened under 107 without a bump (no entry added, none changed
 * in signature, and a binding of either age works with a library of either age): rl8_lstm_split_state[_bound] take an
 * h of any finite size -- they scale the call's planes by a power of two from max |h| and leave it in sixteen bytes
 * behind the planes, which rl8_lstm_step_split_f32 reads behind h_planes and writes behind planes_out.  The planes'
 * size has always been rl8_lstm_split_state_bytes(b), asked of the library at run time: it grew by those sixteen
 * bytes, and inputs that were inside the old envelope (max |h| < 2) give the bits they gave. */
#define RL8_ABI_VERSION 107
int rl8_abi_version(char *arch, int arch_len);

/* Scratch the reductions need (bytes); the caller allocates it once per stream
 * (device memory, 16-byte aligned), ZEROES it once, and passes it to the calls
 * that take `scratch`.  It holds per-block partial rows and the arrival ticket
 * of the single-launch reductions (re-zeroed by each call); two calls sharing
 * one scratch must be ordered on one stream. */
int64_t rl8_scratch_bytes(void);

/* ---------------------------------------------------------------------- *
 * a-1  DummyEnv.step                  src/rl8/env.py:224-230, 253-259
 * state [N] f32 updated in place; action [N] int64 (discrete: state += 2a-1)
 * or f32 (continuous: state += a); reward_out [N] = -|state|.
 * ---------------------------------------------------------------------- */
int rl8_dummy_env_step_f32(float *state, const void *action, int is_discrete,
                           float *reward_out, int64_t n, void *stream);

/* DummyEnv.reset                      src/rl8/env.py:197-203
 * state ~ U(-bounds, bounds) from the build's Philox stream (rl8_philox.h);
 * env_offset = global index of this shard's first env. */
int rl8_dummy_env_reset_f32(float *state, int64_t n, float bounds, uint64_t seed,
                            uint64_t reset_count, int64_t env_offset, void *stream);

/* ---------------------------------------------------------------------- *
 * a-2  CartPole step                  examples/cartpole/env.py:12-64
 * state SoA [4][N] (x, x_dot, theta, theta_dot) in place; action [N] int64 in
 * {0,1,2}; obs_out [N][5] rows (x, x_dot, cos, sin, theta_dot) written with
 * row stride obs_stride floats (5 for a dense [N,5]); reward_out [N].
 * ---------------------------------------------------------------------- */
typedef struct {
  float force_mag, gravity, length, pole_mass, pole_mass_length, total_mass, tau;
  int32_t semi_implicit; /* 0: "euler" (:43-47), 1: semi-implicit (:48-52) */
} rl8_cartpole_cfg;

int rl8_cartpole_step_f32(float *state, const int64_t *action, const rl8_cartpole_cfg *cfg /*host*/,
                          float *obs_out, int64_t obs_stride, float *reward_out, int64_t n,
                          void *stream);

/* CartPole.reset                      examples/cartpole/env.py:128-136
 * state ~ N(0, std) [4][N]; obs_out as above (may be NULL). */
int rl8_cartpole_reset_f32(float *state, int64_t n, float std, uint64_t seed,
                           uint64_t reset_count, int64_t env_offset, float *obs_out,
                           int64_t obs_stride, void *stream);

/* ---------------------------------------------------------------------- *
 * a-6  Distribution.sample / logp     src/rl8/distributions.py:113-170
 * (-> torch.distributions.Categorical.sample == argmax(p / q), q ~ Exp(1))
 * logits [M][A][K] f32; noise: injected q [M][A][K] (may be NULL -> Philox
 * (seed, row_offset + row, step)); action_out [M][A] int64; logp_out [M] f32.
 * deterministic != 0 -> mode.
 * ---------------------------------------------------------------------- */
int rl8_categorical_sample_logp_f32(const float *logits, const float *noise, int64_t *action_out,
                                    float *logp_out, int64_t m, int a, int k, uint64_t seed,
                                    uint64_t step, int64_t row_offset, int deterministic,
                                    void *stream);

/* The same draw for rows of 2 <= k <= RL8_MAX_WIDE_CLASSES classes with a * k < 2^31 (else RL8_ESIZE, before any
 * launch): one wave per row i, looping over the a action dimensions, lanes striding over the classes.  The arithmetic
 * is that of the entry above operation for operation -- correctly rounded exp / log, nl_j = x_j - lse,
 * p_j = exp(nl_j - max nl) / s2, argmax_j p_j / q_j with the first index on ties, logp = sum_d nl[class] -- except
 * that the two sums and the maximum are taken lane by lane and then across the 64 lanes in a fixed xor butterfly, so
 * s and s2 may differ in their last place from the sequential sums above.  Philox word d * k + j of
 * (seed, i + row_offset, step), as above: for k <= RL8_MAX_CLASSES both entries see the same draws. */
int rl8_categorical_wide_sample_logp_f32(const float *logits, const float *noise, int64_t *action_out,
                                         float *logp_out, int64_t m, int a, int k, uint64_t seed,
                                         uint64_t step, int64_t row_offset, int deterministic,
                                         void *stream);

/* Normal / SquashedNormal: mean, log_std [M][A]; noise: injected eps [M][A]
 * (may be NULL -> Philox); action_out [M][A] f32; logp_out [M]. */
int rl8_normal_sample_logp_f32(const float *mean, const float *log_std, const float *noise,
                               float *action_out, float *logp_out, int64_t m, int a,
                               int squashed, uint64_t seed, uint64_t step, int64_t row_offset,
                               int deterministic, void *stream);

/* ---------------------------------------------------------------------- *
 * a-3  Rollout bookkeeping            src/rl8/algorithms/_feedforward.py:378-393
 * One launch per timestep t for a generic Env: rdr[t+1] = gamma*rdr[t] + r and
 * the five column writes.  All destinations are columns of TIME-MAJOR leaves,
 * i.e. contiguous [N][d] slabs; sources are the policy / env outputs [N][d].
 * rdr_t / rdr_t1 may be NULL (normalize_rewards = False).
 * ---------------------------------------------------------------------- */
int rl8_rollout_scatter_f32(const void *action, int64_t action_row_bytes, const float *logp,
                            const float *value, const float *reward, const float *obs,
                            int64_t obs_dim, void *action_col, float *logp_col, float *value_col,
                            float *reward_col, float *obs_col_next, const float *rdr_t,
                            float *rdr_t1, float gamma, int64_t n, void *stream);

/* Fused per-timestep kernel for the built-in dummy envs: sampler (a-6) +
 * env.step (a-1) + bookkeeping (a-3) in ONE launch.
 *   discrete:   features = logits [N][1][2];  noise = q [N][1][2] or NULL
 *   continuous: features = mean [N][1], features2 = log_std [N][1]; noise = eps
 *               [N][1] or NULL; squashed selects SquashedNormal.
 * state [N] in place (the env's state; also written to obs_col_next). */
int rl8_rollout_step_dummy_f32(int is_discrete, int squashed, const float *features,
                               const float *features2, const float *value, const float *noise,
                               float *state, void *action_col, float *logp_col, float *value_col,
                               float *reward_col, float *obs_col_next, const float *rdr_t,
                               float *rdr_t1, float gamma, int64_t n, uint64_t seed, uint64_t step,
                               int64_t env_offset, int deterministic, void *stream);

/* The discrete form for the default recurrent model (models/_recurrent.py:287-321: a two-way logits head and a value
 * head on the LSTM's output), heads included: h [N][256] = h_t, w_pol [2][256], b_pol [2], w_vf [1][256], b_vf [1];
 * logits and value are formed in the kernel exactly as rl8_linear_heads_forward_f32 forms them, the rest as
 * rl8_rollout_step_dummy_f32(is_discrete = 1): one launch per rollout timestep behind the LSTM step instead of three. */
int rl8_rollout_step_dummy_heads_f32(const float *h, const float *w_pol, const float *b_pol, const float *w_vf,
                                     const float *b_vf, const float *noise, float *state, int64_t *action_col,
                                     float *logp_col, float *value_col, float *reward_col, float *obs_col_next,
                                     const float *rdr_t, float *rdr_t1, float gamma, int64_t n, uint64_t seed,
                                     uint64_t step, int64_t env_offset, int deterministic, void *stream);

/* The same for an LSTM of hidden width 64 or 128: h [N][hidden], w_pol [2][hidden], w_vf [1][hidden]; logits and value
 * exactly as rl8_linear_heads_narrow_forward_f32 forms them.  RL8_ESIZE for other widths; h, w_pol, w_vf 16-byte
 * aligned, noise 8-byte aligned. */
int rl8_rollout_step_dummy_heads_narrow_f32(const float *h, int hidden, const float *w_pol, const float *b_pol,
                                            const float *w_vf, const float *b_vf, const float *noise, float *state,
                                            int64_t *action_col, float *logp_col, float *value_col, float *reward_col,
                                            float *obs_col_next, const float *rdr_t, float *rdr_t1, float gamma,
                                            int64_t n, uint64_t seed, uint64_t step, int64_t env_offset,
                                            int deterministic, void *stream);

/* Fused per-timestep kernel for CartPole (K = 3): sampler + physics +
 * bookkeeping.  obs_col_next is a [N][5] slab. */
int rl8_rollout_step_cartpole_f32(const float *logits, const float *value, const float *noise,
                                  float *state, const rl8_cartpole_cfg *cfg /*host*/,
                                  int64_t *action_col, float *logp_col, float *value_col,
                                  float *reward_col, float *obs_col_next, const float *rdr_t,
                                  float *rdr_t1, float gamma, int64_t n, uint64_t seed,
                                  uint64_t step, int64_t env_offset, int deterministic,
                                  void *stream);

/* ---------------------------------------------------------------------- *
 * N2  The other example environments, same SoA-state template
 *
 * MountainCar                         examples/mountain_car/env.py:12-38, :96-104
 * state SoA [2][N] (position, velocity) in place; action [N] int64 in {0,1,2};
 * obs_out [N][2] rows (position, velocity) with row stride obs_stride floats;
 * reward_out [N].  reset: position ~ N(-0.5, 0.05), velocity ~ N(0, 0.05) from the
 * build's Philox stream; obs_out may be NULL.
 * ---------------------------------------------------------------------- */
typedef struct {
  float force_mag, goal_position, goal_velocity, gravity, max_position, max_speed, min_position;
} rl8_mountain_car_cfg;

int rl8_mountain_car_step_f32(float *state, const int64_t *action,
                              const rl8_mountain_car_cfg *cfg /*host*/, float *obs_out,
                              int64_t obs_stride, float *reward_out, int64_t n, void *stream);
int rl8_mountain_car_reset_f32(float *state, int64_t n, uint64_t seed, uint64_t reset_count,
                               int64_t env_offset, float *obs_out, int64_t obs_stride,
                               void *stream);
/* Fused per-timestep kernel (K = 3 sampler + physics + bookkeeping), arguments as
 * rl8_rollout_step_cartpole_f32; obs_col_next is a [N][2] slab. */
int rl8_rollout_step_mountain_car_f32(const float *logits, const float *value, const float *noise,
                                      float *state, const rl8_mountain_car_cfg *cfg /*host*/,
                                      int64_t *action_col, float *logp_col, float *value_col,
                                      float *reward_col, float *obs_col_next, const float *rdr_t,
                                      float *rdr_t1, float gamma, int64_t n, uint64_t seed,
                                      uint64_t step, int64_t env_offset, int deterministic,
                                      void *stream);

/* Pendulum                            examples/pendulum/env.py:12-39, :101-113
 * state SoA [2][N] (th, thdot) in place; action [N] f32 (clipped to +-max_torque
 * inside); obs_out [N][3] rows (cos th', sin th', thdot'); reward_out [N] = minus
 * the cost of the state and torque BEFORE the step.  gravity_coeff = 3g/(2l) and
 * torque_coeff = 3/(m l^2), formed in double by the caller as the reference does
 * (:32).  reset: th ~ U(-pi, pi), thdot ~ U(-1, 1). */
typedef struct {
  float dt, gravity_coeff, torque_coeff, max_speed, max_torque;
} rl8_pendulum_cfg;

int rl8_pendulum_step_f32(float *state, const float *action, const rl8_pendulum_cfg *cfg /*host*/,
                          float *obs_out, int64_t obs_stride, float *reward_out, int64_t n,
                          void *stream);
int rl8_pendulum_reset_f32(float *state, int64_t n, uint64_t seed, uint64_t reset_count,
                           int64_t env_offset, float *obs_out, int64_t obs_stride, void *stream);
/* Fused per-timestep kernel: Normal / SquashedNormal sampler (mean, log_std [N],
 * noise: injected standard normals or NULL) + physics + bookkeeping;
 * action_col [N] f32, obs_col_next [N][3]. */
int rl8_rollout_step_pendulum_f32(int squashed, const float *mean, const float *log_std,
                                  const float *value, const float *noise, float *state,
                                  const rl8_pendulum_cfg *cfg /*host*/, float *action_col,
                                  float *logp_col, float *value_col, float *reward_col,
                                  float *obs_col_next, const float *rdr_t, float *rdr_t1,
                                  float gamma, int64_t n, uint64_t seed, uint64_t step,
                                  int64_t env_offset, int deterministic, void *stream);

/* ---------------------------------------------------------------------- *
 * a-4  Collect statistics             src/rl8/algorithms/_feedforward.py:411-436
 * rewards / rdr leaves with element strides (env_stride, time_stride) so both
 * layouts are accepted; rdr may be NULL.  Writes 12 doubles to stats_out:
 *   [0] n_envs  [1] sum(ret) [2] sum(ret^2) [3] min(ret) [4] max(ret)
 *   [5] n*h     [6] sum(r)   [7] sum(r^2)   [8] min(r)   [9] max(r)
 *   [10] sum(rdr[:,1:]) [11] sum(rdr[:,1:]^2)
 * (raw moments, so that shards can be combined with one all-reduce each for
 * SUM / MIN / MAX before the host forms mean and unbiased std).
 * Rewards that are not finite follow the reference's torch ops: the sums follow IEEE 754, min / max of a set that holds
 * a NaN are NaN (torch.min / torch.max propagate it), and infinities are ordinary extrema.
 * ---------------------------------------------------------------------- */
int rl8_rollout_stats_f32(const float *rewards, const float *rdr, int64_t n, int64_t h,
                          int64_t env_stride, int64_t time_stride, double *stats_out,
                          void *scratch, void *stream);

/* What rl8_rollout_stats_f32 launches for a shape, its strides (in elements) and an alignment (aligned16_all != 0:
 * rewards, and rdr where given, are 16-byte aligned).  Host arithmetic only: no device is touched, and the entry
 * launches exactly what this reports.
 *   STATS_VEC4  four adjacent envs per lane through 16-byte loads: env_stride == 1, N % 4 == 0, time_stride % 4 == 0,
 *               aligned
 *   STATS_VEC1  one env per lane, any strides
 * grid: workgroups of 256 lanes (one partial row each); trips: the env groups the busiest lane visits, more than one
 * when the grid is capped (2048 workgroups; RL8_STATS_GRID_CAP in the environment, read once per process, lowers the
 * cap of the VEC4 route). */
#define RL8_STATS_VEC4 0
#define RL8_STATS_VEC1 1
typedef struct {
  int route;
  int grid;
  int64_t trips;
} rl8_stats_plan_t;
int rl8_rollout_stats_plan(int64_t n, int64_t h, int64_t env_stride, int64_t time_stride, int aligned16_all,
                           rl8_stats_plan_t *out /*host*/);

/* ---------------------------------------------------------------------- *
 * a-5  generalized_advantage_estimate src/rl8/nn/functional.py:50-123
 * Scan: rewards are divided by `reward_denominator` (= f32(reward_scale+1e-8),
 * :106) on load -- and written back when write_scaled_rewards != 0, as the
 * reference does -- then for t = H-1..0
 *   delta = r[t] + (gamma*v[t+1] - v[t]);  adv[t] = delta + gamma_lambda*adv[t+1]
 * adv[H] = 0, ret[t] = adv[t] + v[t] for all H+1 columns (:116-117).
 * moments_out (3 doubles: count, sum, sum of squares of adv[:, :H]) feeds the
 * normalisation; all-reduce it across env shards before normalising.
 * layout: 0 = env-major (LDS-staged tiles), 1 = time-major (register scan).
 * rewards and adv_out / values and ret_out may not alias each other.
 * ---------------------------------------------------------------------- */
int rl8_gae_scan_f32(float *rewards, const float *values, float *adv_out, float *ret_out,
                     int64_t n, int64_t h, int layout, float gamma, float gamma_lambda,
                     float reward_denominator, int write_scaled_rewards, double *moments_out,
                     void *scratch, void *stream);

/* adv[:, :H] = (adv - mean) / (std + 1e-8), mean / unbiased std formed from
 * `moments` (device, 3 doubles) (:118-122).  One sample (N H = 1): the unbiased
 * std is 0/0 and the advantage comes back NaN, as the reference's does. */
int rl8_advantage_normalise_f32(float *adv, int64_t n, int64_t h, int layout,
                                const double *moments, void *stream);

/* The launch plan of rl8_gae_scan_f32 for a shape, a layout and an alignment (aligned16_all != 0: all four of
 * rewards, values, adv_out and ret_out are 16-byte aligned).  Host arithmetic only: no device is touched, and the
 * scan launches exactly what this reports.  Routes:
 *   TIME_VEC4      time-major, four envs per lane through 16-byte accesses (N % 4 == 0, aligned)
 *   TIME_VEC1      time-major, one env per lane
 *   ENV_PIPELINED  env-major, whole rows of odd H+1 <= 35 columns, aligned: tiles of 128 envs copied flat through
 *                  LDS, the next tile's rows requested before this tile's scan; grid capped at what is resident
 *   ENV_FLAT       env-major, whole rows of odd 37 <= H+1 <= 127 columns, aligned: flat 16-byte tile copies
 *   ENV_CHUNKED    env-major, everything else (even H+1, H+1 > 127 in chunks of 127 columns, misaligned
 *                  pointers): rows padded to an odd LDS stride and copied element by element
 * envs_per_block is the workgroup size of the env-major routes (one lane per env) and lanes x envs per lane of the
 * time-major ones; chunk, lds_stride (floats, odd) and lds_bytes (dynamic LDS of the launch) are 0 for time-major. */
#define RL8_GAE_TIME_VEC4 0
#define RL8_GAE_TIME_VEC1 1
#define RL8_GAE_ENV_PIPELINED 2
#define RL8_GAE_ENV_FLAT 3
#define RL8_GAE_ENV_CHUNKED 4
typedef struct {
  int route;
  int envs_per_block;
  int chunk;
  int lds_stride;
  int64_t lds_bytes;
  int grid;
} rl8_gae_plan_t;
int rl8_gae_plan(int64_t n, int64_t h, int layout, int aligned16_all, rl8_gae_plan_t *out /*host*/);

/* The kernel rl8_advantage_normalise_f32 launches (host arithmetic only), or a negative error code:
 * FLAT_VEC4 time-major with N H % 4 == 0 and adv 16-byte aligned, FLAT_VEC1 time-major otherwise, ENV_MAJOR. */
#define RL8_NORM_FLAT_VEC4 0
#define RL8_NORM_FLAT_VEC1 1
#define RL8_NORM_ENV_MAJOR 2
int rl8_advantage_normalise_route(int64_t n, int64_t h, int layout, int aligned16);

/* ---------------------------------------------------------------------- *
 * a-7  ppo_losses + approximate KL, forward AND backward
 *      src/rl8/nn/functional.py:259-363, algorithms/_feedforward.py:545-559
 * Per sample i: features, value[i], action[i], logp_old[i], adv[i], ret[i].
 * Writes grad_* = d(total)/d(input) * grad_scale (grad_scale =
 * 1 / (M_global * grad_accumulation_steps)), and loss_sums_out (device, 5
 * doubles): sum over samples of entropy, policy, vf terms, the sample count,
 * and the KL terms -- raw sums so that env shards combine with one all-reduce;
 * the host divides.  grad pointers may be NULL (forward only).
 * ---------------------------------------------------------------------- */
typedef struct {
  float clip_param;
  float dual_clip_param; /* <= 0: disabled (reference: None) */
  float entropy_coeff;
  float vf_clip_param;
  float vf_coeff;
  float grad_scale;
} rl8_ppo_hparams;

int rl8_ppo_loss_categorical_fwd_bwd_f32(const float *logits, const float *value,
                                         const int64_t *action, const float *logp_old,
                                         const float *adv, const float *ret, int64_t m, int a,
                                         int k, const rl8_ppo_hparams *hp /*host*/,
                                         float *grad_logits, float *grad_value,
                                         double *loss_sums_out, void *scratch, void *stream);

/* The same loss for 2 <= k <= RL8_MAX_WIDE_CLASSES classes with a * k < 2^31 (else RL8_ESIZE, before any launch):
 * one wave per sample over all a dimensions, lanes striding over the classes, every access of a wave a run of 256
 * contiguous bytes.  Per element the arithmetic is that of the generic kernel behind the entry above (expf / logf
 * normalisation, masked classes clamped to the lowest float in the entropy, the action clamped for the gather, the
 * same policy / value terms and gradient formula); sums and the maximum over a row run lane by lane and then across
 * lanes in a fixed xor butterfly.  A row of up to 1024 classes stays in registers between the passes, a longer one
 * is read again from cache.  Loss sums: one lane per wave adds each sample's four terms in double, then the fixed-
 * order block and grid reduction of the entry above (at most RL8_MAX_PARTIALS rows; RL8_LOSS_GRID_CAP caps the grid).
 * grad_logits == NULL (with grad_value == NULL): forward only. */
int rl8_ppo_loss_categorical_wide_fwd_bwd_f32(const float *logits, const float *value,
                                              const int64_t *action, const float *logp_old,
                                              const float *adv, const float *ret, int64_t m, int a,
                                              int k, const rl8_ppo_hparams *hp /*host*/,
                                              float *grad_logits, float *grad_value,
                                              double *loss_sums_out, void *scratch, void *stream);

int rl8_ppo_loss_normal_fwd_bwd_f32(const float *mean, const float *log_std, const float *value,
                                    const float *action, const float *logp_old, const float *adv,
                                    const float *ret, int64_t m, int a, int squashed,
                                    const rl8_ppo_hparams *hp /*host*/, float *grad_mean,
                                    float *grad_log_std, float *grad_value,
                                    double *loss_sums_out, void *scratch, void *stream);

/* ---------------------------------------------------------------------- *
 * a-8  Batcher gather                 src/rl8/_utils.py:211-225
 * index [M] int64 holds REFERENCE sample ids s = env*H + t (the flattening of
 * _feedforward.py:481).  Each of the `n_fields` sources is a buffer leaf with
 * element strides; the matching destination is a dense [M][row_elems] array.
 * Elements are 4 or 8 bytes wide (f32 / int64).
 * index = NULL (ABI 105): every sample of the buffer in order, s = 0 .. m - 1 with m = N h -- the sequence-major
 * copy of a time-major buffer that the recurrent algorithm trains on -- as a transposition through LDS tiles
 * (each byte read and written once, where the indexed kernel moves 6x that for 4-byte leaves).  A tile row holds 128
 * bytes, so consecutive fields go in groups that fit, one launch per group; a field of more than 128 bytes per row
 * closes the current group and takes the indexed kernels with the implicit index i.  m a multiple of h (RL8_ESIZE).
 * Every field is checked before the first launch.
 * ---------------------------------------------------------------------- */
typedef struct {
  const void *src;
  void *dst;
  int64_t env_stride;  /* in elements */
  int64_t time_stride; /* in elements */
  int32_t row_elems;   /* trailing elements per (env, t) cell */
  int32_t elem_bytes;  /* 4 or 8 (rl8_gather_sequences: 1 as well) */
} rl8_gather_field;

#define RL8_MAX_GATHER_FIELDS 8

int rl8_gather_minibatch(const int64_t *index, int64_t m, int64_t h,
                         const rl8_gather_field *fields /*host*/, int n_fields, void *stream);

/* The kernels rl8_gather_minibatch launches (host arithmetic only; `indexed` != 0: an index is given).  The pointers in
 * `fields` are judged for alignment and for NULL, never dereferenced.  routes_out / groups_out: n_fields ints each.
 *   GATHER_GENERAL    one lane per sample, element by element; all such fields share one launch
 *   GATHER_WIDE_ROWS  one wave per row in 16-byte pieces, one launch per field: rows of 256 bytes and up in whole
 *                     16-byte pieces, src and dst 16-byte aligned, env and time strides multiples of 16 bytes
 *   GATHER_TILED      index = NULL and at most 128 bytes per row: the tiled transposition, one launch per group of
 *                     consecutive fields; groups_out[f] is the field's group (0, 1, ...), -1 on the other routes
 * launches_out: tiled groups + wide fields + one if any field is general.  Error codes as rl8_gather_minibatch. */
#define RL8_GATHER_GENERAL 0
#define RL8_GATHER_WIDE_ROWS 1
#define RL8_GATHER_TILED 2
int rl8_gather_minibatch_plan(int indexed, int64_t m, int64_t h, const rl8_gather_field *fields /*host*/, int n_fields,
                              int *routes_out /*host*/, int *groups_out /*host*/, int *launches_out /*host*/);

/* Whole sequences, for the recurrent algorithm on dict observations: sequence q = env * (h / seq_len) + s is samples
 * q seq_len + j, j < seq_len (the reference's numbering); row i seq_len + j of every dst receives
 * src[env][s seq_len + j] for q = seq_index[i] (seq_index = NULL: q = i, every sequence in order, num_seqs of them).
 * elem_bytes 1, 4 or 8 (RL8_ECONFIG otherwise), any row_elems >= 1: a bool[3] leaf is 3 bytes per row and moves byte
 * by byte.  h a multiple of seq_len; src / dst aligned to elem_bytes (RL8_EALIGN). */
int rl8_gather_sequences(const int64_t *seq_index, int64_t num_seqs, int seq_len, int64_t h,
                         const rl8_gather_field *fields /*host*/, int n_fields, void *stream);

/* Padded rolling windows                src/rl8/views.py:54-123 (pad_last_sequence, pad_whole_sequence), 240-321
 * A field is a buffer leaf as in rl8_gather_field (elem_bytes 1, 4 or 8, any row_elems >= 1) and a window length
 * size = shift + 1 >= 1.  Cell j < size of the window that ends at step t of an env is step t' = t - (size - 1) + j:
 *   dst[i][j][:] = src[env][t'][:] and mask[i][j] = 0 where t' >= 0, zeros and mask[i][j] = 1 where t' < 0
 * (dst dense [rows][size][row_elems], mask dense [rows][size] bytes).  size = 1 is the plain gather, dst [rows]
 * [row_elems], and its mask is not read (NULL is fine); fields of different sizes share one launch, so the unwindowed
 * leaves of a dict observation ride along.
 * rl8_gather_windows: row i is sample s = index[i] (env = s / h, t = s % h), index = NULL: s = i, every sample in
 *   order; m rows.  What PaddedRollingWindow.apply_all followed by an index gives.
 * rl8_window_last: row i is env i at the given step t >= 0 (the caller keeps t within the leaf); n rows.  What
 *   pad_last_sequence gives on the leaf's first t + 1 steps.  Lanes run over envs within a window cell, so each source
 *   column of a time-major slab is read as one contiguous run.
 * RL8_ENULL: fields, a src or a dst is NULL.  RL8_ESIZE: m, h, n < 1, t < 0, n_fields outside 1 ..
 * RL8_MAX_GATHER_FIELDS, row_elems < 1, size < 1.  RL8_ECONFIG: elem_bytes not 1, 4 or 8; size > 1 without a mask.
 * RL8_EALIGN: src or dst not aligned to elem_bytes. */
typedef struct {
  const void *src;
  void *dst;
  uint8_t *mask;       /* [rows][size]; NULL when size == 1 */
  int64_t env_stride;  /* in elements */
  int64_t time_stride; /* in elements */
  int32_t row_elems;   /* trailing elements per (env, t) cell */
  int32_t elem_bytes;  /* 1, 4 or 8 */
  int32_t size;        /* shift + 1 */
} rl8_window_field;

int rl8_gather_windows(const int64_t *index, int64_t m, int64_t h, const rl8_window_field *fields /*host*/,
                       int n_fields, void *stream);
int rl8_window_last(int64_t t, int64_t n, const rl8_window_field *fields /*host*/, int n_fields, void *stream);

/* Masked sequence ops                    src/rl8/nn/functional.py:126-257 (masked_avg :147-179, masked_categorical_sample
 * :182-204, masked_log_softmax :207-228, masked_max :231-256)
 * They read what the window entries above write: inputs [rows][size][...] and a byte mask [rows][size].  Every array is
 * dense row-major f32; `mask` is [rows][t] or [rows][k] bytes (torch bool storage), NONZERO = VALID -- the reference's
 * convention for these functions, the opposite of the windows' padding mask -- and NULL means no mask.
 * rl8_masked_pool_f32, x [rows][t][e] -> out [rows][e], over t:
 *   RL8_POOL_AVG  out = (sum_t m x) / sum_t m.  The product m x is formed, so a NaN or inf in a padded cell gives NaN as
 *     mask * x does; a row without a valid cell gives 0 / 0 = NaN; mask == NULL: the mean over t.  The sum runs over
 *     t in ascending order.  Backward: dx = m (dout / count), one division and one multiplication by 0 or 1.
 *   RL8_POOL_MAX  padded cells read as -FLT_MAX; index_out [rows][e] is the first maximal t, the first NaN above
 *     everything (torch.argmax on the CPU); out the value there.  A row without a valid cell therefore gives -FLT_MAX at
 *     index 0.  Backward: dout at `index` unless that cell is padded (masked_fill's backward), zero elsewhere; every
 *     element of dx is written, `index` is only compared with t (no address is formed from it).
 *   Lanes run over the rows x e outputs with the t loop inside: no LDS, any rows, t, e >= 1.
 * rl8_masked_log_softmax_f32, x [rows][k] -> out [rows][k], along k: z = x + (m ? 0 : -FLT_MAX), the float addition of
 *   x + clamp(log(mask), FINFO.min, FINFO.max), then (z - max z) - log(sum exp(z - max z)) in torch's order; a row with
 *   every class masked comes out uniform for moderate x because the same additions are done, not by a special case.
 *   Backward, from the saved output: dx = dout - exp(out) sum_k dout.
 * rl8_masked_categorical_sample_f32: z as above; one draw of Categorical(logits = z): index = argmax_j p_j / q_j with
 *   p = softmax(z - logsumexp z), the first index on ties, q = noise [rows][k] (Exp(1) draws) or, noise == NULL, the
 *   build's Philox stream at (seed, row_offset + row, step, word j); value_out [rows] = z[index], the masked logit that
 *   x.gather(dim, samples) returns.  For k <= RL8_MAX_CLASSES the arithmetic and its order are those of
 *   rl8_categorical_sample_logp_f32 with a = 1: on the same z and address both pick the same classes.
 * Routes of the two [rows][k] families (rl8_masked_rows_route, host only; k < 1: RL8_ESIZE): one lane per row for
 *   k <= RL8_MAX_CLASSES, else one wave per row, strided over k, with xor-butterfly reductions (a fixed order).
 * RL8_ENULL: a required pointer (index_out / index in MAX mode too).  RL8_ESIZE: rows, t, e or k < 1.  RL8_ECONFIG: an
 * unknown mode.  RL8_EALIGN: a float pointer off 4 bytes, an index pointer off 8.  All before any launch. */
#define RL8_POOL_AVG 0
#define RL8_POOL_MAX 1
#define RL8_MASKED_ROWS_LANE 0 /* one lane per row, K <= RL8_MAX_CLASSES (64) */
#define RL8_MASKED_ROWS_WAVE 1 /* one wave per row, strided over K, cross-lane reductions in a fixed order */
int rl8_masked_rows_route(int k);
int rl8_masked_pool_f32(const float *x, const uint8_t *mask, int64_t rows, int t, int e, int mode,
                        float *out /*[rows][e]*/, int64_t *index_out /*[rows][e], MAX only*/, void *stream);
int rl8_masked_pool_backward_f32(const float *dout, const uint8_t *mask, const int64_t *index, int64_t rows, int t, int e,
                                 int mode, float *dx /*[rows][t][e]*/, void *stream);
int rl8_masked_log_softmax_f32(const float *x, const uint8_t *mask, int64_t rows, int k, float *out, void *stream);
int rl8_masked_log_softmax_backward_f32(const float *dout, const float *out, int64_t rows, int k, float *dx, void *stream);
int rl8_masked_categorical_sample_f32(const float *x, const uint8_t *mask, const float *noise /*q [rows][k] or NULL*/,
                                      int64_t rows, int k, uint64_t seed, uint64_t step, int64_t row_offset,
                                      float *value_out /*[rows]*/, int64_t *index_out /*[rows]*/, void *stream);

/* Short-sequence attention: the core of nn.MultiheadAttention, softmax(q k^T scale + masks) v with scale = 1 / sqrt(d),
 * forward and backward (rl8_amd/csrc/attention_kernels.hip).  The projections in front of it and behind it stay the
 * caller's.
 * Operands, all f32: q rows [b][tq], k and v rows [b][tk]; each has its own base pointer and a row stride in floats
 *   (q_stride; kv_stride for both k and v), and head h of a row is the d floats at h d.  A packed [b][t][3 heads d]
 *   projection is read in place as (p, p + e, p + 2e) with strides 3e, a [b][tk][2e] one as (p, p + e) with 2e.
 *   key_padding [b][tk] bytes (torch bool storage), NONZERO = PADDED, or NULL -- torch's key_padding_mask and what
 *   rl8_window_last / rl8_gather_windows write; the OPPOSITE of the rl8_masked_* entries' mask, where nonzero is valid.
 *   bias [tq][tk] f32 or NULL is added to the scaled scores and may hold -inf.
 * rl8_attention_f32: out [b][tq][heads d] dense, out[b][q][h d + c] = sum_t P[q, t] v[b][t][h d + c] with
 *   P = softmax_t(scale q.k + bias), padded keys at -inf; lse [b][heads][tq] = log sum_t exp(s) when a pointer is given.
 *   A query with no admissible key (every key padded or at -inf) has P = 0: out = 0 and lse = +inf, not NaN -- what
 *   torch's math backend returns through nn.MultiheadAttention.
 * rl8_attention_backward_f32, from dout [b][tq][heads d] dense and the forward's out and lse: P = exp(s - lse),
 *   delta_q = dout[q].out[q], dv[t] = sum_q P[q, t] dout[q], dS[q, t] = P[q, t] (dout[q].v[t] - delta_q),
 *   dq[q] = scale sum_t dS[q, t] k[t], dk[t] = scale sum_q dS[q, t] q[q].  Two launches in order on `stream`: dq (which
 *   leaves delta in delta_workspace, [b][heads][tq] floats), then dk and dv.  Every element of dq (rows of dq_stride
 *   floats), dk and dv (rows of dkv_stride floats; the gaps between rows are left alone) is written; lse = +inf makes
 *   every gradient of and through a query without an admissible key exactly 0.  No atomics and no reduction across
 *   lanes: the same bits on every run.
 * One lane per (b, q, h) resp. (b, t, h), the loop over the other sequence inside it; no LDS.  Envelope
 *   (rl8_attention_supports, host only: 1 inside, 0 outside, RL8_ESIZE for an argument < 1): tq, tk <= 64, d <= 16,
 *   any heads and b.
 * RL8_ENULL: a required pointer (everything but key_padding, bias and the forward's lse).  RL8_ESIZE: b, tq, tk, heads
 *   or d < 1, a stride below heads d.  RL8_EALIGN: a float pointer off 4 bytes.  RL8_ECONFIG: a shape outside
 *   rl8_attention_supports.  All before any launch. */
int rl8_attention_supports(int tq, int tk, int heads, int d);
int rl8_attention_f32(const float *q, int64_t q_stride, const float *k, const float *v, int64_t kv_stride,
                      const uint8_t *key_padding, const float *bias, int64_t b, int tq, int tk, int heads, int d,
                      float *out, float *lse /*may be NULL*/, void *stream);
int rl8_attention_backward_f32(const float *q, int64_t q_stride, const float *k, const float *v, int64_t kv_stride,
                               const uint8_t *key_padding, const float *bias, const float *out, const float *lse,
                               const float *dout, int64_t b, int tq, int tk, int heads, int d, float *dq,
                               int64_t dq_stride, float *dk, float *dv, int64_t dkv_stride, float *delta_workspace,
                               void *stream);

/* The fused feedforward block of the attention modules (rl8_amd/csrc/feedforward_kernels.hip), per row of x [rows][f]:
 *   n   = LayerNorm_f(x; gamma, beta, eps)      biased variance from the centred values, rstd = 1 / sqrt(var + eps)
 *   out = (residual ? x : 0) + w2 relu(w1 n + b1) + b2
 * with w1 [hidden][f] and w2 [f][hidden] as nn.Linear holds them, gamma, beta, b2 [f], b1 [hidden]; all f32 and dense.
 * relu hands a NaN through; its gradient's gate is z > 0 (closed at exactly 0).
 * rl8_feedforward_f32: one lane per row, the hidden vector in registers only.
 * rl8_feedforward_backward_f32, from x and dout [rows][f] alone (n and the pre-activations are formed again, by the
 *   forward's own operations in the forward's order, so the gates agree bit for bit): dx [rows][f] (dout added when
 *   `residual`), dgamma, dbeta [f], dw1 [hidden][f], db1 [hidden], dw2 [f][hidden], db2 [f].  Every output may be NULL
 *   and is then not formed; with no output at all nothing is launched.  The parameter gradients are sums of per-workgroup
 *   and per-wave f32 partial sums over row slices that depend on (rows, f, hidden) only, left in `workspace`
 *   (rl8_feedforward_workspace_floats(rows, f, hidden) floats, contents undefined before and after; required when a
 *   parameter gradient is asked for, untouched otherwise) and added up in f64 in a fixed order by the last launch: no
 *   atomics, the same bits on every run.  Launches in order on `stream`: dx (which also leaves the dgamma / dbeta
 *   partials), the dw1 / db1 / dw2 / db2 partials, the sum.
 * Envelope (rl8_feedforward_supports, host only: 1 inside, 0 outside, RL8_ESIZE for an argument < 1): f <= 32,
 *   hidden <= 256, any rows.  rl8_feedforward_limits writes {grid cap, lanes per workgroup} of the row-per-lane kernels
 *   and {grid cap, rows staged per workgroup} of the dw kernel -- beyond cap x rows a workgroup strides -- into
 *   limits[0..3].  rl8_feedforward_workspace_floats: RL8_ESIZE / RL8_ECONFIG as below.
 * RL8_ENULL: a required pointer (every input; the workspace when a parameter gradient is wanted).  RL8_ESIZE: rows, f or
 *   hidden < 1.  RL8_EALIGN: a pointer off 4 bytes.  RL8_ECONFIG: a shape outside rl8_feedforward_supports.  All before
 *   any launch. */
int rl8_feedforward_supports(int f, int hidden);
int rl8_feedforward_limits(int *limits /*host, [4]*/);
int64_t rl8_feedforward_workspace_floats(int64_t rows, int f, int hidden);
int rl8_feedforward_f32(const float *x, const float *gamma, const float *beta, float eps, const float *w1,
                        const float *b1, const float *w2, const float *b2, int64_t rows, int f, int hidden, int residual,
                        float *out, void *stream);
int rl8_feedforward_backward_f32(const float *x, const float *dout, const float *gamma, const float *beta, float eps,
                                 const float *w1, const float *b1, const float *w2, int64_t rows, int f, int hidden,
                                 int residual, float *dx, float *dgamma, float *dbeta, float *dw1, float *db1, float *dw2,
                                 float *db2, float *workspace, void *stream);

/* The same gather for a buffer that is shuffled many times per step()
 * (num_sgd_iters x num_minibatches): rl8_pack_samples lays the fields of every
 * sample side by side once -- packed[s][...] for the reference's sample id
 * s = env*H + t, t < h, row_words 4-byte words per sample (a multiple of 4, at most
 * 32, at least the sum of the fields' row words, fields in the order given; `dst` of the
 * fields is ignored) -- and rl8_gather_packed then reads one row per sample
 * (`src`, `env_stride`, `time_stride` ignored): one random sector per sample
 * instead of one per field. */
int rl8_pack_samples(const rl8_gather_field *fields /*host*/, int n_fields, int64_t n, int64_t h,
                     void *packed, int row_words, void *stream);
int rl8_gather_packed(const int64_t *index, int64_t m, const void *packed, int row_words,
                      const rl8_gather_field *fields /*host*/, int n_fields, void *stream);

/* The launch of the tiled transposition behind rl8_pack_samples and rl8_gather_minibatch(index = NULL) (host arithmetic
 * only): a workgroup moves tiles of 64 envs x tile_steps timesteps through lds_bytes of dynamic LDS (rows of
 * row_words + 1 words); `tiles` of them, taken by `grid` workgroups in a strided loop.  row_words a multiple of 4 in
 * 4 .. 32 (RL8_ESIZE). */
typedef struct {
  int tile_steps;
  int lds_bytes;
  int64_t tiles;
  int grid;
} rl8_pack_plan_t;
int rl8_pack_plan(int64_t n, int64_t h, int row_words, rl8_pack_plan_t *out /*host*/);

/* ---------------------------------------------------------------------- *
 * Dict (Composite) observations: rollout bookkeeping and the AlgoTrading env
 *      src/rl8/algorithms/_feedforward.py:378-393, examples/algotrading/env.py:23-183
 * rl8_rollout_scatter_leaves_f32: what rl8_rollout_scatter_f32 does for action / logp / value / reward / rdr, and
 * 1 .. RL8_MAX_GATHER_FIELDS observation leaves copied into their t+1 columns in the same launch.  A leaf is n rows
 * of row_bytes bytes (any positive count: 1 for bool, 8 for int64, 4 d for f32[d]), source and destination both
 * contiguous; copied 16 bytes at a time where n * row_bytes and both pointers allow, else 8, 4 or 1.  The float and
 * action pointers are 4-byte aligned (RL8_EALIGN); action_row_bytes a multiple of 4.
 * ---------------------------------------------------------------------- */
typedef struct {
  const void *src;
  void *dst;
  int64_t row_bytes;
} rl8_scatter_leaf;

int rl8_rollout_scatter_leaves_f32(const void *action, int64_t action_row_bytes, const float *logp,
                                   const float *value, const float *reward,
                                   const rl8_scatter_leaf *leaves /*host*/, int n_leaves, void *action_col,
                                   float *logp_col, float *value_col, float *reward_col, const float *rdr_t,
                                   float *rdr_t1, float gamma, int64_t n, void *stream);

/* AlgoTrading: state SoA [9][N] fp32 in place, rows invested (0 / 1), position, f, k_cyclic, k_market, t, price,
 * LOG_CHANGE(price), LOG_CHANGE(price, position).  The observation is four leaves: mask [N][3] bytes (hold, buy,
 * sell allowed), invested [N] int64 and the two log-changes [N] f32 each.
 * reset (:85-93): f ~ U(0, f_bounds), k_* ~ U(-bounds, bounds), t in 0..9, price ~ U(100, 10000) from the build's
 * Philox stream, not invested, position 0, mask (1, 1, 0); the four leaf outputs together or all NULL.
 * step (:131-183): action [N] int64 in {0 hold, 1 buy, 2 sell}, the mask is not enforced (as in the reference);
 * price' = price * ((1 + k_market) * (1 + k_cyclic * sin(t' f))), accurate sin / log, one rounding per operation.
 * invested / action pointers 8-byte aligned, floats 4-byte (RL8_EALIGN). */
int rl8_algotrading_reset_f32(float *state, int64_t n, float f_bounds, float k_cyclic_bounds, float k_market_bounds,
                              uint64_t seed, uint64_t reset_count, int64_t env_offset, uint8_t *mask_out,
                              int64_t *invested_out, float *log_change_out, float *log_change_position_out,
                              void *stream);
int rl8_algotrading_step_f32(float *state, const int64_t *action, uint8_t *mask_out, int64_t *invested_out,
                             float *log_change_out, float *log_change_position_out, float *reward_out, int64_t n,
                             void *stream);
/* Fused per-timestep kernel (K = 3 sampler on the model's masked logits + the step + bookkeeping), arguments as
 * rl8_rollout_step_cartpole_f32 with the four leaves' t+1 columns in place of obs_col_next. */
int rl8_rollout_step_algotrading_f32(const float *logits, const float *value, const float *noise, float *state,
                                     int64_t *action_col, float *logp_col, float *value_col, float *reward_col,
                                     uint8_t *mask_next, int64_t *invested_next, float *log_change_next,
                                     float *log_change_position_next, const float *rdr_t, float *rdr_t1, float gamma,
                                     int64_t n, uint64_t seed, uint64_t step, int64_t env_offset, int deterministic,
                                     void *stream);

/* ---------------------------------------------------------------------- *
 * N1  Default policy / value tower, fused
 *      src/rl8/models/_feedforward.py:336-375 (DefaultDiscreteModel),
 *      :263-310 (DefaultContinuousModel), src/rl8/nn/modules/mlp.py:12-52
 * One tower = Linear(d_in, 256) ReLU Linear(256, 256) ReLU Linear(256, n_out),
 * fp32 throughout (layer 2 on v_mfma_f32_32x32x2_f32), activations kept on
 * chip.  d_in <= 16, n_out <= 8.  Weights in torch.nn.Linear layout
 * ([out][in] row-major); the 256x256 matrix is passed in MFMA fragment order,
 * produced by rl8_mlp_pack_w2_f32 (transposed = 0 for the forward pass and the
 * weight-gradient pass, 1 for the data-gradient pass of the backward).
 * ---------------------------------------------------------------------- */
int rl8_mlp_pack_w2_f32(const float *w2 /*[256][256]*/, float *w2_packed /*[65536]*/,
                        int transposed, void *stream);

/* out [M][n_out] = tower(x [M][d_in]).  For training, save_h1 / save_h2
 * ([M][256] each, 16-byte aligned) receive the post-ReLU activations; both NULL
 * for inference. */
int rl8_mlp_tower_forward_f32(const float *x, int64_t m, int d_in, const float *w1,
                              const float *b1, const float *w2_packed, const float *b2,
                              const float *w3, const float *b3, int n_out, float *out,
                              float *save_h1, float *save_h2, void *stream);

/* The same forward with the 256x256 product as THREE fp16 MFMAs per 16 k: each
 * activation row of h1 is scaled by a power of two chosen from a bound on its
 * magnitude (max|b1| + sum_i |x_i| max|w1[:, i]|, placed at 2^14) and W2 by one
 * power of two for the matrix, so both operands sit in the upper fp16 exponent
 * range; each is then split into hi = fp16(v), lo = fp16(v - hi) (22 significand
 * bits) and lo.hi + hi.lo + hi.hi is accumulated in fp32; the epilogue multiplies
 * by the inverse powers of two (exact).  Inputs, outputs and saved activations are fp32
 * exactly as for rl8_mlp_tower_forward_f32 (h1 bit-identical at d_in <= 3 and equal to fp32 rounding above -- there layer 1
 * runs on the matrix pipe too; out / h2 equal to fp32 rounding).
 * save_h1 may be NULL while save_h2 is given: the plane backward kernels recompute h1 from the
 * observations and never read it.  save_gate2 (optional) [M][8] words receives the ReLU gate of
 * layer 2, bit j of row s = (h2[s][j] > 0): the data-gradient kernels need only that bit of h2
 * (32 B per row instead of 1 KiB), and it may be given WITHOUT save_h2 (rank-one heads: see
 * rl8_mlp_wgrad_gate_bits_f32).  Widths (round 5): any d_in <= 8 with n_out <= 8, and d_in 9..16 with n_out <= 4
 * (rl8_mlp_forward_f16_supports) -- the
 * kernels are compiled for width CLASSES d_in {1, 2, 3, 8, 16} x n_out {1, 2, 4, 8} and a class serves every run-time
 * width it holds (weights past d_in zero, observations past d_in not loaded, output rows past n_out zero and not stored;
 * class 8, d_in = 4..8, forms z1 = W1 x as ONE 16x16x32 MFMA per sixteen units and rows that holds the four fp16 plane
 * products of eight inputs; class 16 chains two of them) -- else RL8_ESIZE: wider towers run rl8_mlp_tower_forward_f32.  The plane BACKWARD entries
 * below serve d_in 1..5 x n_out 1..4 (rl8_mlp_backward_f16_supports; the weight-gradient kernels are compiled per width,
 * the data-gradient kernels per class -- d_in 4, 5 in class 8, which recomputes the forward's z1 product bit for bit and
 * forms dW1 / db1 as MFMAs over the wave's rows); a tower inside the forward's envelope but outside theirs is trained
 * through the fp32-MFMA data gradient + bf16-plane weight gradient (save_h1 given).  (The bf16-plane forward / data-gradient
 * entries of rounds 1-2, rl8_mlp_tower_{forward,backward}_split_f32, were removed in round 3.)
 * w2_f16 (rl8_mlp_f16_packed_bytes() bytes:
 * two fp16 planes in fragment order + {scale, 1/scale}) comes from
 * rl8_mlp_pack_w2_f16.  The fragment order depends on `transposed`: 0 (this forward; since round 3 a kernel of
 * v_mfma_f32_16x16x32_f16, a wave per 32 rows) packs 16-byte unit ((hs*8 + ct)*2 + plane)*64 + lane with
 * B(col = 16 (8 (hs & 1) + ct) + (lane & 15), k = 32 (hs >> 1) + 8 (lane >> 4) + e), e = 0..7; 1 (the data-gradient
 * kernels, 32x32x16) keeps unit ((s*8 + ct)*2 + plane)*64 + lane with B(col = 32 ct + (lane & 31),
 * k = 16 s + 8 (lane >> 5) + e) of the transposed matrix.  A pack made for one is not valid for the other.
 * Replaces the same reference call sites
 * (rl8/models/_feedforward.py:115-132 forward of the 256-256 towers). */
int64_t rl8_mlp_f16_packed_bytes(void);
int rl8_mlp_forward_f16_supports(int d_in, int n_out);
int rl8_mlp_pack_w2_f16(const float *w2 /*[256][256]*/, int transposed, void *w2_f16, void *stream);
int rl8_mlp_tower_forward_f16_f32(const float *x, int64_t m, int d_in, const float *w1,
                                  const float *b1, const void *w2_f16, const float *b2,
                                  const float *w3, const float *b3, int n_out, float *out,
                                  float *save_h1, float *save_h2, uint32_t *save_gate2, void *stream);

/* A head of TWO outputs whose gradients are exact negatives of each other (a two-way categorical:
 * rl8_ppo_loss_categorical_fwd_bwd_f32 emits them so) has dZ2 = gate * dOut[.][0] * (W3[0] - W3[1]):
 * the weight gradient then needs one binary operand and three plane products per 16 samples
 * instead of six (as for single-output towers, which rl8_mlp_wgrad_fused_split_f32 handles by
 * itself).  rl8_mlp_dout_pair_check leaves 0 in *flag_out (device int) iff dout [m][2] has
 * dout[s][1] == -dout[s][0] bit for bit in every row; only then may rl8_mlp_wgrad_fused_pair_f32
 * replace rl8_mlp_wgrad_fused_split_f32(..., n_out = 2, ...): same arguments, same outputs. */
int rl8_mlp_dout_pair_check(const float *dout /*[m][2]*/, int64_t m, int *flag_out /*device*/, void *stream);
int rl8_mlp_wgrad_fused_pair_f32(const float *h2, const float *dout, const float *x, const float *w1,
                                 const float *b1, const float *w3, int64_t m, int d_in,
                                 float *workspace, float *dw2_out, float *partials, void *stream);

/* Rank-one heads without h2.  rl8_mlp_tower_forward_f16_f32 with save_h2 = NULL and save_gate2 given stores the
 * gate bits alone (32 bytes per row instead of 1 KiB, none of the h2 store path); the data gradient's gate mode
 * never needed h2; and the weight gradient's only other use of it, dW3 = dOut^T h2, follows from the sums M the
 * gate-plane kernel forms anyway (dW2[j][i] = W3[j] M[j][i]):  with h2 = gate * (h1 W2^T + b2),
 *   dW3[j] = sum_i W2[j][i] M[j][i] + b2[j] * sum_s gate[s][j] dOut[s].
 * rl8_mlp_wgrad_gate_bits_f32: outputs of rl8_mlp_wgrad_fused_split_f32 (n_out = 1) / _pair_f32 (n_out = 2, after
 * a clean rl8_mlp_dout_pair_check) from gate2 [m][8] instead of h2; w2 [256][256] and b2 [256] are the layer's
 * own parameters.  In fp32 the result differs from the direct sum by the rounding the forward's own 256-term dot
 * products put into h2 -- what another fp32 evaluation of h2 (the reference's) differs from this one by.
 * Since round 3 the second operand dOut[s] * h1[s][i] is carried as two fp16 planes times a power of two per column i
 * (two plane products per 16 rows; the column bounds come from one pass over dout and x in front of the first
 * segment and live in the 256 bytes behind the slabs of `workspace`); RL8_WGRAD_GATE_PLANES=bf16 in the environment
 * selects the three exact bf16 planes of round 2.  dW2 stays within the fp32 kernels' error against the tensor's
 * largest entry; an entry made only of rows 2^17 below its column's bound keeps ~1e-5 of its own size.
 * RL8_WGRAD_PHASES=inphase (read once per process) gives every wave of the fp16-plane kernel the one phase order it
 * had before half of them were set to produce first (d_in <= 2): same bits, for A/B timing and the equality test. */
int rl8_mlp_wgrad_gate_bits_f32(const uint32_t *gate2, const float *dout, const float *x, const float *w1,
                                const float *b1, const float *w2, const float *b2, const float *w3,
                                int64_t m, int d_in, int n_out, float *workspace, float *dw2_out,
                                float *partials, void *stream);

/* The data-gradient half of the fused backward pass on the same fp16 planes (three MFMAs
 * per 16 k): no dZ2 store; instead of the saved h1 the kernel takes layer 1 itself (w1, b1) and recomputes
 * the ReLU gate h1 > 0 <=> b1 + x . w1 > 0 with the forward pass's own fma chain; gate2 -- the
 * forward's save_gate2 -- is required; w2t_f16 from rl8_mlp_pack_w2_f16(..., transposed = 1).
 * dZ2 rows are scaled by a power of two from the row bound sum_q |dOut_q| max|W3_q|, W2^T
 * by the pack's, both undone on the accumulators.  Fills [dW1 | db1] of `*partial_rows_out`
 * partial rows (layout of rl8_mlp_tower_backward_f32); the caller follows with
 * rl8_mlp_wgrad_fused_split_f32 for dW2 and the head segments.
 * Replaces the autograd backward of the 256-256 towers
 * (rl8/algorithms/_feedforward.py:374-386 loss.backward()). */
int rl8_mlp_backward_f16_supports(int d_in, int n_out);
int rl8_mlp_tower_backward_f16_f32(const float *x, const float *w1, const float *b1, const float *dout,
                                   int64_t m, int d_in, const void *w2t_f16, const float *w3, int n_out,
                                   float *partials, int *partial_rows_out /*host*/, const uint32_t *gate2,
                                   void *stream);

/* Gate mode of the fp16 data-gradient kernel, for heads whose dZ2 is gate * d[s] * w3e[k] -- n_out = 1
 * (w3e = W3[0]), or n_out = 2 with dout[s][1] == -dout[s][0] in every row (rl8_mlp_dout_pair_check;
 * w3e = W3[0] - W3[1], d = dout[.][0]):  dH1[s][i] = d[s] * sum_k gate[s][k] * (w3e[k] W2[k][i]).
 * The gate is the A operand (one fp16 plane of zeros and ones straight from the gate bits), B the two
 * planes of w3e[k] W2[k][i] from rl8_mlp_pack_w2_f16_gate (rl8_mlp_f16_packed_bytes() bytes; re-made
 * when W2 or W3 change): two plane products per 16 k instead of three.  Other arguments, partial rows
 * and the follow-up weight-gradient call as rl8_mlp_tower_backward_f16_f32. */
int rl8_mlp_pack_w2_f16_gate(const float *w2 /*[256][256]*/, const float *w3 /*[n_out][256]*/, int n_out,
                             void *w2t_gate, void *stream);
int rl8_mlp_tower_backward_gate_f16_f32(const float *x, const float *w1, const float *b1, const float *dout,
                                        int64_t m, int d_in, const void *w2t_gate, int n_out,
                                        float *partials, int *partial_rows_out /*host*/,
                                        const uint32_t *gate2, void *stream);

/* Backward of one tower ("dgrad" half): given dOut [M][n_out] and the saved
 * activations h1 / h2, writes dZ2 [M][256] (input of rl8_mlp_wgrad_f32, which
 * forms dW2 = dZ2^T h1) and `*partial_rows_out` rows (<= rl8_mlp_backward_max_rows()) of
 * rl8_mlp_backward_partial_floats(d_in, n_out) floats each into `partials`:
 *   [dW1 (256*d_in) | db1 (256) | db2 (256) | dW3 (n_out*256) | db3 (n_out)]
 * whose column sums are the parameter gradients.  w2t_packed is
 * rl8_mlp_pack_w2_f32(..., transposed = 1).  partial_rows_out is a host pointer. */
int64_t rl8_mlp_backward_partial_floats(int d_in, int n_out);
int rl8_mlp_backward_max_rows(void);
int rl8_mlp_tower_backward_f32(const float *x, const float *h1, const float *h2,
                               const float *dout, int64_t m, int d_in, const float *w2t_packed,
                               const float *w3, int n_out, float *dz2_out, float *partials,
                               int *partial_rows_out /*host*/, void *stream);

/* dW2 (+)= dZ2^T h1 on bf16 planes, with h1 = relu(x W1^T + b1) recomputed from the
 * observations instead of read back (workspace: rl8_mlp_wgrad_workspace_bytes()). */
int rl8_mlp_wgrad_split_f32(const float *dz2, const float *x, const float *w1, const float *b1,
                            int64_t m, int d_in, float *workspace, float *dw2_out, int accumulate,
                            void *stream);

/* The fused backward: rl8_mlp_tower_backward_f16_f32 followed by this call, whose weight-gradient
 * kernel re-forms dZ2 = (dOut x W3) * (h2 > 0) and h1 itself (thread = column) and
 * accumulates the head gradients on the way.  dw2_out [256][256] receives dW2; the
 * head segments [db2 | dW3] of `partials` (the same buffer and row count the first
 * call reported) are filled and the db3 segment is zeroed: db3 = the column sums of
 * dOut, which the caller forms itself.  Widths: rl8_mlp_backward_f16_supports.  Since round 3 the
 * products run on two fp16 planes per operand, each scaled by a power of two per column of the
 * output it indexes (three plane products per 16 rows; RL8_WGRAD_PLANES=bf16: the six bf16 ones).
 * Inputs longer than 2^23 rows are summed in 2^23-row segments, in order (this call and
 * rl8_mlp_wgrad_split_f32): the fp32 accumulation chains do not grow with m. */
int rl8_mlp_wgrad_fused_split_f32(const float *h2, const float *dout, const float *x, const float *w1,
                                  const float *b1, const float *w3, int64_t m, int d_in, int n_out,
                                  float *workspace, float *dw2_out, float *partials, void *stream);

/* Weight gradient of the 256x256 layer: dw2_out [256][256] (+)= dZ2^T h1 over M
 * rows (fp32 MFMA; per-workgroup partial slabs in `workspace`, summed in a fixed
 * order).  workspace: rl8_mlp_wgrad_workspace_bytes() bytes (one 256 x 256 slab per CU + 256 bytes for the
 * fp16-plane kernels: operand bounds, the guard's sample counts and decision -- written per call -- and, in the
 * last 128 bytes, two uint32 counters that only grow: [32] calls that consulted the guard, [33] calls it sent to
 * the exact bf16 planes).  No initialisation needed; zero the last 256 bytes once if the counters are to be read.
 *
 * The guard (round 4): the fp16 planes of rl8_mlp_wgrad_fused_split_f32 / rl8_mlp_wgrad_gate_bits_f32 carry 22 bits
 * of a term within 2^-17 of its column's bound.  Each call samples dOut (one KiB in sixteen) behind the pass that
 * takes the bounds; if more than 2^-7 of the non-zero entries lie below 2^-12 of the largest, the call's sums are
 * formed on three exact bf16 planes instead (both generations are launched, one leaves at once: no host round
 * trip).  RL8_WGRAD_PLANES / RL8_WGRAD_GATE_PLANES = bf16: always the exact planes; = f16!: never (diagnostics). */
int64_t rl8_mlp_wgrad_workspace_bytes(void);
int rl8_mlp_wgrad_f32(const float *dz2, const float *h1, int64_t m, float *workspace,
                      float *dw2_out, int accumulate, void *stream);
/* The same product over rows that sit `pitch` floats apart (multiples of 4,
 * >= 256): e.g. one gate of an LSTM's [M][4][256] gate gradients, pitch 1024. */
int rl8_mlp_wgrad_strided_f32(const float *dz2, int64_t dz2_pitch, const float *h1, int64_t h1_pitch,
                              int64_t m, float *workspace, float *dw2_out, int accumulate,
                              void *stream);
/* The same product on the bf16 matrix pipe (fp32-accurate bf16-plane products, both
 * operands prefetched from memory): the LSTM's dW_hh[q] = dG_q^T h_{t-1}
 * (autograd of src/rl8/models/_recurrent.py:312-333).  With x / colsums it also leaves, per
 * workgroup, the column sums  sum_rows dZ[row][col] * x[row][i]  and  sum_rows dZ[row][col]:
 * the same gate's dW_ih and bias gradients, from the dZ values its producers hold anyway
 * (d_in in {1, 2, 3, 5}; the caller adds the *colsum_rows_out rows in order). */
int rl8_mlp_wgrad_split_strided_f32(const float *dz, int64_t dz_pitch, const float *h, int64_t h_pitch,
                                    int64_t m, float *workspace, float *dw_out, int accumulate,
                                    const float *x /* [m][d_in] dense, or NULL */, int d_in,
                                    float *colsums /* [<= 256 rows][256 * (d_in + 1)], or NULL */,
                                    int *colsum_rows_out, void *stream);

/* ---------------------------------------------------------------------- *
 * a-9, second generation: ONE LSTM timestep with the recurrent product as an
 *      fp32-accurate product on the fp16 matrix pipe (the towers' two-plane scheme: |h| < 1, so
 *      the state's planes are those of h * 2^14; W_hh carries one power of two for the matrix)
 *      src/rl8/models/_recurrent.py:312-333 (the nn.LSTM call of the default recurrent
 *      models), algorithms/_recurrent.py:385-431 (its per-timestep use in collect())
 * The time loop is the caller's: one launch per timestep, states exchanged through HBM.
 *
 * rl8_lstm_pack_split: torch-layout parameters -> `packed` (rl8_lstm_split_packed_bytes()
 *   bytes: W_hh as two fp16 planes in the kernel's fragment order + its power of two) and `wb`
 *   (rl8_lstm_split_wb_floats() floats: [1024][8] = [w_ih row | 0.. | b_ih + b_hh]).
 * rl8_lstm_split_state: h [B][pitch] fp32 -> `planes` (rl8_lstm_split_state_bytes(B) bytes),
 *   the step kernel's A operand.  rl8_lstm_split_state_bound: the same, and max |h| over the rows as a float's bit
 *   pattern in *bound_out (what rl8_lstm_wgrad_f16_f32 takes as h_bound for the first timestep).
 *   Envelope.  h may be a caller's own (torch.nn.LSTM takes any h_0), so both entries take max |h| over the FINITE
 *   entries of the call while they make the planes of h * 2^14, and a second launch keeps those while that maximum is
 *   below 2 (an LSTM's own outputs: the bits are those of ABI 107, and h is read once) or makes them again as those of
 *   h * 2^(14 - e), max < 2^e, from 2 up to FLT_MAX.  The
 *   factor, its inverse and the two maxima are the last sixteen bytes of `planes` (counted in
 *   rl8_lstm_split_state_bytes).  One factor per call: an entry far below the call's maximum keeps the two
 *   planes' 22 bits while it is above 2^(e - 17) and an absolute step of 2^(e - 38) below that (fp16's subnormal step
 *   in the low plane; e = 0 under 2), so rows of 0.3 beside a row of 2^10 lose nothing, and entries under 2^(e - 39)
 *   read as zero: 256 of them are less than 2^(e - 31) * max |W_hh| of a pre-activation.
 *   A row holding an infinity or a NaN gives non-finite planes for that row only, and NaN h_t, c_t in that row
 *   (torch does the same for a NaN; one infinity it lets saturate the row's gates instead); *bound_out then holds that entry's bit pattern.
 * rl8_lstm_step_split_f32: x row r at x + r * x_pitch (d_in floats); h_planes of h_{t-1};
 *   c_prev row r at c_prev + r * c_prev_pitch; writes h_t, c_t rows at the given pitches
 *   (floats) and, when `gates` is not NULL, the post-activation gates i, f, g, o as
 *   [4][256] per row at gates + r * gates_pitch (what rl8_lstm_backward_f32 reads); when
 *   `planes_out` is not NULL, h_t also as fp16 planes (rl8_lstm_split_state's layout) for the
 *   next timestep's call, so that only the first step of a sequence needs rl8_lstm_split_state.
 *   `h_planes` must come from rl8_lstm_split_state[_bound] or from an earlier step's `planes_out`: the kernel takes
 *   the inverse of the planes' factor from the sixteen bytes behind them, and writes 2^14, 2^-14 behind `planes_out`
 *   (|h_t| < 1).  With that any finite h_0 is inside the envelope while max |h_0| * max |W_hh| < 2^126 (the two
 *   inverses meet in one fp32 factor; past that pre-activations of 2^126 and more are formed, which torch saturates
 *   and this kernel may turn into NaN); W_hh's own power of two holds down to a largest weight of 2^-96.  The factor
 *   sits at the offset of b's planes: planes made for one b are not the planes of another b.
 *   d_in in {1, 2, 3, 5} (rl8_lstm_split_supports); other widths keep rl8_lstm_forward_f32.
 * ---------------------------------------------------------------------- */
int rl8_lstm_split_supports(int d_in);
int64_t rl8_lstm_split_packed_bytes(void);
int64_t rl8_lstm_split_wb_floats(void);
int64_t rl8_lstm_split_state_bytes(int64_t b);
int rl8_lstm_pack_split(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                        int d_in, void *packed, float *wb, void *stream);
int rl8_lstm_split_state(const float *h, int64_t pitch, int64_t b, void *planes, void *stream);
int rl8_lstm_split_state_bound(const float *h, int64_t pitch, int64_t b, void *planes, uint32_t *bound_out,
                               void *stream);
int rl8_lstm_step_split_f32(const float *x, int64_t x_pitch, int d_in, const void *h_planes,
                            const float *c_prev, int64_t c_prev_pitch, const void *w_planes,
                            const float *wb, int64_t b, float *h_out, int64_t h_out_pitch, float *c_out,
                            int64_t c_out_pitch, float *gates, int64_t gates_pitch,
                            void *planes_out /* h_t as planes for the next step (another buffer than h_planes), or NULL */,
                            void *stream);

/* ---------------------------------------------------------------------- *
 * a-9  Default recurrent models' LSTM, fused
 *      src/rl8/models/_recurrent.py:201-321 (torch.nn.LSTM(d_in, 256, num_layers=1,
 *      batch_first=True) inside DefaultContinuous/DiscreteRecurrentModel)
 * One layer, hidden 256, fp32 (matrix products on v_mfma_f32_32x32x2_f32), gate
 * order i, f, g, o as in torch, 1 <= d_in <= 7 (rl8_lstm_supports).
 *
 * rl8_lstm_pack_f32: torch-layout parameters (w_ih [1024][d_in], w_hh [1024][256],
 * b_ih, b_hh [1024]) -> `packed` (rl8_lstm_pack_floats() floats): per gate, the
 * 256 x (256 + 8) matrix [w_hh | w_ih | b_ih + b_hh | 0] in MFMA fragment order.
 *
 * rl8_lstm_forward_f32: x [B][L][d_in] dense; h0, c0 [B][256] -> hs [B][L][256]
 * (every h_t), hn, cn [B][256].  For training, save_gates [B][L][4][256]
 * (post-activation i, f, g, o) and save_c [B][L][256] receive what
 * rl8_lstm_backward_f32 needs; both NULL for rollouts.
 * ---------------------------------------------------------------------- */
int rl8_lstm_supports(int d_in);
int64_t rl8_lstm_pack_floats(void);
int rl8_lstm_pack_f32(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                      int d_in, float *packed, void *stream);
int rl8_lstm_forward_f32(const float *x, int64_t b, int l, int d_in, const float *h0, const float *c0,
                         const float *w_packed, float *hs, float *hn, float *cn, float *save_gates,
                         float *save_c, void *stream);

/* Backward through time ("dgrad" half): given dhs [B][L][256] (gradient of every
 * h_t output) and what the forward saved, writes the pre-activation gate
 * gradients dgates [B][L][4][256] and `*partial_rows_out` rows
 * (<= rl8_lstm_backward_max_rows()) of rl8_lstm_backward_partial_floats(d_in)
 * floats into `partials`: [dW_ih (1024 * d_in) | db (1024)], whose column sums are
 * the gradients of w_ih and of each bias vector.  whht_packed [4][65536]: block q =
 * rl8_mlp_pack_w2_f32(w_hh[256q : 256q + 256], transposed = 1).  The recurrent
 * weight gradient is dW_hh[256q : 256q + 256] = rl8_mlp_wgrad_strided_f32(dgates +
 * 256q, 1024, h_prev, 256, B*L, ...) with h_prev[b][t] = h_{t-1} (h0 at t = 0).
 * No gradient is produced for x, h0, c0 or the final states.  * partials == NULL: the data-gradient kernel only (dG out); the input-weight and bias
 * gradients then come from rl8_mlp_wgrad_split_strided_f32's column sums.
 */
int64_t rl8_lstm_backward_partial_floats(int d_in);
int rl8_lstm_backward_max_rows(void);
int rl8_lstm_backward_f32(const float *x, int64_t b, int l, int d_in, const float *c0,
                          const float *gates, const float *cs, const float *dhs,
                          const float *whht_packed, float *dgates, float *partials,
                          int *partial_rows_out /*host*/, void *stream);

/* rl8_lstm_backward_f32's data-gradient kernel and nothing else (it reads no x): dgates [B][L][4][256] from dhs and
 * what a forward saved, for any input width -- the all-fp32 backward through time of the wide-input family below.
 * 32 * L * 4096 < 2^31; whht_packed 16-byte aligned. */
int rl8_lstm_backward_dgates_f32(int64_t b, int l, const float *c0, const float *gates, const float *cs,
                                 const float *dhs, const float *whht_packed, float *dgates, void *stream);

/* The same data gradient with the recurrent product dL/dh_{t-1} = sum_q dG_q x W_hh[q] on the
 * 16-bit matrix pipe (bf16 planes, three per operand, six plane products: fp32-accurate), a
 * wave per 32 sequences for all L steps (lstm_rows_kernels.hip).  What torch.nn.LSTM's backward
 * computes for the module of src/rl8/models/_recurrent.py:201-321 when
 * src/rl8/algorithms/_recurrent.py calls loss.backward().
 * rl8_lstm_rows_backward_pack: w_hh [1024][256] (torch layout, gates i, f, g, o) -> `packed`
 *   (rl8_lstm_rows_backward_pack_bytes() bytes, 16-byte aligned): the planes of W_hh^T in the
 *   order the kernel streams them.  Re-pack when w_hh changes.
 * rl8_lstm_rows_backward_f32: c0 [B][256], gates [B][L][4][256] and cs [B][L][256] as the
 *   forward saved them, dhs [B][L][256] -> dgates [B][L][4][256]; `dc_scratch` [B][256] floats
 *   (contents irrelevant on entry, undefined on return); dg_bound_out (device word, may be NULL) receives the bit
 *   pattern of max |dgates|: the bound rl8_mlp_wgrad_f16_strided_f32 scales its fp16 planes by.  All arrays 16-byte
 *   aligned; 32 * L * 4096 < 2^31.  The input-weight, bias and recurrent-weight gradients come from
 *   rl8_mlp_wgrad_split_strided_f32 on dgates as before. */
int64_t rl8_lstm_rows_backward_pack_bytes(void);
int rl8_lstm_rows_backward_pack(const float *w_hh, void *packed, void *stream);
int rl8_lstm_rows_backward_f32(int64_t b, int l, const float *c0, const float *gates, const float *cs,
                               const float *dhs, const void *packed, float *dgates, float *dc_scratch,
                               uint32_t *dg_bound_out, void *stream);
/* The same with dL/dh_t of the output heads formed inside from heads_dout [b][l][4] (the gradient of the heads' outputs,
 * zero-padded to four per row-step) and heads_w [4][256] (their nn.Linear weights stacked, zero rows past their number):
 * the [b][l][256] array is neither written by rl8_linear_heads_backward_f32 (dh_out NULL) nor read here.
 * Limit.  This form runs the recurrent product on two fp16 planes of dG, scaled per sequence and step by a power of two
 * that places a bound on that step's |dh| + |dc| at 2^6.  The forget gate's gradient dc * c_{t-1} * f (1 - f) carries
 * the cell state, so it stays below fp16's top while |c_{t-1}| < 4 094 (2^6 * |c| / 4 < 65 504); cell states are
 * carried across horizons and never clamped, so a caller has to know this.  Past the limit the plane overflows to
 * infinity and every gate gradient of THAT sequence's earlier timesteps is NaN -- other sequences are untouched -- and
 * *dg_bound_out is then not finite either (a NaN's bit pattern), so that rl8_lstm_wgrad_f16_f32 /
 * rl8_mlp_wgrad_f16_strided_f32 cannot scale such gradients by a finite bound: the weight gradients come out
 * non-finite, never finite and wrong.  The way out is the switch RL8_AMD_LSTM_BACKWARD_PLANES=bf16 (read here, on
 * every call; see the list of LSTM switches at the head of this file): three exact bf16 planes, six plane products, the
 * whole of fp32's range, at about the cost of rl8_lstm_rows_backward_f32. */
int rl8_lstm_rows_backward_heads_f32(int64_t b, int l, const float *c0, const float *gates, const float *cs,
                                     const float *heads_dout, const float *heads_w, const void *packed, float *dgates,
                                     float *dc_scratch, uint32_t *dg_bound_out, void *stream);
/* rl8_mlp_wgrad_split_strided_f32 on fp16 planes (three plane products instead of six): dz and h each scaled by one
 * power of two taken from *dz_bound / *h_bound -- device words holding a float >= max |dz| / max |h| over all rows
 * read (dg_bound_out above; 1.0f for an LSTM's outputs). */
int rl8_mlp_wgrad_f16_strided_f32(const float *dz, int64_t dz_pitch, const uint32_t *dz_bound, const float *h,
                                  int64_t h_pitch, const uint32_t *h_bound, int64_t m, float *workspace,
                                  float *dw_out, int accumulate, const float *x, int d_in, float *colsums,
                                  int *colsum_rows_out, void *stream);

/* The four gates of one LSTM timestep in one launch of the fp16-plane weight gradient: dz = the step's dG rows ([m] rows
 * of dz_pitch >= 1024 floats, gate q at columns [256 q, 256 q + 256)), dw_out [4][256][256] (+)= dG_q^T h per gate,
 * colsums (optional, with x / d_in) [4][*colsum_rows_out][256 (d_in + 1)]; h is then read from HBM once instead of four
 * times.  m >= 128 (RL8_ESIZE below: use rl8_mlp_wgrad_f16_strided_f32 per gate); bounds as there. */
int rl8_lstm_wgrad_f16_f32(const float *dz, int64_t dz_pitch, const uint32_t *dz_bound, const float *h, int64_t h_pitch,
                           const uint32_t *h_bound, int64_t m, float *workspace, float *dw_out, int accumulate,
                           const float *x, int d_in, float *colsums, int *colsum_rows_out, void *stream);

/* ---------------------------------------------------------------------- *
 * a-9, wide input: the same LSTM (one layer, hidden 256, fp32 on v_mfma_f32_32x32x2_f32, gates i, f, g, o) behind
 *      observations of 8 <= d_in <= 128 floats (lstm_wide_in_kernels.hip).  The operand row of the recurrent product
 *      is [h_{t-1} (256) | x_t (d_in) | 1 | 0..], K = 256 + 8 * ceil((d_in + 1) / 8).  The saved gates and cell states
 *      have rl8_lstm_forward_f32's layouts: rl8_lstm_rows_backward[_heads]_f32 or rl8_lstm_backward_dgates_f32 form
 *      dgates from them, the W_hh weight-gradient entries (colsums NULL) dW_hh, rl8_lstm_wide_in_wgrad_f32 dW_ih and db.
 *
 * rl8_lstm_wide_in_supports: 1 for 8 <= d_in <= 128, else 0 (host only).
 * rl8_lstm_wide_in_lds_bytes: dynamic LDS of a launch at d_in: kernel 0 the forward (2 workgroups per CU), 1 the
 *   weight gradient (1 per CU); RL8_ESIZE outside the envelope (host only).
 * rl8_lstm_wide_in_pack_f32: torch-layout parameters (w_ih [1024][d_in], w_hh [1024][256], b_ih, b_hh [1024]) ->
 *   `packed` (rl8_lstm_wide_in_pack_floats(d_in) = 1024 * K floats, 16-byte aligned): per gate the 256 x K matrix
 *   [w_hh | w_ih | b_ih + b_hh | 0..] in MFMA fragment order.  Re-pack when a parameter changes.
 * rl8_lstm_wide_in_forward_f32: x [B][L][d_in] dense; h0 (16-byte aligned), c0 [B][256] -> hs [B][L][256], hn, cn
 *   [B][256]; save_gates [B][L][4][256] and save_c [B][L][256] both given (training) or both NULL (L = 1 with both
 *   NULL is the rollout step).  32 * L * 4096 < 2^31.
 * rl8_lstm_wide_in_wgrad_f32: dw_ih_out [1024][d_in] = dgates^T x and db_out [1024] = the column sums of dgates over
 *   the m = B * L rows (dgates [m][1024] 16-byte aligned, x [m][d_in]); db comes from a ones column beside the x tile,
 *   not from a second pass.  `workspace`: rl8_lstm_wide_in_workspace_bytes(d_in) bytes (one [256][d_in + 1] slab per
 *   gate and workgroup).  The grid is a function of m and d_in alone and the slabs are summed in slab order: bitwise
 *   reproducible.
 * Every entry returns RL8_ENULL / RL8_ESIZE / RL8_EALIGN before any launch.
 * ---------------------------------------------------------------------- */
int rl8_lstm_wide_in_supports(int d_in);
int64_t rl8_lstm_wide_in_lds_bytes(int kernel, int d_in);
int64_t rl8_lstm_wide_in_pack_floats(int d_in);
int rl8_lstm_wide_in_pack_f32(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, int d_in,
                              float *packed, void *stream);
int rl8_lstm_wide_in_forward_f32(const float *x, int64_t b, int l, int d_in, const float *h0, const float *c0,
                                 const float *w_packed, float *hs, float *hn, float *cn, float *save_gates,
                                 float *save_c, void *stream);
int64_t rl8_lstm_wide_in_workspace_bytes(int d_in);
int rl8_lstm_wide_in_wgrad_f32(const float *dgates, const float *x, int64_t m, int d_in, float *workspace,
                               float *dw_ih_out, float *db_out, void *stream);

/* ---------------------------------------------------------------------- *
 * a-9, stacks of width 256: a layer ABOVE the first of an LSTM with num_layers >= 2 (lstm_stack256_kernels.hip; fp32 on
 *      v_mfma_f32_32x32x2_f32, gates i, f, g, o).  Its input row is the 256 floats of the layer below's hs[b][t]; the
 *      operand row of the recurrent product is [h_{t-1} (256) | x_t (256) | 1 | 0 x 7], K = 520.  Layer 0 runs on the
 *      entries of its own input width (rl8_lstm_forward_f32 / rl8_lstm_step_split_f32 / rl8_lstm_wide_in_forward_f32).
 *      The saved gates and cell states have rl8_lstm_forward_f32's layouts: rl8_lstm_rows_backward_f32 or
 *      rl8_lstm_backward_dgates_f32 form dgates from them; the W_hh weight-gradient entries (colsums NULL) form dW_hh
 *      per step and, in one more accumulation over all m = B * L rows with h = the layer below's hs (pitch 256), dW_ih;
 *      rl8_lstm_stack256_dx_f32 forms the layer below's dL/dhs and this layer's bias gradient.
 *
 * rl8_lstm_stack256_supports: 1 where the build has these kernels (host only).
 * rl8_lstm_stack256_lds_bytes: dynamic LDS of a launch: kernel 0 the forward (66 688 B, 2 workgroups per CU), 1 the
 *   input / bias gradient (65 792 B, 2 per CU); RL8_ESIZE for any other kernel (host only).
 * rl8_lstm_stack256_pack_f32: torch-layout parameters of the layer (w_ih, w_hh [1024][256], b_ih, b_hh [1024]) ->
 *   `packed` (rl8_lstm_stack256_pack_floats() = 1024 * 520 floats, 16-byte aligned): per gate the 256 x 520 matrix
 *   [w_hh | w_ih | b_ih + b_hh | 0 x 7] in MFMA fragment order.  Re-pack when a parameter changes.
 * rl8_lstm_stack256_forward_f32: x [B][L][256] dense (the layer below's hs) and h0, both 16-byte aligned, c0 [B][256] ->
 *   hs [B][L][256], hn, cn [B][256]; save_gates [B][L][4][256] and save_c [B][L][256] both given (training) or both
 *   NULL; either way the same bits in hs, hn, cn.  32 * L * 4096 < 2^31.
 * rl8_lstm_stack256_dx_f32: dx_out [m][256] = dgates [m][1024] x w_ih and db_out [1024] = the column sums of dgates,
 *   from one read of dgates (16-byte aligned).  `wiht_packed`: w_ih [1024][256] packed per gate by
 *   rl8_mlp_pack_w2_f32(transposed = 1), as rl8_lstm_backward_f32 takes w_hh (4 x 65 536 floats, 16-byte aligned).
 *   `workspace`: rl8_lstm_stack256_workspace_bytes(m) bytes (one [1024] slab of column sums per workgroup; RL8_ESIZE
 *   for m < 1).  The grid is a function of m alone, each workgroup sums its rows in row order in fp32, and the slabs
 *   are summed in slab order in fp64: bitwise reproducible.
 * Every entry returns RL8_ENULL / RL8_ESIZE / RL8_EALIGN before any launch.
 * ---------------------------------------------------------------------- */
int rl8_lstm_stack256_supports(void);
int64_t rl8_lstm_stack256_lds_bytes(int kernel);
int64_t rl8_lstm_stack256_pack_floats(void);
int rl8_lstm_stack256_pack_f32(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, float *packed,
                               void *stream);
int rl8_lstm_stack256_forward_f32(const float *x, int64_t b, int l, const float *h0, const float *c0,
                                  const float *w_packed, float *hs, float *hn, float *cn, float *save_gates,
                                  float *save_c, void *stream);
int64_t rl8_lstm_stack256_workspace_bytes(int64_t m);
int rl8_lstm_stack256_dx_f32(const float *dgates, int64_t m, const float *wiht_packed, float *workspace, float *dx_out,
                             float *db_out, void *stream);

/* The recurrent models' output heads (src/rl8/models/_recurrent.py:230-236, 287-292),
 * all of them at once: out [M][n] = h [M][256] x w^T + b, w [n][256] (the heads'
 * nn.Linear weights stacked), n <= 8.  Backward: dh_out [M][256] = dout x w and
 * `*partial_rows_out` rows (<= rl8_linear_heads_max_rows()) of [dW (n*256) | db (n)]
 * whose column sums are the parameter gradients; dh_out NULL: the parameter gradients only (the recurrent models'
 * backward forms dh inside rl8_lstm_rows_backward_heads_f32).
 * rl8_linear_heads_forward_pair_f32: two layers that stay separate arrays (the rollout's logits head and value head,
 * algorithms/_recurrent.py:400-420 via policy.sample()) in one pass over h: out_a [M][n_a], out_b [M][n_b],
 * n_a + n_b <= 8. */
int rl8_linear_heads_max_rows(void);
int rl8_linear_heads_forward_f32(const float *h, int64_t m, const float *w, const float *b, int n_out,
                                 float *out, void *stream);
int rl8_linear_heads_forward_pair_f32(const float *h, int64_t m, const float *w_a, const float *b_a, int n_a,
                                      float *out_a, const float *w_b, const float *b_b, int n_b, float *out_b,
                                      void *stream);
int rl8_linear_heads_backward_f32(const float *h, const float *dout, int64_t m, const float *w,
                                  int n_out, float *dh_out, float *partials,
                                  int *partial_rows_out /*host*/, void *stream);

/* ---- Narrow towers: Linear(d_in, H) ReLU Linear(H, H) ReLU Linear(H, n_out), H = 64 or 128 (mlp_narrow_kernels.hip).
 * Weights in torch layout, unpacked: w1 [H][d_in], b1 [H], w2 [H][H], b2 [H], w3 [n_out][H], b3 [n_out]; d_in <= 16,
 * n_out <= 8.  Layer 2 (and, backward, dh1 and dW2) on fp32 MFMA; no activation goes to HBM.
 * rl8_mlp_narrow_supports: 1 when (hidden, d_in, n_out) is compiled in, else 0.
 * rl8_mlp_narrow_forward_f32: x [m][d_in] -> out [m][n_out].
 * rl8_mlp_narrow_backward_f32: recomputes the forward from x and writes one partial slab of gradients per workgroup
 *   into `workspace` (rl8_mlp_narrow_workspace_bytes(m, ...) bytes, no initialisation); rl8_mlp_narrow_reduce_f32
 *   then sums the slabs in a fixed order (fp64) into grads_out = [dW1 (H d_in) | db1 (H) | dW2 (H H) | db2 (H) |
 *   dW3 (n_out H) | db3 (n_out)] floats: bitwise reproducible.  No gradient is produced for x.
 * rl8_mlp_narrow_backward_dx_f32: the same, and dx [m][d_in] = dz1 W1 (the gradient of x) from the same launch;
 *   workspace layout and the reduce call are unchanged and the workspace holds the same bits.  dx == NULL: exactly
 *   rl8_mlp_narrow_backward_f32.
 * All pointers 4-byte aligned; m >= 1; RL8_ESIZE for widths outside the compiled set. */
int rl8_mlp_narrow_supports(int hidden, int d_in, int n_out);
int64_t rl8_mlp_narrow_workspace_bytes(int64_t m, int hidden, int d_in, int n_out);
int rl8_mlp_narrow_forward_f32(const float *x, int64_t m, int d_in, const float *w1, const float *b1, const float *w2,
                               const float *b2, const float *w3, const float *b3, int n_out, int hidden, float *out,
                               void *stream);
int rl8_mlp_narrow_backward_f32(const float *x, const float *dout, int64_t m, int d_in, const float *w1,
                                const float *b1, const float *w2, const float *b2, const float *w3, int n_out,
                                int hidden, float *workspace, void *stream);
int rl8_mlp_narrow_reduce_f32(const float *workspace, int64_t m, int hidden, int d_in, int n_out, float *grads_out,
                              void *stream);
int rl8_mlp_narrow_backward_dx_f32(const float *x, const float *dout, int64_t m, int d_in, const float *w1,
                                   const float *b1, const float *w2, const float *b2, const float *w3, int n_out,
                                   int hidden, float *workspace, float *dx, void *stream);

/* ---- Wide-input towers: Linear(d_in, 256) ReLU Linear(256, 256) ReLU Linear(256, n_out), 17 <= d_in <= 128,
 * 1 <= n_out <= 8 (mlp_wide_in_kernels.hip): fp32 throughout, every product but the head on v_mfma_f32_32x32x2_f32.
 * The entries above keep their envelope (d_in <= 16); these are the widths behind it.
 * rl8_mlp_wide_in_supports: 1 inside the envelope, else 0 (host only).
 * rl8_mlp_wide_in_pack_w1_f32: w1 [256][d_in] (torch layout) -> w1_packed, rl8_mlp_wide_in_pack_floats(d_in) floats
 *   (256 * 8 * ceil(d_in / 8)): MFMA fragment order, zeros past d_in.  w1_packed 16-byte aligned.
 * rl8_mlp_wide_in_forward_f32: x [m][d_in] -> out [m][n_out]; w2_packed from rl8_mlp_pack_w2_f32(transposed = 0).
 *   save_h1 / save_h2 ([m][256] each, 16-byte aligned): both or neither; with them the post-ReLU activations are
 *   stored for the backward entries.
 * rl8_mlp_wide_in_backward_f32: from h1, h2, dout [m][n_out], w3 [n_out][256] and w2t_packed
 *   (rl8_mlp_pack_w2_f32(transposed = 1)) writes dz2_out [m][256] = (dout W3) . [h2 > 0] and dz1_out [m][256] =
 *   (dZ2 W2) . [h1 > 0] (ReLU'(0) = 0), and one row of partials per workgroup, rl8_mlp_wide_in_partial_floats(n_out)
 *   floats each: [db1 (256) | db2 (256) | dW3 (n_out * 256) | db3 (n_out)]; *partial_rows_out (host) rows, at most
 *   rl8_mlp_wide_in_max_rows(), a function of m alone; the caller sums them in row order.  No gradient of x.
 *   h1, h2, dz1_out, dz2_out, w2t_packed 16-byte aligned.
 * rl8_mlp_wide_in_wgrad_f32: dw1_out [256][d_in] = (accumulate ? dw1_out : 0) + dz1^T x over the m rows, fp32 MFMA,
 *   one slab per workgroup in `workspace` (rl8_mlp_wide_in_workspace_bytes(d_in) bytes, no initialisation) summed in
 *   slab order; the grid is a function of m alone: bitwise reproducible.  dz1 16-byte aligned.
 *   (dW2 = dz2^T h1 is rl8_mlp_wgrad_split_strided_f32 or rl8_mlp_wgrad_f32: both take their operands from memory.)
 * rl8_mlp_wide_in_lds_bytes: the dynamic LDS of one workgroup of kernel 0 (forward, two workgroups per CU), 1 (data
 *   gradient, two per CU) or 2 (weight gradient at d_in, one per CU); host only.
 * Every other pointer 4-byte aligned; RL8_ENULL / RL8_ESIZE (m < 1, d_in or n_out outside the envelope) / RL8_EALIGN
 * before any launch.  The helpers return RL8_ESIZE for a width outside the envelope. */
int rl8_mlp_wide_in_supports(int d_in, int n_out);
int64_t rl8_mlp_wide_in_lds_bytes(int kernel, int d_in);
int64_t rl8_mlp_wide_in_pack_floats(int d_in);
int rl8_mlp_wide_in_pack_w1_f32(const float *w1, int d_in, float *w1_packed, void *stream);
int rl8_mlp_wide_in_forward_f32(const float *x, int64_t m, int d_in, const float *w1_packed, const float *b1,
                                const float *w2_packed, const float *b2, const float *w3, const float *b3, int n_out,
                                float *out, float *save_h1, float *save_h2, void *stream);
int64_t rl8_mlp_wide_in_partial_floats(int n_out);
int rl8_mlp_wide_in_max_rows(void);
int rl8_mlp_wide_in_backward_f32(const float *h1, const float *h2, const float *dout, int64_t m,
                                 const float *w2t_packed, const float *w3, int n_out, float *dz1_out, float *dz2_out,
                                 float *partials, int *partial_rows_out /*host*/, void *stream);
int64_t rl8_mlp_wide_in_workspace_bytes(int d_in);
int rl8_mlp_wide_in_wgrad_f32(const float *dz1, const float *x, int64_t m, int d_in, float *workspace, float *dw1_out,
                              int accumulate, void *stream);

/* ---- Wide-head towers (DEFAULT PRODUCT PATH): Linear(d_in, 256) ReLU Linear(256, 256) ReLU Linear(256, n_out),
 * 1 <= d_in <= 128, 9 <= n_out <= 128 summed over the heads (mlp_wide_out_kernels.hip): fp32 throughout, every product,
 * the head and its gradients included, on v_mfma_f32_32x32x2_f32.  The entries above keep their envelopes (n_out <= 8).
 * rl8_mlp_wide_out_supports: 1 inside the envelope, else 0 (host only).
 * rl8_mlp_wide_out_pack_f32: a torch-layout weight -> MFMA fragment order, zero-padded, rl8_mlp_wide_out_pack_floats(
 *   matrix, n) floats, `packed` 16-byte aligned.  matrix 0: w = W1 [256][n], n = d_in in 1..128, for the forward
 *   (256 * 8 * ceil(n / 8) floats); matrix 1: w = W3 [n][256], n = n_out, for the forward (32 * ceil(n / 32) * 256
 *   floats); matrix 2: the same W3 for the data gradient (256 * 8 * ceil(n / 8) floats).
 * rl8_mlp_wide_out_forward_f32: x [m][d_in] -> out [m][n_out] = b3 + h2 W3^T; w1_packed / w3_packed from matrix 0 / 1,
 *   w2_packed from rl8_mlp_pack_w2_f32(transposed = 0).  save_h1 / save_h2 ([m][256] each, 16-byte aligned): both or
 *   neither; with them the post-ReLU activations are stored for the backward entries; `out` is the same bits either way.
 * rl8_mlp_wide_out_backward_f32: from h1, h2, dout [m][n_out], w3t_packed (matrix 2) and w2t_packed
 *   (rl8_mlp_pack_w2_f32(transposed = 1)) writes dz2_out [m][256] = (dout W3) . [h2 > 0] and dz1_out [m][256] =
 *   (dZ2 W2) . [h1 > 0] (ReLU'(0) = 0), and one row of partials per workgroup, rl8_mlp_wide_out_partial_floats(n_out)
 *   floats each: [db1 (256) | db2 (256) | db3 (n_out)]; *partial_rows_out (host) rows, at most
 *   rl8_mlp_wide_out_max_rows(), a function of m alone; the caller sums them in row order.  No dW3 (it is a product
 *   over the rows: below) and no gradient of x.  h1, h2, dz1_out, dz2_out and the packs 16-byte aligned.
 * rl8_mlp_wide_out_wgrad_f32: out [256][c] = (accumulate ? out : 0) + a^T b over the m rows, a [m][256] (16-byte
 *   aligned), b [m][c], 1 <= c <= 128, fp32 MFMA, one slab per workgroup in `workspace`
 *   (rl8_mlp_wide_out_workspace_bytes(c) bytes, no initialisation) summed in slab order; the grid is a function of m
 *   alone: bitwise reproducible.  `transpose`: out is [c][256].  dW1 = dz1^T x (c = d_in, any d_in of the envelope) and
 *   dW3 = (h2^T dout)^T (c = n_out, transpose = 1).  (dW2 = dz2^T h1 is rl8_mlp_wgrad_split_strided_f32 or
 *   rl8_mlp_wgrad_f32.)
 * rl8_mlp_wide_out_lds_bytes: the dynamic LDS of one workgroup of kernel 0 (forward, two workgroups per CU), 1 (data
 *   gradient, two per CU) or 2 (weight gradient at c columns, one per CU); host only.
 * Every other pointer 4-byte aligned; RL8_ENULL / RL8_ESIZE (m < 1, a width outside the envelope) / RL8_EALIGN before
 * any launch.  The helpers return RL8_ESIZE for a width outside the envelope. */
int rl8_mlp_wide_out_supports(int d_in, int n_out);
int64_t rl8_mlp_wide_out_lds_bytes(int kernel, int c);
int64_t rl8_mlp_wide_out_pack_floats(int matrix, int n);
int rl8_mlp_wide_out_pack_f32(const float *w, int matrix, int n, float *packed, void *stream);
int rl8_mlp_wide_out_forward_f32(const float *x, int64_t m, int d_in, const float *w1_packed, const float *b1,
                                 const float *w2_packed, const float *b2, const float *w3_packed, const float *b3,
                                 int n_out, float *out, float *save_h1, float *save_h2, void *stream);
int64_t rl8_mlp_wide_out_partial_floats(int n_out);
int rl8_mlp_wide_out_max_rows(void);
int rl8_mlp_wide_out_backward_f32(const float *h1, const float *h2, const float *dout, int64_t m,
                                  const float *w2t_packed, const float *w3t_packed, int n_out, float *dz1_out,
                                  float *dz2_out, float *partials, int *partial_rows_out /*host*/, void *stream);
int64_t rl8_mlp_wide_out_workspace_bytes(int c);
int rl8_mlp_wide_out_wgrad_f32(const float *a, const float *b, int64_t m, int c, float *workspace, float *out,
                               int accumulate, int transpose, void *stream);

/* ---- BatchNorm1d behind the first layer of a narrow tower, folded into that layer (batchnorm_tower_kernels.hip).  In
 * training mode the norm of z1 = x W1^T + b1 over the batch is an affine map of x: with mu = mean_i x_i and the biased
 * covariance C = (1/m) sum_i (x_i - mu)(x_i - mu)^T, unit j has batch mean m_z_j = W1_j . mu + b1_j, batch variance
 * v_j = W1_j C W1_j^T, r_j = 1 / sqrt(v_j + eps), and y_j = a_j . x + c_j with a_j = gamma_j r_j W1_j and
 * c_j = beta_j - gamma_j r_j (W1_j . mu).  The tower then runs rl8_mlp_narrow_* with w1 = a, b1 = c.
 * rl8_tower_moments_f64: x [m][d_in] fp32 -> mu [d_in], cov [d_in][d_in] in fp64.  One pass: sums of x - p and of
 *   (x - p)(x - p)^T about the pivot p = x[0] in fp64, one partial slab per workgroup in `workspace`
 *   (rl8_tower_moments_workspace_bytes(m, d_in) bytes, no initialisation), summed in slab order by a second launch
 *   into mu = p + S1 / m, cov = S2 / m - (S1 / m)(S1 / m)^T.  No atomics: the same bits on every run; a constant column
 *   has a row and a column of cov that are exactly 0.
 * rl8_batchnorm_fold_f32: one launch.  training != 0: from (mu, cov, m >= 2) and w1 [H][d_in], b1, gamma, beta [H], eps
 *   -> a [H][d_in], c [H] (fp32) and r, m_z, v [H] (fp64), all formed in fp64 and rounded once; running_mean /
 *   running_var [H] (both or neither) move in place by `factor` -- by 1 / *tracked where `tracked` (device int64, the
 *   count of batches INCLUDING this one) is given -- towards m_z and the unbiased v m / (m - 1).  training == 0:
 *   a_j = gamma_j W1_j / sqrt(running_var_j + eps), c_j = beta_j + gamma_j (b1_j - running_mean_j) / sqrt(running_var_j
 *   + eps); nothing else is read or written.
 * rl8_tower_limits (host only): limits[0..4] = the moments kernel's workgroup cap and rows per step, the narrow tower
 *   kernels' workgroup caps at H = 64 and 128 and their rows per step.
 * RL8_ENULL: a required pointer.  RL8_ESIZE: m < 1 (fold in training mode: m < 2), d_in outside 1 .. 16, hidden not 64
 *   or 128.  RL8_EALIGN: a float pointer off 4 bytes, a double / int64 pointer off 8.  All before any launch. */
int rl8_tower_limits(int *limits /*host*/);
int64_t rl8_tower_moments_workspace_bytes(int64_t m, int d_in);
int rl8_tower_moments_f64(const float *x, int64_t m, int d_in, double *mu, double *cov, double *workspace, void *stream);
int rl8_batchnorm_fold_f32(const double *mu, const double *cov, int64_t m, int d_in, int hidden, const float *w1,
                           const float *b1, const float *gamma, const float *beta, double eps, float *running_mean,
                           float *running_var, double factor, const int64_t *tracked, int training, float *a, float *c,
                           double *r, double *m_z, double *v, void *stream);

/* ---- Narrow LSTMs: one layer, biased, batch_first, hidden width H = 64 or 128, d_in <= 16 (lstm_narrow_kernels.hip).
 * Weights in torch layout, unpacked: w_ih [4H][d_in], w_hh [4H][H], b_ih / b_hh [4H], gate order i, f, g, o.  The
 * products run on fp32 MFMA with the time loop inside the kernel.
 * rl8_lstm_narrow_supports: 1 when (hidden, d_in) is compiled in, else 0.
 * rl8_lstm_narrow_forward_f32: x [b][l][d_in], h0 / c0 [b][H] -> hs [b][l][H], hn / cn [b][H].  save_gates
 *   ([b][l][4][H], post-activation) and save_c ([b][l][H], cell states) both NULL: inference; both set: training, for
 *   the backward.  hs, hn and cn are bitwise the same in both modes.
 * rl8_lstm_narrow_backward_f32: backward through time from dL/dhs (dhs [b][l][H]) and what the training forward
 *   saved; writes the gate gradients and one partial slab of weight gradients per sequence chunk into `workspace`
 *   (rl8_lstm_narrow_workspace_bytes(b, l, ...) bytes, no initialisation); rl8_lstm_narrow_reduce_f32 then sums the
 *   slabs in a fixed order (fp64) into grads_out = [dW_ih (4H d_in) | dW_hh (4H H) | db (4H)] floats, db being the
 *   gradient of b_ih and of b_hh alike: bitwise reproducible.  No gradient for h0 or c0 (for x: the call of
 *   rl8_lstm_narrow_input_grad_f32 below, where wanted); c_n is not differentiable.
 * Pointers 4-byte aligned, workspace 16-byte aligned; b >= 1, 1 <= l < 2^31 / (256 H); RL8_ESIZE for widths outside
 * the compiled set. */
int rl8_lstm_narrow_supports(int hidden, int d_in);
int64_t rl8_lstm_narrow_workspace_bytes(int64_t b, int l, int hidden, int d_in);
int rl8_lstm_narrow_forward_f32(const float *x, int64_t b, int l, int d_in, const float *h0, const float *c0,
                                const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, int hidden,
                                float *hs, float *hn, float *cn, float *save_gates, float *save_c, void *stream);
int rl8_lstm_narrow_backward_f32(const float *x, int64_t b, int l, int d_in, const float *h0, const float *c0,
                                 const float *w_hh, int hidden, const float *hs, const float *gates, const float *cs,
                                 const float *dhs, float *workspace, void *stream);
int rl8_lstm_narrow_reduce_f32(const float *workspace, int64_t b, int l, int hidden, int d_in, float *grads_out,
                               void *stream);

/* rl8_lstm_narrow_backward_f32 with dL/dhs given by the output heads it came through instead of as an array:
 * dL/dh[b][t][u] = sum_q heads_dout[b][t][q] heads_w[q][u], q < 4, formed inside the backward through time (heads_dout
 * [b][l][4] and heads_w [4][H], both zero-padded beyond the heads' outputs; heads_dout 16-byte aligned).  Same
 * workspace, same reduce call after it; the [b][l][H] array is neither written by rl8_linear_heads_narrow_backward_f32
 * (dh_out NULL) nor read here.  With dhs formed by that entry, the two forms give the same bits. */
int rl8_lstm_narrow_backward_heads_f32(const float *x, int64_t b, int l, int d_in, const float *h0, const float *c0,
                                       const float *w_hh, int hidden, const float *hs, const float *gates,
                                       const float *cs, const float *heads_dout, const float *heads_w, float *workspace,
                                       void *stream);

/* dL/dx of layer 0, for models with learned parameters in front of the LSTM (an embedding, an encoder):
 * dx[n][k] = sum_j dz[n][j] w_ih[j][k] over the n = b l row-steps, j < 4H, k < d_in, from the gate gradients dz that
 * rl8_lstm_narrow_backward_f32 / rl8_lstm_narrow_backward_heads_f32 left at the front of `workspace` (call it after
 * either, with the same b, l, hidden, d_in; before or after the reduce).  w_ih [4H][d_in] in torch layout, dx
 * [b][l][d_in] (exactly b l d_in floats are written).  fp32 MFMA in a fixed k order: bitwise reproducible and
 * independent of the grid.  workspace 16-byte aligned, w_ih and dx 4-byte; sizes as for the other narrow entries. */
int rl8_lstm_narrow_input_grad_f32(const float *workspace, int64_t b, int l, int d_in, const float *w_ih, int hidden,
                                   float *dx, void *stream);

/* ---- Output heads of the narrow recurrent models: Linear(H, n) layers on h [m][H], H = 64 or 128, evaluated together
 * (lstm_narrow_heads_kernels.hip): w [n_out][H] (the heads' weights stacked), b [n_out], n_out <= 8.
 * rl8_linear_heads_narrow_forward_f32: out [m][n_out] = h x w^T + b, one pass over h.
 * rl8_linear_heads_narrow_forward_pair_f32: two layers that stay separate arrays (out_a [m][n_a], out_b [m][n_b],
 *   n_a + n_b <= 8) in the same pass.  The arithmetic for one output and its order depend on H alone: single form, pair
 *   form and rl8_rollout_step_dummy_heads_narrow_f32 agree bit for bit.
 * rl8_linear_heads_narrow_backward_f32: grads_out = [dW (n_out H) | db (n_out)] and, unless dh_out is NULL, dh_out
 *   [m][H] = dout x w.  One partial slab per workgroup in `workspace` (rl8_linear_heads_narrow_workspace_bytes(m, ...)
 *   bytes, no initialisation; the grid is a function of m alone), summed in a fixed order in fp64: bitwise reproducible.
 * h and w 16-byte aligned for the forward entries, every other pointer 4-byte aligned; m >= 1; RL8_ESIZE for other
 * widths and for n_out outside 1..8. */
int64_t rl8_linear_heads_narrow_workspace_bytes(int64_t m, int hidden, int n_out);
int rl8_linear_heads_narrow_forward_f32(const float *h, int64_t m, int hidden, const float *w, const float *b, int n_out,
                                        float *out, void *stream);
int rl8_linear_heads_narrow_forward_pair_f32(const float *h, int64_t m, int hidden, const float *w_a, const float *b_a,
                                             int n_a, float *out_a, const float *w_b, const float *b_b, int n_b,
                                             float *out_b, void *stream);
int rl8_linear_heads_narrow_backward_f32(const float *h, const float *dout, int64_t m, int hidden, const float *w,
                                         int n_out, float *dh_out, float *workspace, float *grads_out, void *stream);

/* ---- Stacked LSTMs: layers 1.. of nn.LSTM(d_in, H, num_layers >= 2), H = 64 or 128, biased, batch_first, fp32, no
 * dropout (lstm_narrow_kernels.hip, lstm_narrow_stack_*).  One upper layer per call: its input x [b][l][H] is the
 * lower layer's hs; layer 0 runs rl8_lstm_narrow_*.  Weights in torch layout: w_ih [4H][H], w_hh [4H][H], b_ih / b_hh
 * [4H].  rl8_lstm_stack_supports: 1 when `hidden` is compiled in, else 0.
 * rl8_lstm_stack_forward_f32: the input projection of all b l row-steps into zin ([b][l][4][H] floats of scratch,
 *   16-byte aligned, not needed after the call), then the recurrent forward: h0 / c0 [b][H] -> hs [b][l][H], hn / cn
 *   [b][H].  save_gates / save_c as for rl8_lstm_narrow_forward_f32; hs, hn and cn are bitwise the same in both modes.
 * rl8_lstm_stack_backward_f32: backward through time from dhs [b][l][H] and what the training forward saved, then
 *   dx [b][l][H] = dL/dx (the lower layer's dhs) and one partial slab of weight gradients per sequence chunk in
 *   `workspace` (rl8_lstm_stack_workspace_bytes(b, l, hidden) bytes = 4 (b l 4H + chunks 4H (2H + 1)), no
 *   initialisation, reusable from layer to layer); rl8_lstm_stack_reduce_f32 then sums the slabs in a fixed order
 *   (fp64) into grads_out = [dW_ih (4H H) | dW_hh (4H H) | db (4H)]: bitwise reproducible.  No gradient for h0 or c0.
 * Pointers 4-byte aligned, zin and workspace 16-byte aligned; sizes as for the narrow entries; RL8_ESIZE for other
 * widths. */
int rl8_lstm_stack_supports(int hidden);
int64_t rl8_lstm_stack_workspace_bytes(int64_t b, int l, int hidden);
int rl8_lstm_stack_forward_f32(const float *x, int64_t b, int l, const float *h0, const float *c0, const float *w_ih,
                               const float *w_hh, const float *b_ih, const float *b_hh, int hidden, float *zin,
                               float *hs, float *hn, float *cn, float *save_gates, float *save_c, void *stream);
int rl8_lstm_stack_backward_f32(const float *x, int64_t b, int l, const float *h0, const float *c0, const float *w_ih,
                                const float *w_hh, int hidden, const float *hs, const float *gates, const float *cs,
                                const float *dhs, float *workspace, float *dx, void *stream);
int rl8_lstm_stack_reduce_f32(const float *workspace, int64_t b, int l, int hidden, float *grads_out, void *stream);

/* ---- OPT-IN: towers of a SCALAR observation as exact piecewise-linear tables (round 4 prototype; VERDICT r3 item 10,
 * DESIGN.md section 9).  Special to d_in = 1 -- the dummy envs of BASELINE configs 2 and 4 -- and never a replacement
 * for the general tower kernels above, which every other shape runs and against which this path is tested.  The
 * table (breakpoints ascending, then per interval an anchor, n_out values at the anchor, n_out slopes) is built by
 * the caller in fp64 from the tower's weights (rl8_amd/nn/piecewise_mlp.py; reference arithmetic:
 * src/rl8/models/_feedforward.py:336-375) and handed over as floats:
 *   table = [ breaks[p] | anchor[p + 1] | value[(p + 1) * n_out] | slope[(p + 1) * n_out] ]
 *   out[r][q] = value[i][q] + slope[i][q] * (x[r] - anchor[i]),   i = number of breakpoints < x[r].
 * p <= rl8_pw_max_breaks(), n_out <= 3. */
int rl8_pw_max_breaks(void);
int rl8_pw_tower_forward_f32(const float *x, int64_t m, const float *table, int p, int n_out, float *out, void *stream);
/* Per interval i the sums over its rows of dOut and of dOut * x, all the backward pass of such a tower needs from the
 * rows: sums_out[i][0][q] = sum dout[r][q], sums_out[i][1][q] = sum dout[r][q] * x[r]  (fp64, [(p + 1)][2][n_out]).
 * Accumulated EXACTLY on a common power-of-two scale in 64-bit integers (two per sum, 74 bits), so the result does not
 * depend on the order of the atomics: bitwise reproducible.  m <= 2^25 per call.  workspace:
 * rl8_pw_workspace_bytes(p, n_out) bytes, 16-byte aligned, no initialisation.  A non-finite dOut or x makes every sum
 * NaN.  RL8_ESIZE when the accumulators do not fit LDS (p * n_out beyond ~3000): the caller keeps the general path. */
int64_t rl8_pw_workspace_bytes(int p, int n_out);
int rl8_pw_segment_sums_f32(const float *x, const float *dout, int64_t m, int n_out, const float *breaks, int p,
                            void *workspace, double *sums_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RL8_AMD_H */
