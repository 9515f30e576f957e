// Categorical action spaces of more than RL8_MAX_CLASSES classes: the sampler and the fused PPO loss with one WAVE per
// sample row, where rollout_kernels.hip and ppo_loss_kernels.hip keep a row in one lane's array of 64 floats.
// Lanes stride over the classes (class j of a row sits in lane j % 64), so every access of a wave is a run of 256
// contiguous bytes; sums and maxima over a row are taken lane by lane in ascending j and then across the lanes with the
// xor butterflies of wave_rows.hip.h -- a fixed order, the same bits in every lane and in every run.
// Compiled with -ffp-contract=off: every reference operation rounds once.
//
// No kernel here declares a per-lane array with a run-time index: the sampler walks its row again for every pass (a
// rollout's rows are few and stay in L1 / L2 between walks), the loss keeps a row of up to 1024 classes in registers
// (NCH = ceil(k / 64) rounded up to a power of two, every index a compile-time constant) and walks a longer one again.
#include <stdlib.h>

#include "common.hip.h"
#include "device_math.hip.h"
#include "ppo_loss_publish.hip.h"
#include "wave_rows.hip.h"

namespace rl8 {
namespace {

// ---- sampler ------------------------------------------------------------------------------------------------------
// categorical_normalise_dyn<true> followed by the loop of categorical_sample_kernel (rollout_kernels.hip), operation
// for operation, the row read again where those keep it in an array: nl_j = x_j - lse, p_j = exp(nl_j - mx2) / s2.
// mx2 = max_j nl_j is (max_j x_j) - lse because a rounded subtraction is monotone.
__global__ __launch_bounds__(kBlock) void categorical_wide_sample_kernel(
    const float *__restrict__ logits, const float *__restrict__ noise, int64_t *__restrict__ action,
    float *__restrict__ logp, int64_t m, int a, int k, uint64_t seed, uint64_t step, int64_t row_offset,
    int deterministic) {
  for_each_wave_row(m, [&](int64_t i, int lane) {
    float lp = 0.0f;
    for (int d = 0; d < a; ++d) {
      const float *x = logits + (i * a + d) * k;
      const float *q = noise ? noise + (i * a + d) * k : nullptr;
      float mx = -INFINITY;
      for (int j = lane; j < k; j += kWave) {
        const float v = x[j];
        mx = v > mx ? v : mx;
      }
      mx = wave_max(mx);
      float s = 0.0f;
      for (int j = lane; j < k; j += kWave) s += cr_expf(x[j] - mx);
      const float lse = mx + cr_logf(wave_sum(s));
      const float mx2 = mx - lse;
      float s2 = 0.0f;
      for (int j = lane; j < k; j += kWave) s2 += cr_expf((x[j] - lse) - mx2);
      s2 = wave_sum(s2);
      int best = 0x7fffffff;  // (a lane that saw no value above -inf never beats one that did)
      float best_v = -INFINITY;
      for (int j = lane; j < k; j += kWave) {  // (ascending j within the lane, strict >: the lane's first maximum)
        const float p = cr_expf((x[j] - lse) - mx2) / s2;
        float v;
        if (deterministic) {
          v = p;
        } else {
          const float qj = q ? q[j] : rl8_exponential(seed, (uint64_t)(i + row_offset), step, (uint32_t)(d * k + j));
          v = p / qj;
        }
        if (v > best_v) {
          best_v = v;
          best = j;
        }
      }
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) {  // the larger value, the lower index on a tie: any order agrees
        const float ov = __shfl_xor(best_v, off, kWave);
        const int oj = __shfl_xor(best, off, kWave);
        if (ov > best_v || (ov == best_v && oj < best)) {
          best_v = ov;
          best = oj;
        }
      }
      if (best == 0x7fffffff) best = 0;  // (nothing above -inf anywhere, e.g. NaN logits: class 0, as the lane kernel)
      const float nlb = x[best] - lse;
      lp = d == 0 ? nlb : lp + nlb;
      if (lane == 0) action[i * a + d] = best;
    }
    if (lane == 0) logp[i] = lp;
  });
}

// ---- loss ---------------------------------------------------------------------------------------------------------
// One row of one action dimension across the wave.  NCH > 0: classes c * 64 + lane, c < NCH, in registers -- x, then
// p = exp(nl - mx2) / s2 -- with every array index a compile-time constant; NCH == 0: nothing kept, the row is read
// again and p formed again wherever it is needed.
template <int NCH>
struct WideRow {
  static constexpr int kHeld = NCH > 0 ? NCH : 1;
  float x[kHeld], p[kHeld];
  float lse, mx2, s2;
};

template <int NCH, class F>
__device__ __forceinline__ void for_each_class(int k, int lane, F &&f) {  // f(c, j): ascending j within the lane
  if constexpr (NCH > 0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = c * kWave + lane;
      if (j < k) f(c, j);
    }
  } else {
    for (int j = lane; j < k; j += kWave) f(0, j);
  }
}

template <int NCH>
__device__ __forceinline__ float wide_x(const WideRow<NCH> &r, const float *__restrict__ row, int c, int j) {
  if constexpr (NCH > 0) return r.x[c];
  else return row[j];
}
template <int NCH>
__device__ __forceinline__ float wide_p(const WideRow<NCH> &r, const float *__restrict__ row, int c, int j) {
  if constexpr (NCH > 0) return r.p[c];
  else return expf((row[j] - r.lse) - r.mx2) / r.s2;
}

// categorical_normalise_dyn<false> (device_math.hip.h) across the wave; returns sum_j entropy_logit(nl_j) p_j when
// `with_entropy`.
template <int NCH>
__device__ __forceinline__ float wide_normalise(const float *__restrict__ row, int k, int lane, bool with_entropy,
                                                WideRow<NCH> &r) {
  float mx = -INFINITY;
  for_each_class<NCH>(k, lane, [&](int c, int j) {
    const float v = row[j];
    if constexpr (NCH > 0) r.x[c] = v;
    mx = v > mx ? v : mx;
  });
  mx = wave_max(mx);
  float s = 0.0f;
  for_each_class<NCH>(k, lane, [&](int c, int j) { s += expf(wide_x<NCH>(r, row, c, j) - mx); });
  r.lse = mx + logf(wave_sum(s));
  r.mx2 = mx - r.lse;  // (= max_j nl_j: a rounded subtraction is monotone)
  float s2 = 0.0f;
  for_each_class<NCH>(k, lane, [&](int c, int j) {
    const float e = expf((wide_x<NCH>(r, row, c, j) - r.lse) - r.mx2);
    if constexpr (NCH > 0) r.p[c] = e;
    s2 += e;
  });
  r.s2 = wave_sum(s2);
  if constexpr (NCH > 0) for_each_class<NCH>(k, lane, [&](int c, int) { r.p[c] = r.p[c] / r.s2; });
  float e = 0.0f;
  if (with_entropy) {
    for_each_class<NCH>(k, lane, [&](int c, int j) {
      e += entropy_logit(wide_x<NCH>(r, row, c, j) - r.lse) * wide_p<NCH>(r, row, c, j);
    });
    e = wave_sum(e);
  }
  return e;
}

// Arithmetic per element: ppo_loss_categorical_generic_kernel (ppo_loss_kernels.hip).  All 64 lanes carry the sample's
// scalars (logp, entropy, the policy and value terms: the same bits in every lane); lane 0 adds them to the loss sums
// and writes grad_value.
template <int NCH, bool HAS_GRAD>
__global__ __launch_bounds__(kBlock) void ppo_loss_categorical_wide_kernel(
    const float *__restrict__ logits, const float *__restrict__ value, const int64_t *__restrict__ action,
    const float *__restrict__ logp_old, const float *__restrict__ adv, const float *__restrict__ ret, int64_t m, int a,
    int k, rl8_ppo_hparams hp, float *__restrict__ grad_logits, float *__restrict__ grad_value,
    double *__restrict__ partials, double *__restrict__ sums_out) {
  __shared__ double smem[kLossCols * kWavesPerBlock];
  double acc[kLossCols] = {0.0, 0.0, 0.0, 0.0};
  const bool with_entropy = hp.entropy_coeff != 0.0f;
  for_each_wave_row(m, [&](int64_t i, int lane) {
    WideRow<NCH> r;
    float logp = 0.0f, ent = 0.0f, hd = 0.0f;
    for (int d = 0; d < a; ++d) {
      const float *row = logits + (i * a + d) * k;
      hd = -wide_normalise<NCH>(row, k, lane, with_entropy, r);
      int64_t ai = action[i * a + d];
      ai = ai < 0 ? 0 : (ai >= k ? k - 1 : ai);
      const float l = row[ai] - r.lse;
      logp = d == 0 ? l : logp + l;
      if (with_entropy) ent = d == 0 ? hd : ent + hd;
    }
    const PolicyTerm pt = ppo_policy_term(logp, logp_old[i], adv[i], hp);
    float dv;
    const float vterm = ppo_vf_term(value[i], ret[i], hp, &dv);
    if (lane == 0) {
      acc[0] += (double)ent;
      acc[1] += (double)pt.term;
      acc[2] += (double)vterm;
      acc[3] += (double)pt.kl;
    }
    if constexpr (HAS_GRAD) {
      if (lane == 0) grad_value[i] = hp.grad_scale * hp.vf_coeff * dv;
      for (int d = 0; d < a; ++d) {
        const float *row = logits + (i * a + d) * k;
        // (one action dimension: the row, lse, s2 and the entropy of the forward half are still in registers)
        if (a > 1) hd = -wide_normalise<NCH>(row, k, lane, with_entropy, r);
        const int64_t act = action[i * a + d];
        float *g = grad_logits + (i * a + d) * k;
        for_each_class<NCH>(k, lane, [&](int c, int j) {
          const float p = wide_p<NCH>(r, row, c, j);
          const float dlogp = (j == act ? 1.0f : 0.0f) - p;
          float gj = -pt.dterm_dlogp * dlogp;
          if (with_entropy)
            gj -= hp.entropy_coeff * (-p * (entropy_logit(wide_x<NCH>(r, row, c, j) - r.lse) + hd));
          g[j] = hp.grad_scale * gj;
        });
      }
    }
  });
  block_reduce<kLossCols, SumOp>(acc, smem);
  publish_loss_row(acc, partials, blockIdx.x, gridDim.x, (double)m, sums_out, smem);
}

// Workgroups of four waves, one sample per wave and pass (RL8_LOSS_GRID_CAP: the tuning knob of the loss kernels).
int wide_loss_grid(int64_t m) {
  int grid = grid_for(m, kWavesPerBlock);
  static int cap = -1;
  if (cap < 0) {
    const char *v = getenv("RL8_LOSS_GRID_CAP");
    cap = v ? atoi(v) : 0;
  }
  if (cap > 0) {
    const int64_t gg = (m + kWavesPerBlock - 1) / kWavesPerBlock;
    grid = (int)(gg < cap ? gg : cap);
    if (grid > RL8_MAX_PARTIALS) grid = RL8_MAX_PARTIALS;
    if (grid < 1) grid = 1;
  }
  return grid;
}

int wide_sizes_status(int64_t m, int a, int k) {
  if (m <= 0 || a <= 0 || k < 2 || k > RL8_MAX_WIDE_CLASSES) return RL8_ESIZE;
  if ((int64_t)a * k >= ((int64_t)1 << 31)) return RL8_ESIZE;  // (the Philox word d k + j and the int class index)
  return RL8_OK;
}

}  // namespace
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_categorical_wide_sample_logp_f32(const float *logits, const float *noise, int64_t *action_out,
                                                 float *logp_out, int64_t m, int a, int k, uint64_t seed, uint64_t step,
                                                 int64_t row_offset, int deterministic, void *stream) {
  if (!logits || !action_out || !logp_out) return RL8_ENULL;
  const int st = wide_sizes_status(m, a, k);
  if (st != RL8_OK) return st;
  categorical_wide_sample_kernel<<<grid_for(m, kWavesPerBlock), kBlock, 0, (hipStream_t)stream>>>(
      logits, noise, action_out, logp_out, m, a, k, seed, step, row_offset, deterministic);
  return launch_status();
}

RL8_API int rl8_ppo_loss_categorical_wide_fwd_bwd_f32(const float *logits, const float *value, const int64_t *action,
                                                      const float *logp_old, const float *adv, const float *ret,
                                                      int64_t m, int a, int k, const rl8_ppo_hparams *hp,
                                                      float *grad_logits, float *grad_value, double *loss_sums_out,
                                                      void *scratch, void *stream) {
  if (!logits || !value || !action || !logp_old || !adv || !ret || !loss_sums_out || !scratch) return RL8_ENULL;
  if ((grad_logits == nullptr) != (grad_value == nullptr)) return RL8_ENULL;
  int st = wide_sizes_status(m, a, k);
  if (st != RL8_OK) return st;
  st = check_ppo_hparams(hp);
  if (st != RL8_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  double *partials = (double *)scratch;
  const int grid = wide_loss_grid(m);
#define RL8_LAUNCH_WIDE(NCH)                                                                                          \
  do {                                                                                                                \
    if (grad_logits)                                                                                                  \
      ppo_loss_categorical_wide_kernel<NCH, true><<<grid, kBlock, 0, s>>>(                                            \
          logits, value, action, logp_old, adv, ret, m, a, k, *hp, grad_logits, grad_value, partials, loss_sums_out); \
    else                                                                                                              \
      ppo_loss_categorical_wide_kernel<NCH, false><<<grid, kBlock, 0, s>>>(                                           \
          logits, value, action, logp_old, adv, ret, m, a, k, *hp, nullptr, nullptr, partials, loss_sums_out);        \
  } while (0)
  // the row in registers up to 1024 classes (NCH chunks of 64, a power of two), read again beyond
  if (k <= 1 * kWave) RL8_LAUNCH_WIDE(1);
  else if (k <= 2 * kWave) RL8_LAUNCH_WIDE(2);
  else if (k <= 4 * kWave) RL8_LAUNCH_WIDE(4);
  else if (k <= 8 * kWave) RL8_LAUNCH_WIDE(8);
  else if (k <= 16 * kWave) RL8_LAUNCH_WIDE(16);
  else RL8_LAUNCH_WIDE(0);
#undef RL8_LAUNCH_WIDE
  return launch_status();
}
