// The hand-off of the fused PPO loss kernels (ppo_loss_kernels.hip, categorical_wide_kernels.hip): every block
// publishes one row of four fp64 sums, the last block to arrive adds the rows in row order.
#pragma once

#include "common.hip.h"

namespace rl8 {

constexpr int kLossCols = 4;  // entropy, policy, vf, kl

// Publishes this block's row; the last block to arrive sums rows [0, rows) in
// order and writes out[0..4] = sum entropy, policy, vf, sample count, sum kl.
__device__ __forceinline__ void publish_loss_row(double (&acc)[kLossCols], double *partials,
                                                 int row, int rows, double count, double *out,
                                                 double *smem) {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < kLossCols; ++c)
      publish_partial(partials + (int64_t)row * kPartialWidth + c, acc[c]);
  }
  if (!last_block_arrives(ticket_word(partials))) return;
  double tot[kLossCols] = {0.0, 0.0, 0.0, 0.0};
  fold_partial_rows<kLossCols>(partials, rows, [&](const double(&v)[kLossCols]) {
#pragma unroll
    for (int c = 0; c < kLossCols; ++c) tot[c] += v[c];
  });
  block_reduce<kLossCols, SumOp>(tot, smem);
  if (threadIdx.x == 0) {
    out[0] = tot[0];
    out[1] = tot[1];
    out[2] = tot[2];
    out[3] = count;
    out[4] = tot[3];
    *ticket_word(partials) = 0u;
  }
}

inline int check_ppo_hparams(const rl8_ppo_hparams *hp) {
  if (!hp) return RL8_ENULL;
  if (!(hp->clip_param > 0.0f && hp->clip_param < 1.0f)) return RL8_ECONFIG;
  if (!(hp->vf_clip_param > 0.0f)) return RL8_ECONFIG;
  return RL8_OK;
}

}  // namespace rl8
