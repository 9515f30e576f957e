// Host launchers of lstm_narrow_kernels.hip that lstm_narrow_wide_in_kernels.hip calls: the recurrent forward from a
// pre-formed zin and the backward through time know nothing of x, so a family with another input width launches them
// as they are.  Defined at the end of lstm_narrow_kernels.hip; not exported from the library (hidden visibility).
#pragma once

#include "common.hip.h"

namespace rl8 {
namespace lstm_narrow {

// b >= 1, l >= 1 and the 32-bit descriptor offsets of the narrow kernels hold (rl8_lstm_narrow_* return RL8_ESIZE).
bool shared_sizes_ok(int64_t b, int l, int hidden);
// Sequences per weight-gradient chunk and the chunk (slab) count for `hidden` = 64 or 128: functions of b alone.
void shared_chunks(int hidden, int64_t b, int64_t *per, int *count);
// lstm_narrow_stack_forward_kernel: zin [b][l][4][H] -> hs, hn, cn (save_gates / save_c both or neither).
int shared_recurrent_forward(hipStream_t s, int hidden, const float *zin, int64_t b, int l, const float *h0,
                             const float *c0, const float *w_hh, float *hs, float *hn, float *cn, float *save_gates,
                             float *save_c);
// lstm_narrow_backward_kernel (heads_dout == nullptr: dL/dh from dhs) or lstm_narrow_backward_heads_kernel: dz out.
int shared_backward(hipStream_t s, int hidden, int64_t b, int l, const float *c0, const float *w_hh,
                    const float *gates, const float *cs, const float *dhs, const float *heads_dout,
                    const float *heads_w, float *dz);

}  // namespace lstm_narrow
}  // namespace rl8
