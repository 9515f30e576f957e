// LSTM gate non-linearities shared by the fp32 LSTM kernels (lstm_kernels.hip,
// lstm_narrow_kernels.hip), on the hardware exp2 / rcp (1 ulp each; the
// reference's tolerance is 1e-5): sigmoid(x) = 1 / (1 + e^-x),
// tanh(x) = 1 - 2 / (e^2x + 1).
#pragma once

#include <hip/hip_runtime.h>

namespace rl8 {

__device__ __forceinline__ float sigmoid_f(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
__device__ __forceinline__ float tanh_f(float x) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f);
}

}  // namespace rl8
