// The narrow towers' forward, backward and reduce launches behind the C ABI (kernels: mlp_narrow.hip.h; the backward
// that also forms dx is launched from mlp_narrow_dx_kernels.hip).
#include "mlp_narrow.hip.h"

namespace rl8 {
namespace narrow {

// grads[e] = sum over the slabs, in slab order, in fp64 (db3: high and low parts).
__global__ __launch_bounds__(kThreads) void mlp_narrow_reduce_kernel(const float *__restrict__ slabs, int slab_count,
                                                                     int floats, int n_out, float *__restrict__ grads) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= floats) return;
  const int stride = floats + n_out;
  const bool b3 = e >= floats - n_out;
  double s = 0.0;
  for (int g = 0; g < slab_count; ++g) {
    s += (double)slabs[(int64_t)g * stride + e];
    if (b3) s += (double)slabs[(int64_t)g * stride + e + n_out];
  }
  grads[e] = (float)s;
}

template <int H, int KIN, int KOUT>
int launch_forward(hipStream_t s, const float *x, int64_t m, int d_in, const float *w1, const float *b1,
                   const float *w2, const float *b2, const float *w3, const float *b3, int n_out, float *out) {
  constexpr size_t bytes = forward_lds_floats<H, KIN, KOUT>() * sizeof(float);
  static_assert(bytes * Geo<H>::kWgPerCU <= 160 * 1024, "forward LDS");
  constexpr auto *kernel = &mlp_narrow_forward_kernel<H, KIN, KOUT>;
  if (const int e = allow_dynamic_lds<kernel>((int)bytes)) return e;
  kernel<<<grid_for<H>(m), kThreads, bytes, s>>>(x, m, d_in, w1, b1, w2, b2, w3, b3, n_out, out);
  return launch_status();
}

template <int H, int KIN, int KOUT>
int launch_backward(hipStream_t s, const float *x, const float *dout, int64_t m, int d_in, const float *w1,
                    const float *b1, const float *w2, const float *b2, const float *w3, int n_out, float *slabs) {
  constexpr size_t bytes = backward_lds_floats<H, KIN, KOUT>() * sizeof(float);
  static_assert(bytes * Geo<H>::kWgPerCU <= 160 * 1024, "backward LDS");
  constexpr auto *kernel = &mlp_narrow_backward_kernel<H, KIN, KOUT>;
  if (const int e = allow_dynamic_lds<kernel>((int)bytes)) return e;
  kernel<<<grid_for<H>(m), kThreads, bytes, s>>>(x, dout, m, d_in, w1, b1, w2, b2, w3, n_out, slabs, nullptr);
  return launch_status();
}

template <int H, int KIN, int KOUT>
struct Forward {
  template <typename... A>
  static int run(A... args) { return launch_forward<H, KIN, KOUT>(args...); }
};
template <int H, int KIN, int KOUT>
struct Backward {
  template <typename... A>
  static int run(A... args) { return launch_backward<H, KIN, KOUT>(args...); }
};

inline int grad_floats_rt(int hidden, int d_in, int n_out) {
  return hidden == 64 ? grad_floats<64>(d_in, n_out) : grad_floats<128>(d_in, n_out);
}
inline int slab_floats_rt(int hidden, int d_in, int n_out) {
  return hidden == 64 ? slab_floats<64>(d_in, n_out) : slab_floats<128>(d_in, n_out);
}

inline int grid_rt(int hidden, int64_t m) { return hidden == 64 ? grid_for<64>(m) : grid_for<128>(m); }

}  // namespace narrow
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_mlp_narrow_supports(int hidden, int d_in, int n_out) {
  return (hidden == 64 || hidden == 128) && d_in >= 1 && d_in <= kMaxIn && n_out >= 1 && n_out <= kMaxOut;
}

RL8_API int64_t rl8_mlp_narrow_workspace_bytes(int64_t m, int hidden, int d_in, int n_out) {
  if (m < 1 || !rl8_mlp_narrow_supports(hidden, d_in, n_out)) return RL8_ESIZE;
  return (int64_t)narrow::grid_rt(hidden, m) * narrow::slab_floats_rt(hidden, d_in, n_out) * (int64_t)sizeof(float);
}

RL8_API int rl8_mlp_narrow_forward_f32(const float *x, int64_t m, int d_in, const float *w1, const float *b1,
                                       const float *w2, const float *b2, const float *w3, const float *b3, int n_out,
                                       int hidden, float *out, void *stream) {
  if (!x || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !out) return RL8_ENULL;
  if (m < 1 || !rl8_mlp_narrow_supports(hidden, d_in, n_out)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)w1, (const void *)b1, (const void *)w2, (const void *)b2,
                        (const void *)w3, (const void *)b3, (const void *)out})
    if (!narrow::aligned4(p)) return RL8_EALIGN;
  return narrow::dispatch<narrow::Forward>(hidden, d_in, n_out, (hipStream_t)stream, x, m, d_in, w1, b1, w2, b2, w3,
                                           b3, n_out, out);
}

RL8_API int rl8_mlp_narrow_backward_f32(const float *x, const float *dout, int64_t m, int d_in, const float *w1,
                                        const float *b1, const float *w2, const float *b2, const float *w3, int n_out,
                                        int hidden, float *workspace, void *stream) {
  if (!x || !dout || !w1 || !b1 || !w2 || !b2 || !w3 || !workspace) return RL8_ENULL;
  if (m < 1 || !rl8_mlp_narrow_supports(hidden, d_in, n_out)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)dout, (const void *)w1, (const void *)b1, (const void *)w2,
                        (const void *)b2, (const void *)w3, (const void *)workspace})
    if (!narrow::aligned4(p)) return RL8_EALIGN;
  return narrow::dispatch<narrow::Backward>(hidden, d_in, n_out, (hipStream_t)stream, x, dout, m, d_in, w1, b1, w2, b2,
                                            w3, n_out, workspace);
}

RL8_API int rl8_mlp_narrow_reduce_f32(const float *workspace, int64_t m, int hidden, int d_in, int n_out,
                                      float *grads_out, void *stream) {
  if (!workspace || !grads_out) return RL8_ENULL;
  if (m < 1 || !rl8_mlp_narrow_supports(hidden, d_in, n_out)) return RL8_ESIZE;
  if (!narrow::aligned4(workspace) || !narrow::aligned4(grads_out)) return RL8_EALIGN;
  const int floats = narrow::grad_floats_rt(hidden, d_in, n_out);
  narrow::mlp_narrow_reduce_kernel<<<(floats + narrow::kThreads - 1) / narrow::kThreads, narrow::kThreads, 0,
                                     (hipStream_t)stream>>>(workspace, narrow::grid_rt(hidden, m), floats, n_out, grads_out);
  return launch_status();
}
