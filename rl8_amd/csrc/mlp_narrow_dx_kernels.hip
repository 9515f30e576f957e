// rl8_mlp_narrow_backward_dx_f32: the narrow towers' backward with the gradient of x (the DX instantiations of
// mlp_narrow_backward_kernel, mlp_narrow.hip.h).  A translation unit of its own, so that the instantiations without dx
// are compiled exactly as before.
#include "mlp_narrow.hip.h"

namespace rl8 {
namespace narrow {

template <int H, int KIN, int KOUT>
int launch_backward_dx(hipStream_t s, const float *x, const float *dout, int64_t m, int d_in, const float *w1,
                       const float *b1, const float *w2, const float *b2, const float *w3, int n_out, float *slabs,
                       float *dx) {
  constexpr size_t bytes = (backward_lds_floats<H, KIN, KOUT>() + (size_t)H * (KIN + 4)) * sizeof(float);
  static_assert(bytes * Geo<H>::kWgPerCU <= 160 * 1024, "backward LDS with the W1 tile");
  constexpr auto *kernel = &mlp_narrow_backward_kernel<H, KIN, KOUT, true>;
  if (const int e = allow_dynamic_lds<kernel>((int)bytes)) return e;
  kernel<<<grid_for<H>(m), kThreads, bytes, s>>>(x, dout, m, d_in, w1, b1, w2, b2, w3, n_out, slabs, dx);
  return launch_status();
}

template <int H, int KIN, int KOUT>
struct BackwardDx {
  template <typename... A>
  static int run(A... args) { return launch_backward_dx<H, KIN, KOUT>(args...); }
};

}  // namespace narrow
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_mlp_narrow_backward_dx_f32(const float *x, const float *dout, int64_t m, int d_in, const float *w1,
                                           const float *b1, const float *w2, const float *b2, const float *w3,
                                           int n_out, int hidden, float *workspace, float *dx, void *stream) {
  if (!dx) return rl8_mlp_narrow_backward_f32(x, dout, m, d_in, w1, b1, w2, b2, w3, n_out, hidden, workspace, stream);
  if (!x || !dout || !w1 || !b1 || !w2 || !b2 || !w3 || !workspace) return RL8_ENULL;
  if (m < 1 || !rl8_mlp_narrow_supports(hidden, d_in, n_out)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)dout, (const void *)w1, (const void *)b1, (const void *)w2,
                        (const void *)b2, (const void *)w3, (const void *)workspace, (const void *)dx})
    if (!narrow::aligned4(p)) return RL8_EALIGN;
  return narrow::dispatch<narrow::BackwardDx>(hidden, d_in, n_out, (hipStream_t)stream, x, dout, m, d_in, w1, b1, w2,
                                              b2, w3, n_out, workspace, dx);
}

