// The block every SelfAttention / CrossAttention ends with, fused per token (rl8_amd/nn/fused_feedforward.py):
//   n   = LayerNorm_F(x; gamma, beta, eps)         biased variance, rstd = 1 / sqrt(var + eps)
//   out = (residual ? x : 0) + W2 act(W1 n + b1) + b2
// on rows x [R][F], W1 [H][F], W2 [F][H] (nn.Linear's layout), F <= 32, H <= 256, act = ReLU, fp32.
// Compiled with -ffp-contract=off: every multiply-add that is meant to be one instruction is an fmaf.
//
// Forward and dx: one lane per token, F a template parameter, the loop over hidden units inside the lane; the token's x,
// n, dout and accumulators are registers and the hidden vector never exists in memory.  The weights are wave-uniform and
// come through scalar loads: W1's row j is F consecutive floats, W2's column j is read where it lies, at stride H (no
// transposed copy, no LDS).  The backward saves nothing but x: n and every z_j are formed again by the functions the
// forward uses (layer_norm, pre_activation), so that all kernels agree on every gate bit for bit.
//
// Parameter gradients, the same bits on every run (no atomics): partial sums over row slices that depend on the shape
// only, written to a workspace, summed in fp64 in a fixed order by a second launch.
//   dW1, db1, dW2, db2: feedforward_wgrad_kernel, one lane per hidden unit with W1[j], W2[:, j] and their 2F + 1
//     accumulators in registers; the workgroup stages n and dout of kWgradRows tokens in LDS and every lane reads them
//     as broadcasts.  With H <= 128 the 256 lanes are 2 or 4 groups of hidden units that take the staged tokens in turn.
//   dgamma, dbeta: dn = W1^T dz exists per token in the dx kernel and nowhere else, so that kernel sums dn xhat and dn
//     over its lane's tokens and over the wave (lane shuffles, no LDS) and writes one partial row per wave.
#include <math.h>

#include "common.hip.h"

namespace rl8 {
namespace {

constexpr int kMaxF = 32;
constexpr int kMaxHidden = 256;
constexpr int kWgradRows = kBlock;    // tokens a workgroup of the wgrad kernel stages at a time (one per thread)
constexpr int kWgradMaxGrid = 512;    // 2 workgroups per CU
constexpr int kSumSplit = 16;         // row interleaves of the final sum
constexpr int kSumElems = kBlock / kSumSplit;

struct Relu {
  // NaN goes through, as torch.relu's; -0 becomes +0.
  __device__ __forceinline__ static float apply(float z) { return !(z <= 0.0f) ? z : 0.0f; }
  // torch's gate: closed at exactly 0.
  __device__ __forceinline__ static float gate(float z, float da) { return z > 0.0f ? da : 0.0f; }
};

// xhat = (x - mean) rstd and n = xhat gamma + beta of one row; the variance from the centred values (two passes).
// x may alias xhat.
template <int F>
__device__ __forceinline__ float layer_norm(const float (&x)[F], const float *__restrict__ gamma,
                                            const float *__restrict__ beta, float eps, float (&xhat)[F], float (&n)[F]) {
  float mean = 0.0f;
#pragma unroll
  for (int c = 0; c < F; ++c) mean = mean + x[c];
  mean = mean * (1.0f / F);
  float var = 0.0f;
#pragma unroll
  for (int c = 0; c < F; ++c) {
    xhat[c] = x[c] - mean;
    var = fmaf(xhat[c], xhat[c], var);
  }
  const float rstd = 1.0f / sqrtf(var * (1.0f / F) + eps);
#pragma unroll
  for (int c = 0; c < F; ++c) {
    xhat[c] = xhat[c] * rstd;
    n[c] = fmaf(xhat[c], gamma[c], beta[c]);
  }
  return rstd;
}

// z_j = b1[j] + W1[j] . n, the features in ascending order: the ONE place it is formed (n and w are anything indexable).
template <int F, class N, class W>
__device__ __forceinline__ float pre_activation(const N &n, const W &w, float b) {
  float z = b;
#pragma unroll
  for (int c = 0; c < F; ++c) z = fmaf(n[c], w[c], z);
  return z;
}

template <int F>
__device__ __forceinline__ void load_row(const float *__restrict__ p, float (&x)[F]) {
#pragma unroll
  for (int c = 0; c < F; ++c) x[c] = p[c];
}

template <int F, class Act>
__global__ __launch_bounds__(kBlock) void feedforward_forward_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
    const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2,
    const float *__restrict__ b2, int64_t rows, int hidden, int residual, float *__restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += stride) {
    float xr[F], xhat[F], n[F], acc[F];
    load_row(x + r * F, xr);
    layer_norm(xr, gamma, beta, eps, xhat, n);
#pragma unroll
    for (int c = 0; c < F; ++c) acc[c] = b2[c];
    for (int j = 0; j < hidden; ++j) {
      const float a = Act::apply(pre_activation<F>(n, w1 + j * F, b1[j]));
#pragma unroll
      for (int c = 0; c < F; ++c) acc[c] = fmaf(a, w2[c * hidden + j], acc[c]);
    }
    float *o = out + r * F;
#pragma unroll
    for (int c = 0; c < F; ++c) o[c] = residual ? xr[c] + acc[c] : acc[c];
  }
}

// dx of one token from x and dout; with LN, the wave's sums of dn xhat (dgamma) and dn (dbeta) to
// ln_partials[(block 4 + wave)][2F] as well.  dx may be NULL when only those are wanted.
template <int F, class Act, bool LN>
__global__ __launch_bounds__(kBlock) void feedforward_backward_x_kernel(
    const float *__restrict__ x, const float *__restrict__ dout, const float *__restrict__ gamma,
    const float *__restrict__ beta, float eps, const float *__restrict__ w1, const float *__restrict__ b1,
    const float *__restrict__ w2, int64_t rows, int hidden, int residual, float *__restrict__ dx,
    float *__restrict__ ln_partials) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  float sg[LN ? F : 1], sb[LN ? F : 1];
  if (LN) {
#pragma unroll
    for (int c = 0; c < F; ++c) sg[c] = sb[c] = 0.0f;
  }
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += stride) {
    float xhat[F], n[F], g[F], dn[F];
    load_row(x + r * F, xhat);
    load_row(dout + r * F, g);
    const float rstd = layer_norm(xhat, gamma, beta, eps, xhat, n);
#pragma unroll
    for (int c = 0; c < F; ++c) dn[c] = 0.0f;
    for (int j = 0; j < hidden; ++j) {
      const float z = pre_activation<F>(n, w1 + j * F, b1[j]);
      float da = 0.0f;
#pragma unroll
      for (int c = 0; c < F; ++c) da = fmaf(w2[c * hidden + j], g[c], da);
      const float dz = Act::gate(z, da);
#pragma unroll
      for (int c = 0; c < F; ++c) dn[c] = fmaf(w1[j * F + c], dz, dn[c]);
    }
    if (LN) {
#pragma unroll
      for (int c = 0; c < F; ++c) {
        sg[c] = fmaf(dn[c], xhat[c], sg[c]);
        sb[c] = sb[c] + dn[c];
      }
    }
    if (dx) {
      // dx = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)), dxhat = dn gamma
      float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
      for (int c = 0; c < F; ++c) {
        dn[c] = dn[c] * gamma[c];
        m1 = m1 + dn[c];
        m2 = fmaf(dn[c], xhat[c], m2);
      }
      m1 = m1 * (1.0f / F);
      m2 = m2 * (1.0f / F);
      float *o = dx + r * F;
#pragma unroll
      for (int c = 0; c < F; ++c) {
        const float d = rstd * ((dn[c] - m1) - xhat[c] * m2);
        o[c] = residual ? g[c] + d : d;
      }
    }
  }
  if (LN) {
    // (every lane is back here, also those that had no row: they add 0)
#pragma unroll
    for (int c = 0; c < F; ++c) {
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) {
        sg[c] = sg[c] + __shfl_down(sg[c], off, kWave);
        sb[c] = sb[c] + __shfl_down(sb[c], off, kWave);
      }
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
      float *p = ln_partials + ((int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave) * (2 * F);
#pragma unroll
      for (int c = 0; c < F; ++c) {
        p[c] = sg[c];
        p[F + c] = sb[c];
      }
    }
  }
}

// Lanes of the wgrad kernel: `lanes` = H rounded up to 64, 128 or 256 hidden-unit lanes, 256 / lanes groups of them.
inline int wgrad_lanes(int hidden) { return hidden <= 64 ? 64 : hidden <= 128 ? 128 : 256; }
inline int wgrad_groups(int hidden) { return kBlock / wgrad_lanes(hidden); }
// Floats of one partial row, laid out as the outputs are: dW1 [H][F], db1 [H], dW2 [F][H], db2 [F].
inline int64_t wgrad_row_floats(int f, int hidden) { return 2 * (int64_t)f * hidden + hidden + f; }

// One partial row per (workgroup, group) at partials[(block groups + group)]: the sums over the tokens that group took
// of the workgroup's chunks (chunk = blockIdx, blockIdx + grid, ...; inside a chunk, token = group, group + groups, ...).
template <int F, class Act>
__global__ __launch_bounds__(kBlock) void feedforward_wgrad_kernel(
    const float *__restrict__ x, const float *__restrict__ dout, const float *__restrict__ gamma,
    const float *__restrict__ beta, float eps, const float *__restrict__ w1, const float *__restrict__ b1,
    const float *__restrict__ w2, int64_t rows, int hidden, int lanes, float *__restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float n_s[kWgradRows][F];
  __shared__ __attribute__((aligned(16))) float g_s[kWgradRows][F];
  const int groups = kBlock / lanes;
  const int j = threadIdx.x % lanes, group = threadIdx.x / lanes;  // (a wave lies inside one group)
  const bool unit = j < hidden, feature = j < F;
  float w1r[F], w2r[F], dw1[F], dw2[F];
#pragma unroll
  for (int c = 0; c < F; ++c) {
    w1r[c] = unit ? w1[j * F + c] : 0.0f;
    w2r[c] = unit ? w2[c * hidden + j] : 0.0f;
    dw1[c] = dw2[c] = 0.0f;
  }
  const float b1r = unit ? b1[j] : 0.0f;
  float db1 = 0.0f, db2 = 0.0f;
  const int64_t chunks = (rows + kWgradRows - 1) / kWgradRows;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const int64_t base = chunk * kWgradRows;
    const int count = (int)(rows - base < kWgradRows ? rows - base : kWgradRows);
    __syncthreads();  // (the previous chunk has been read)
    if ((int)threadIdx.x < count) {
      float xhat[F], n[F];
      load_row(x + (base + threadIdx.x) * F, xhat);
      layer_norm(xhat, gamma, beta, eps, xhat, n);
      const float *g = dout + (base + threadIdx.x) * F;
#pragma unroll
      for (int c = 0; c < F; ++c) {
        n_s[threadIdx.x][c] = n[c];
        g_s[threadIdx.x][c] = g[c];
      }
    }
    __syncthreads();
    for (int t = group; t < count; t += groups) {
      const float z = pre_activation<F>(n_s[t], w1r, b1r);
      const float a = Act::apply(z);
      float da = 0.0f;
#pragma unroll
      for (int c = 0; c < F; ++c) da = fmaf(w2r[c], g_s[t][c], da);
      const float dz = Act::gate(z, da);
#pragma unroll
      for (int c = 0; c < F; ++c) {
        dw1[c] = fmaf(dz, n_s[t][c], dw1[c]);
        dw2[c] = fmaf(g_s[t][c], a, dw2[c]);
      }
      db1 = db1 + dz;
      if (feature) db2 = db2 + g_s[t][j];
    }
  }
  float *p = partials + ((int64_t)blockIdx.x * groups + group) * (2 * (int64_t)F * hidden + hidden + F);
  if (unit) {
#pragma unroll
    for (int c = 0; c < F; ++c) {
      p[j * F + c] = dw1[c];
      p[F * hidden + hidden + c * hidden + j] = dw2[c];
    }
    p[F * hidden + j] = db1;
  }
  if (feature) p[2 * F * hidden + hidden + j] = db2;
}

// The outputs of the final sum: element e of a partial row of `row_floats` belongs to the one whose range holds it.
struct SumTargets {
  float *dw1, *db1, *dw2, *db2;  // each may be NULL: not written
  float *dgamma, *dbeta;
};

// out[e] = sum over partial rows, rows kSumSplit apart in ascending order in fp64, the kSumSplit sums then in order.
__global__ __launch_bounds__(kBlock) void feedforward_sum_kernel(const float *__restrict__ w_partials, int w_rows,
                                                               const float *__restrict__ ln_partials, int ln_rows,
                                                               int f, int hidden, SumTargets to) {
  __shared__ double part[kSumSplit][kSumElems];
  const int w_floats = 2 * f * hidden + hidden + f;
  const int e = blockIdx.x * kSumElems + threadIdx.x % kSumElems, split = threadIdx.x / kSumElems;
  const bool is_w = e < w_floats, is_ln = !is_w && e < w_floats + 2 * f;
  const float *src = is_w ? w_partials : ln_partials;  // (NULL: that half is not wanted)
  const int at = is_w ? e : e - w_floats;
  const int count = !src ? 0 : is_w ? w_rows : is_ln ? ln_rows : 0;
  const int64_t pitch = is_w ? w_floats : 2 * f;
  double s = 0.0;
#pragma unroll 8  // (loads in the air together; the additions stay in row order)
  for (int r = split; r < count; r += kSumSplit) s = s + (double)src[r * pitch + at];
  part[split][threadIdx.x % kSumElems] = s;
  __syncthreads();
  if (split != 0 || !(is_w || is_ln)) return;
#pragma unroll
  for (int q = 1; q < kSumSplit; ++q) s = s + part[q][threadIdx.x];
  float *dst;
  if (e < f * hidden) dst = to.dw1 ? to.dw1 + e : nullptr;
  else if (e < f * hidden + hidden) dst = to.db1 ? to.db1 + (e - f * hidden) : nullptr;
  else if (e < 2 * f * hidden + hidden) dst = to.dw2 ? to.dw2 + (e - f * hidden - hidden) : nullptr;
  else if (e < w_floats) dst = to.db2 ? to.db2 + (e - 2 * f * hidden - hidden) : nullptr;
  else if (e < w_floats + f) dst = to.dgamma ? to.dgamma + (e - w_floats) : nullptr;
  else dst = to.dbeta ? to.dbeta + (e - w_floats - f) : nullptr;
  if (dst) *dst = (float)s;
}

inline bool aligned_to(const void *p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// One instantiation per feature count: f.template operator()<F>().
template <class Fn>
inline void with_features(int f, Fn &&fn) {
  switch (f) {
#define RL8_FEATURES(F)          \
  case F:                        \
    fn.template operator()<F>(); \
    break;
    RL8_FEATURES(1) RL8_FEATURES(2) RL8_FEATURES(3) RL8_FEATURES(4) RL8_FEATURES(5) RL8_FEATURES(6) RL8_FEATURES(7)
    RL8_FEATURES(8) RL8_FEATURES(9) RL8_FEATURES(10) RL8_FEATURES(11) RL8_FEATURES(12) RL8_FEATURES(13)
    RL8_FEATURES(14) RL8_FEATURES(15) RL8_FEATURES(16) RL8_FEATURES(17) RL8_FEATURES(18) RL8_FEATURES(19)
    RL8_FEATURES(20) RL8_FEATURES(21) RL8_FEATURES(22) RL8_FEATURES(23) RL8_FEATURES(24) RL8_FEATURES(25)
    RL8_FEATURES(26) RL8_FEATURES(27) RL8_FEATURES(28) RL8_FEATURES(29) RL8_FEATURES(30) RL8_FEATURES(31)
    RL8_FEATURES(32)
#undef RL8_FEATURES
  }
}

inline int wgrad_grid(int64_t rows) { return grid_for(rows, kWgradRows, kWgradMaxGrid); }

struct ForwardLaunch {
  const float *x, *gamma, *beta;
  float eps;
  const float *w1, *b1, *w2, *b2;
  int64_t rows;
  int hidden, residual;
  float *out;
  hipStream_t stream;
  template <int F>
  void operator()() const {
    feedforward_forward_kernel<F, Relu><<<grid_for(rows, kBlock), kBlock, 0, stream>>>(
        x, gamma, beta, eps, w1, b1, w2, b2, rows, hidden, residual, out);
  }
};

struct BackwardLaunch {
  const float *x, *dout, *gamma, *beta;
  float eps;
  const float *w1, *b1, *w2;
  int64_t rows;
  int hidden, residual;
  float *dx;
  SumTargets to;
  float *workspace;
  hipStream_t stream;
  template <int F>
  void operator()() const {
    const bool want_ln = to.dgamma || to.dbeta, want_w = to.dw1 || to.db1 || to.dw2 || to.db2;
    const int x_grid = grid_for(rows, kBlock), w_grid = wgrad_grid(rows);
    const int w_rows = w_grid * wgrad_groups(hidden);
    float *ln_partials = workspace ? workspace + w_rows * wgrad_row_floats(F, hidden) : nullptr;
    if (want_ln)
      feedforward_backward_x_kernel<F, Relu, true><<<x_grid, kBlock, 0, stream>>>(
          x, dout, gamma, beta, eps, w1, b1, w2, rows, hidden, residual, dx, ln_partials);
    else if (dx)
      feedforward_backward_x_kernel<F, Relu, false><<<x_grid, kBlock, 0, stream>>>(
          x, dout, gamma, beta, eps, w1, b1, w2, rows, hidden, residual, dx, nullptr);
    if (want_w)
      feedforward_wgrad_kernel<F, Relu><<<w_grid, kBlock, 0, stream>>>(x, dout, gamma, beta, eps, w1, b1, w2, rows,
                                                                      hidden, wgrad_lanes(hidden), workspace);
    if (want_w || want_ln) {
      const int elems = (int)wgrad_row_floats(F, hidden) + 2 * F;
      feedforward_sum_kernel<<<(elems + kSumElems - 1) / kSumElems, kBlock, 0, stream>>>(
          want_w ? workspace : nullptr, w_rows, want_ln ? ln_partials : nullptr, x_grid * kWavesPerBlock, F, hidden, to);
    }
  }
};

}  // namespace
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_feedforward_supports(int f, int hidden) {
  if (f < 1 || hidden < 1) return RL8_ESIZE;
  return f <= kMaxF && hidden <= kMaxHidden ? 1 : 0;
}

RL8_API int rl8_feedforward_limits(int *limits) {
  if (!limits) return RL8_ENULL;
  limits[0] = kMaxGrid;
  limits[1] = kBlock;
  limits[2] = kWgradMaxGrid;
  limits[3] = kWgradRows;
  return RL8_OK;
}

RL8_API int64_t rl8_feedforward_workspace_floats(int64_t rows, int f, int hidden) {
  if (rows < 1 || f < 1 || hidden < 1) return RL8_ESIZE;
  if (rl8_feedforward_supports(f, hidden) != 1) return RL8_ECONFIG;
  return (int64_t)wgrad_grid(rows) * wgrad_groups(hidden) * wgrad_row_floats(f, hidden) +
         (int64_t)grid_for(rows, kBlock) * kWavesPerBlock * 2 * f;
}

RL8_API int rl8_feedforward_f32(const float *x, const float *gamma, const float *beta, float eps, const float *w1,
                                const float *b1, const float *w2, const float *b2, int64_t rows, int f, int hidden,
                                int residual, float *out, void *stream) {
  if (!x || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || !out) return RL8_ENULL;
  if (rows < 1 || f < 1 || hidden < 1) return RL8_ESIZE;
  if (!aligned_to(x, 4) || !aligned_to(gamma, 4) || !aligned_to(beta, 4) || !aligned_to(w1, 4) || !aligned_to(b1, 4) ||
      !aligned_to(w2, 4) || !aligned_to(b2, 4) || !aligned_to(out, 4))
    return RL8_EALIGN;
  if (rl8_feedforward_supports(f, hidden) != 1) return RL8_ECONFIG;
  with_features(f, ForwardLaunch{x, gamma, beta, eps, w1, b1, w2, b2, rows, hidden, residual != 0, out,
                                 (hipStream_t)stream});
  return launch_status();
}

RL8_API int rl8_feedforward_backward_f32(const float *x, const float *dout, const float *gamma, const float *beta,
                                         float eps, const float *w1, const float *b1, const float *w2, int64_t rows,
                                         int f, int hidden, int residual, float *dx, float *dgamma, float *dbeta,
                                         float *dw1, float *db1, float *dw2, float *db2, float *workspace,
                                         void *stream) {
  const bool want_params = dgamma || dbeta || dw1 || db1 || dw2 || db2;
  if (!x || !dout || !gamma || !beta || !w1 || !b1 || !w2 || (want_params && !workspace)) return RL8_ENULL;
  if (rows < 1 || f < 1 || hidden < 1) return RL8_ESIZE;
  if (!aligned_to(x, 4) || !aligned_to(dout, 4) || !aligned_to(gamma, 4) || !aligned_to(beta, 4) ||
      !aligned_to(w1, 4) || !aligned_to(b1, 4) || !aligned_to(w2, 4) || !aligned_to(dx, 4) || !aligned_to(dgamma, 4) ||
      !aligned_to(dbeta, 4) || !aligned_to(dw1, 4) || !aligned_to(db1, 4) || !aligned_to(dw2, 4) ||
      !aligned_to(db2, 4) || !aligned_to(workspace, 4))
    return RL8_EALIGN;
  if (rl8_feedforward_supports(f, hidden) != 1) return RL8_ECONFIG;
  if (!dx && !want_params) return RL8_OK;
  with_features(f, BackwardLaunch{x, dout, gamma, beta, eps, w1, b1, w2, rows, hidden, residual != 0, dx,
                                  SumTargets{dw1, db1, dw2, db2, dgamma, dbeta}, want_params ? workspace : nullptr,
                                  (hipStream_t)stream});
  return launch_status();
}
