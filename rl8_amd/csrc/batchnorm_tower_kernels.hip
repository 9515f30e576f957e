// A training-mode BatchNorm1d directly behind the first Linear of a narrow tower is an affine map of x whose
// coefficients are functions of the batch's first and second moments of x (d_in <= 16): with mu = mean_i x_i and
// C = (1/m) sum_i (x_i - mu)(x_i - mu)^T, unit j has batch mean m_j = W1_j . mu + b1_j and biased batch variance
// v_j = W1_j C W1_j^T, so y_j = a_j . x + c_j with r_j = 1 / sqrt(v_j + eps), s_j = gamma_j r_j, a_j = s_j W1_j and
// c_j = beta_j - s_j (W1_j . mu).  The tower then runs on mlp_narrow_kernels.hip with W1' = A, b1' = c.
//
// tower_moments_kernel: one pass over x.  A workgroup stages 64 rows of d = x - p (p = x[0], in fp64) in LDS; thread
// (i, j) of 16 x 16 owns S2[i][j] = sum d_i d_j and a copy of S1[j] = sum d_j, reading the staged row as two LDS
// broadcasts.  One slab [S1 (16) | S2 (256)] of doubles per workgroup; tower_moments_reduce_kernel adds the slabs in
// slab order and forms mu = p + S1 / m, C = S2 / m - (S1 / m)(S1 / m)^T.  No atomics; the grid is a function of m alone:
// the same bits on every run.  A constant column has d = 0 on every row, hence a row and a column of C that are exactly 0.
//
// batchnorm_fold_kernel: thread j forms unit j's coefficients in fp64 and rounds them once.
#include "common.hip.h"

namespace rl8 {
namespace bn {

constexpr int kD = 16;               // d_in padded
constexpr int kRows = 64;            // rows staged per step
constexpr int kGridCap = 2 * kCUs;   // slabs at most
constexpr int kSlab = kD + kD * kD;  // doubles per slab
constexpr int kPer = kRows * kD / kBlock;
constexpr int kFoldThreads = 128;

inline int moments_grid(int64_t m) {
  const int64_t tiles = (m + kRows - 1) / kRows;
  return (int)(tiles < kGridCap ? tiles : kGridCap);
}

// The tile's elements of this thread: element e = tid + 256 u is (row e / 16, column e % 16 = tid % 16).
__device__ __forceinline__ void fetch(const float *__restrict__ x, int64_t m, int d_in, int64_t tile, int tid, double pc,
                                      double (&v)[kPer]) {
  const int c = tid & (kD - 1);
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int64_t row = tile * kRows + (tid + kBlock * u) / kD;
    v[u] = (c < d_in && row < m) ? (double)x[row * d_in + c] - pc : 0.0;
  }
}

__global__ __launch_bounds__(kBlock) void tower_moments_kernel(const float *__restrict__ x, int64_t m, int d_in,
                                                                double *__restrict__ slabs) {
  __shared__ double ds[kRows * kD];
  const int tid = threadIdx.x, i = tid >> 4, j = tid & (kD - 1);
  const double pc = j < d_in ? (double)x[j] : 0.0;
  const int64_t tiles = (m + kRows - 1) / kRows;
  double s1 = 0.0, s2 = 0.0, v[kPer];
  fetch(x, m, d_in, blockIdx.x, tid, pc, v);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's readers are done
#pragma unroll
    for (int u = 0; u < kPer; ++u) ds[tid + kBlock * u] = v[u];
    if (tile + gridDim.x < tiles) fetch(x, m, d_in, tile + gridDim.x, tid, pc, v);
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < kRows; ++r) {
      const double a = ds[r * kD + i], b = ds[r * kD + j];
      s2 = fma(a, b, s2);
      s1 += b;
    }
  }
  double *slab = slabs + (int64_t)blockIdx.x * kSlab;
  if (i == 0) slab[j] = s1;
  slab[kD + tid] = s2;
}

// One entry of the slabs summed in slab order, eight loads in the air at a time (one load per add is latency, not bytes).
__device__ __forceinline__ double sum_slabs(const double *__restrict__ entry, int slab_count) {
  constexpr int kAhead = 8;
  double s = 0.0;
  int g = 0;
  for (; g + kAhead <= slab_count; g += kAhead) {
    double v[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) v[u] = entry[(int64_t)(g + u) * kSlab];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) s += v[u];
  }
  for (; g < slab_count; ++g) s += entry[(int64_t)g * kSlab];
  return s;
}

__global__ __launch_bounds__(kBlock) void tower_moments_reduce_kernel(const double *__restrict__ slabs, int slab_count,
                                                                       const float *__restrict__ x, int64_t m, int d_in,
                                                                       double *__restrict__ mu, double *__restrict__ cov) {
  __shared__ double mean[kD];
  const int tid = threadIdx.x, i = tid >> 4, j = tid & (kD - 1);
  const double s2 = sum_slabs(slabs + kD + tid, slab_count);
  if (tid < kD) {
    mean[tid] = sum_slabs(slabs + tid, slab_count) / (double)m;
    if (tid < d_in) mu[tid] = (double)x[tid] + mean[tid];
  }
  __syncthreads();
  if (i < d_in && j < d_in) cov[i * d_in + j] = s2 / (double)m - mean[i] * mean[j];
}

struct FoldArgs {
  const double *mu, *cov;
  int64_t m;
  int d_in, hidden;
  const float *w1, *b1, *gamma, *beta;
  double eps;
  float *running_mean, *running_var;
  double factor;
  const int64_t *tracked;
  float *a, *c;
  double *r, *m_z, *v;
};

template <bool TRAINING>
__global__ __launch_bounds__(kFoldThreads) void batchnorm_fold_kernel(FoldArgs p) {
  __shared__ double mus[kD], covs[kD * kD];
  const int j = threadIdx.x, d_in = p.d_in;
  if constexpr (TRAINING) {  // (the moments once into LDS: every unit reads all of them)
    for (int e = j; e < d_in * d_in; e += kFoldThreads) covs[e] = p.cov[e];
    if (j < d_in) mus[j] = p.mu[j];
    __syncthreads();
  }
  if (j >= p.hidden) return;
  const float *w = p.w1 + j * d_in;
  const double gamma = (double)p.gamma[j], beta = (double)p.beta[j];
  if constexpr (TRAINING) {
    double wm = 0.0, var = 0.0;
    for (int k = 0; k < d_in; ++k) wm = fma((double)w[k], mus[k], wm);
    for (int i = 0; i < d_in; ++i) {
      double t = 0.0;
      for (int k = 0; k < d_in; ++k) t = fma(covs[i * d_in + k], (double)w[k], t);
      var = fma((double)w[i], t, var);
    }
    var = var > 0.0 ? var : 0.0;  // (a quadratic form of a covariance: below 0 by rounding alone)
    const double r = 1.0 / sqrt(var + p.eps), s = gamma * r, mean = wm + (double)p.b1[j];
    for (int k = 0; k < d_in; ++k) p.a[j * d_in + k] = (float)(s * (double)w[k]);
    p.c[j] = (float)(beta - s * wm);
    p.r[j] = r;
    p.m_z[j] = mean;
    p.v[j] = var;
    if (p.running_mean) {
      const double f = p.tracked ? 1.0 / (double)*p.tracked : p.factor;
      const double unbiased = var * ((double)p.m / (double)(p.m - 1));
      p.running_mean[j] = (float)((1.0 - f) * (double)p.running_mean[j] + f * mean);
      p.running_var[j] = (float)((1.0 - f) * (double)p.running_var[j] + f * unbiased);
    }
  } else {
    const double s = gamma / sqrt((double)p.running_var[j] + p.eps);
    for (int k = 0; k < d_in; ++k) p.a[j * d_in + k] = (float)(s * (double)w[k]);
    p.c[j] = (float)(beta + s * ((double)p.b1[j] - (double)p.running_mean[j]));
  }
}

inline bool aligned_to(const void *p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }
inline bool sizes_ok(int d_in) { return d_in >= 1 && d_in <= kD; }

}  // namespace bn
}  // namespace rl8

using namespace rl8;

RL8_API int rl8_tower_limits(int *limits) {
  if (!limits) return RL8_ENULL;
  limits[0] = bn::kGridCap;  // moments: workgroups at most
  limits[1] = bn::kRows;     // moments: rows per workgroup and step
  limits[2] = 2 * kCUs;      // narrow towers of width 64: workgroups at most
  limits[3] = kCUs;          // narrow towers of width 128
  limits[4] = 64;            // narrow towers: rows per workgroup and step
  return RL8_OK;
}

RL8_API int64_t rl8_tower_moments_workspace_bytes(int64_t m, int d_in) {
  if (m < 1 || !bn::sizes_ok(d_in)) return RL8_ESIZE;
  return (int64_t)bn::moments_grid(m) * bn::kSlab * (int64_t)sizeof(double);
}

RL8_API int rl8_tower_moments_f64(const float *x, int64_t m, int d_in, double *mu, double *cov, double *workspace,
                                  void *stream) {
  if (!x || !mu || !cov || !workspace) return RL8_ENULL;
  if (m < 1 || !bn::sizes_ok(d_in)) return RL8_ESIZE;
  if (!bn::aligned_to(x, 4) || !bn::aligned_to(mu, 8) || !bn::aligned_to(cov, 8) || !bn::aligned_to(workspace, 8))
    return RL8_EALIGN;
  const int grid = bn::moments_grid(m);
  bn::tower_moments_kernel<<<grid, kBlock, 0, (hipStream_t)stream>>>(x, m, d_in, workspace);
  bn::tower_moments_reduce_kernel<<<1, kBlock, 0, (hipStream_t)stream>>>(workspace, grid, x, m, d_in, mu, cov);
  return launch_status();
}

RL8_API int rl8_batchnorm_fold_f32(const double *mu, const double *cov, int64_t m, int d_in, int hidden, const float *w1,
                                   const float *b1, const float *gamma, const float *beta, double eps,
                                   float *running_mean, float *running_var, double factor, const int64_t *tracked,
                                   int training, float *a, float *c, double *r, double *m_z, double *v, void *stream) {
  if (!w1 || !b1 || !gamma || !beta || !a || !c) return RL8_ENULL;
  if (training ? (!mu || !cov || !r || !m_z || !v || !running_mean != !running_var) : (!running_mean || !running_var))
    return RL8_ENULL;
  if (!bn::sizes_ok(d_in) || (hidden != 64 && hidden != 128) || (training ? m < 2 : m < 0)) return RL8_ESIZE;
  for (const void *p : {(const void *)w1, (const void *)b1, (const void *)gamma, (const void *)beta, (const void *)a,
                        (const void *)c, (const void *)running_mean, (const void *)running_var})
    if (!bn::aligned_to(p, 4)) return RL8_EALIGN;
  for (const void *p : {(const void *)mu, (const void *)cov, (const void *)r, (const void *)m_z, (const void *)v,
                        (const void *)tracked})
    if (!bn::aligned_to(p, 8)) return RL8_EALIGN;
  const bn::FoldArgs args{mu, cov, m, d_in, hidden, w1, b1, gamma, beta, eps, running_mean, running_var, factor,
                          tracked, a, c, r, m_z, v};
  if (training)
    bn::batchnorm_fold_kernel<true><<<1, bn::kFoldThreads, 0, (hipStream_t)stream>>>(args);
  else
    bn::batchnorm_fold_kernel<false><<<1, bn::kFoldThreads, 0, (hipStream_t)stream>>>(args);
  return launch_status();
}
