// Narrow towers behind wide inputs and wide heads: Linear(d_in, H) ReLU Linear(H, H) ReLU Linear(H, n_out) with
// H = 64 or 128, 1 <= d_in <= 128, 1 <= n_out <= 128 and d_in > 16 or n_out > 8 (inside 16 x 8 the towers stay on
// mlp_narrow_kernels.hip, whose VALU layer 1 and VALU head stop there).  fp32 throughout; all five products and their
// gradients run on v_mfma_f32_32x32x2_f32 as exact k-ordered fp32 fma chains.
//
// Weights never enter LDS.  At H = 128, d_in = n_out = 128 the three matrices are 64 KiB each and do not fit a CU's
// LDS beside the activation tiles, so a pack kernel lays every matrix a call needs out in the order the MFMA B operand
// wants it ("fragment order": [k-group of 8][32-column tile][lane][4 k-steps], zeros past the real size), and the
// products read one 16-byte fragment per lane per four k-steps straight from that pack, one k-group ahead of the
// MFMAs that use it.  The packs are <= 64 KiB each and shared by every workgroup, so they live in L2.  LDS holds
// activations only:
//   forward : x [64][KP + 4] | h1 [64][H + 4] | h2 [64][H + 4]
//   backward: x [64][KP + 4] | dout [64][NP + 4] | h1 -> dz1 [64][H + 4] | h2 -> dz2 [64][H + 4]
// KP / NP = d_in / n_out rounded up to the compiled class 32, 64 or 128 (the tiles of the products whose N side is
// d_in or n_out); the k-loops over d_in / n_out run ceil(. / 8) groups, whatever the class.
//
// Forward: a workgroup (4 waves) walks 64-row tiles and stores `out` only.  Backward: ONE kernel.  Per tile it
// recomputes h1 / h2 with the forward's code (hence its bits), then
//   dW3 += dout^T h2,  dz2 = (dout W3) . [h2 > 0] (in place over h2),  dW2 += dz2^T h1,
//   dz1 = (dz2 W2) . [h1 > 0] (in place over h1),  dW1 += dz1^T x,  and, when asked, dx = dz1 W1.
// The weight gradients stay in MFMA accumulators across the workgroup's tiles (k runs over the rows): 16 floats per
// lane per 32 x 32 tile, at most 3 x 64 at H = 128 with both sides at 128, where one workgroup per CU has 512
// registers per lane.  The bias gradients are column sums of dout / dz2 / dz1 in fp64.  Each workgroup writes one
// slab [dW1 | db1 | dW2 | db2 | dW3 | db3 | db3 low parts] and mlp_narrow_wide_reduce_kernel adds the slabs in slab
// order in fp64.  The grid is a function of m and the class alone: no atomics, bitwise reproducible.
//
// MFMA operand maps: mlp_narrow.hip.h.
#include "mfma_tile.hip.h"

namespace rl8 {
namespace narrow_wide {

constexpr int kRows = 64;
constexpr int kThreads = 256;
constexpr int kMaxSide = 128;

inline int tiles32(int n) { return n <= 32 ? 1 : n <= 64 ? 2 : 4; }  // the compiled class of d_in / n_out, in 32-column tiles
inline int groups8(int n) { return (n + 7) / 8; }

// How the 2 x NTN output tiles of a [64][32 NTN] product are split over the four waves.
template <int NTN>
struct Split {
  static_assert(NTN == 1 || NTN == 2 || NTN == 4, "column tiles: 1, 2 or 4");
  static constexpr int kMT = NTN == 4 ? 2 : 1;  // 32-row tiles per wave
  __device__ static int nt(int w) { return NTN == 4 ? w : NTN == 2 ? (w & 1) : 0; }
  __device__ static int mt0(int w) { return NTN == 4 ? 0 : NTN == 2 ? (w >> 1) : w; }
  __device__ static bool active(int w) { return NTN > 1 || w < 2; }
};

__device__ __forceinline__ int acc_row(int v, int hh) { return (v & 3) + 8 * (v >> 2) + 4 * hh; }

// acc[m] (rows 32 (mt0 + m) .., columns 32 nt ..) = init + A B: A [64][ls] in LDS (k along the row), B a fragment pack
// of NTN column tiles, k over kg groups of 8 in k order.  Only for waves with Split<NTN>::active.
template <int NTN>
__device__ __forceinline__ void product(const float *as, int ls, const float *__restrict__ pack, int kg, int wave,
                                        int lane, float init, f32x16 (&acc)[Split<NTN>::kMT]) {
  using S = Split<NTN>;
  const int l32 = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int m = 0; m < S::kMT; ++m)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[m][v] = init;
  const f32x4 *bp = reinterpret_cast<const f32x4 *>(pack) + S::nt(wave) * 64 + lane;
  const float *ap = as + (32 * S::mt0(wave) + l32) * ls + 4 * hh;
  f32x4 b = bp[0];
#pragma unroll 2
  for (int g = 0; g < kg; ++g) {
    const f32x4 bn = bp[(g + 1 < kg ? g + 1 : g) * (NTN * 64)];  // the next group's fragment, in flight under the MFMAs
    f32x4 a[S::kMT];
#pragma unroll
    for (int m = 0; m < S::kMT; ++m) a[m] = *reinterpret_cast<const f32x4 *>(ap + 32 * m * ls + 8 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int m = 0; m < S::kMT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][e], b[e], acc[m], 0, 0, 0);
    b = bn;
  }
}

// The product with its bias (zero past ncols) and an epilogue f(row of the tile, column, value) per element.
template <int NTN, class F>
__device__ __forceinline__ void tile_product(const float *as, int ls, const float *__restrict__ pack, int kg,
                                             const float *__restrict__ bias, int ncols, int wave, int lane, F &&f) {
  using S = Split<NTN>;
  if (!S::active(wave)) return;
  const int col = 32 * S::nt(wave) + (lane & 31), hh = lane >> 5;
  f32x16 acc[S::kMT];
  product<NTN>(as, ls, pack, kg, wave, lane, (bias && col < ncols) ? bias[col] : 0.0f, acc);
#pragma unroll
  for (int m = 0; m < S::kMT; ++m)
#pragma unroll
    for (int v = 0; v < 16; ++v) f(32 * (S::mt0(wave) + m) + acc_row(v, hh), col, acc[m][v]);
}

// dW [32 NI][32 NJ] += A^T B over the tile's 64 rows (k = row): A [64][las], B [64][lbs] in LDS.  Wave w owns tiles
// w TW .. w TW + TW - 1 of the NI x NJ, tile t = (t / NJ, t % NJ).
template <int NI, int NJ>
struct WSplit {
  static constexpr int kTiles = NI * NJ, TW = (kTiles + 3) / 4;
  static_assert(kTiles == 2 || kTiles % 4 == 0, "weight-gradient tiles: 2, or a multiple of the four waves");
};
template <int NI, int NJ>
__device__ __forceinline__ void wgrad(const float *as, int las, const float *bs, int lbs, int wave, int lane,
                                      f32x16 (&acc)[WSplit<NI, NJ>::TW]) {
  using W = WSplit<NI, NJ>;
  if (wave * W::TW >= W::kTiles) return;
  const int l32 = lane & 31, hh = lane >> 5;
#pragma unroll 1
  for (int g = 0; g < kRows / 8; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 8 * g + 4 * hh + e;
#pragma unroll
      for (int u = 0; u < W::TW; ++u) {
        const int t = wave * W::TW + u;
        acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(as[r * las + 32 * (t / NJ) + l32], bs[r * lbs + 32 * (t % NJ) + l32],
                                                      acc[u], 0, 0, 0);
      }
    }
}
template <int NI, int NJ>
__device__ __forceinline__ void store_wgrad(const f32x16 (&acc)[WSplit<NI, NJ>::TW], int wave, int lane,
                                            float *__restrict__ dst, int ld, int rows, int cols) {
  using W = WSplit<NI, NJ>;
  if (wave * W::TW >= W::kTiles) return;
  const int l32 = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int u = 0; u < W::TW; ++u) {
    const int t = wave * W::TW + u, j = 32 * (t % NJ) + l32;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int i = 32 * (t / NJ) + acc_row(v, hh);
      if (i < rows && j < cols) dst[i * ld + j] = acc[u][v];
    }
  }
}

// One [64][W] tile of a row-major [m][width] array into LDS (row stride W + 4), zeros past m / width.
template <int W>
__device__ __forceinline__ void fill_tile(const float *__restrict__ src, int64_t m, int width, int64_t tile, int tid,
                                          float *dst) {
#pragma unroll 8
  for (int e = tid; e < kRows * W; e += kThreads) {
    const int r = e / W, c = e % W;
    const int64_t row = tile * kRows + r;
    dst[r * (W + 4) + c] = (c < width && row < m) ? src[row * width + c] : 0.0f;
  }
}

template <int H, int NTI, int NTO>
struct Geo {
  static_assert(H == 64 || H == 128, "narrow towers: H = 64 or 128");
  static constexpr int NT = H / 32, LS = H + 4, XS = 32 * NTI + 4, DS = 32 * NTO + 4;
  static constexpr size_t kForwardLds = (size_t)kRows * (XS + 2 * LS) * sizeof(float);
  static constexpr size_t kBackwardLds = (size_t)kRows * (XS + DS + 2 * LS) * sizeof(float);
  static constexpr int kForwardPerCU = 2 * kForwardLds <= 160 * 1024 ? 2 : 1;
  // (weight-gradient accumulators per lane, across the tiles: two workgroups per CU leave a lane 256 registers)
  static constexpr int kWgradRegs = 16 * (WSplit<NT, NTI>::TW + WSplit<NT, NT>::TW + WSplit<NTO, NT>::TW);
  static constexpr int kBackwardPerCU = (2 * kBackwardLds <= 160 * 1024 && kWgradRegs <= 48) ? 2 : 1;
  static_assert(kBackwardLds <= 160 * 1024, "LDS");
};

inline int grad_floats(int h, int d_in, int n_out) { return h * d_in + h + h * h + h + n_out * h + n_out; }
inline int slab_floats(int h, int d_in, int n_out) { return grad_floats(h, d_in, n_out) + n_out; }  // + db3's low parts

// The packs of one call, in workspace order (floats; each a multiple of 256).
struct Packs {
  int f1, f2, f3, g3, g2, g1, end;  // forward: f1 f2 f3; backward: f1 f2 g3 g2 g1
};
inline Packs pack_offsets(int h, int d_in, int n_out, bool backward) {
  const int nt = h / 32, hg = h / 8;
  Packs p{};
  int at = 0;
  const auto take = [&at](int kg, int ntn) {
    const int o = at;
    at += kg * ntn * 256;
    return o;
  };
  p.f1 = take(groups8(d_in), nt);
  p.f2 = take(hg, nt);
  if (backward) {
    p.g3 = take(groups8(n_out), nt);
    p.g2 = take(hg, nt);
    p.g1 = take(hg, tiles32(d_in));
  } else {
    p.f3 = take(hg, tiles32(n_out));
  }
  p.end = at;
  return p;
}

// dst[offset ..] = B in fragment order, B[k][j] = src[k sk + j sj] for k < K, j < N and zero elsewhere:
// element ((g ntn + nt) 64 + lane) 4 + e holds k = 8 g + 4 (lane >> 5) + e, j = 32 nt + (lane & 31).
struct PackJob {
  const float *src;
  int k, n, sk, sj, kg, ntn, offset;
};
struct PackJobs {
  PackJob job[5];
};
__global__ __launch_bounds__(kThreads) void mlp_narrow_wide_pack_kernel(PackJobs jobs, float *__restrict__ dst) {
  const PackJob j = jobs.job[blockIdx.y];
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= j.kg * j.ntn * 256) return;
  const int e = idx & 3, lane = (idx >> 2) & 63, t = idx >> 8;
  const int k = 8 * (t / j.ntn) + 4 * (lane >> 5) + e, col = 32 * (t % j.ntn) + (lane & 31);
  dst[j.offset + idx] = (k < j.k && col < j.n) ? j.src[(int64_t)k * j.sk + (int64_t)col * j.sj] : 0.0f;
}

template <int H, int NTI, int NTO>
__global__ __launch_bounds__(kThreads, (Geo<H, NTI, NTO>::kForwardPerCU)) void mlp_narrow_wide_forward_kernel(
    const float *__restrict__ x, int64_t m, int d_in, const float *__restrict__ f1, const float *__restrict__ b1,
    const float *__restrict__ f2, const float *__restrict__ b2, const float *__restrict__ f3,
    const float *__restrict__ b3, int n_out, float *__restrict__ out) {
  using G = Geo<H, NTI, NTO>;
  constexpr int LS = G::LS, XS = G::XS;
  extern __shared__ float lds[];
  float *xs = lds, *h1s = xs + kRows * XS, *h2s = h1s + kRows * LS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kg1 = (d_in + 7) / 8;
  const int64_t tiles = (m + kRows - 1) / kRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's readers of xs / h1s / h2s are done
    fill_tile<32 * NTI>(x, m, d_in, tile, tid, xs);
    __syncthreads();
    tile_product<G::NT>(xs, XS, f1, kg1, b1, H, wave, lane,
                        [&](int r, int c, float z) { h1s[r * LS + c] = z > 0.0f ? z : 0.0f; });
    __syncthreads();
    tile_product<G::NT>(h1s, LS, f2, H / 8, b2, H, wave, lane,
                        [&](int r, int c, float z) { h2s[r * LS + c] = z > 0.0f ? z : 0.0f; });
    __syncthreads();
    tile_product<NTO>(h2s, LS, f3, H / 8, b3, n_out, wave, lane, [&](int r, int c, float z) {
      const int64_t row = tile * kRows + r;
      if (row < m && c < n_out) out[row * n_out + c] = z;
    });
  }
}

template <int H, int NTI, int NTO>
__global__ __launch_bounds__(kThreads, (Geo<H, NTI, NTO>::kBackwardPerCU)) void mlp_narrow_wide_backward_kernel(
    const float *__restrict__ x, const float *__restrict__ dout, int64_t m, int d_in, const float *__restrict__ f1,
    const float *__restrict__ b1, const float *__restrict__ f2, const float *__restrict__ b2,
    const float *__restrict__ g3, const float *__restrict__ g2, const float *__restrict__ g1, int n_out,
    float *__restrict__ slabs, float *__restrict__ dx) {
  using G = Geo<H, NTI, NTO>;
  using S = Split<G::NT>;
  constexpr int LS = G::LS, XS = G::XS, DS = G::DS, NT = G::NT;
  static_assert(NT >= 2, "every wave owns a tile of the [64][H] products");
  extern __shared__ float lds[];
  float *xs = lds, *ds = xs + kRows * XS, *h1s = ds + kRows * DS, *h2s = h1s + kRows * LS;
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = 32 * S::nt(wave) + (lane & 31);  // this lane's column of the [64][H] products
  const int kg1 = (d_in + 7) / 8, kg3 = (n_out + 7) / 8;

  f32x16 w1acc[WSplit<NT, NTI>::TW], w2acc[WSplit<NT, NT>::TW], w3acc[WSplit<NTO, NT>::TW];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
#pragma unroll
    for (int u = 0; u < WSplit<NT, NTI>::TW; ++u) w1acc[u][v] = 0.0f;
#pragma unroll
    for (int u = 0; u < WSplit<NT, NT>::TW; ++u) w2acc[u][v] = 0.0f;
#pragma unroll
    for (int u = 0; u < WSplit<NTO, NT>::TW; ++u) w3acc[u][v] = 0.0f;
  }
  double db1 = 0.0, db2 = 0.0, db3 = 0.0;  // thread tid: column tid of dz1 / dz2 / dout

  const int64_t tiles = (m + kRows - 1) / kRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's readers of xs / ds / h1s are done
    fill_tile<32 * NTI>(x, m, d_in, tile, tid, xs);
    fill_tile<32 * NTO>(dout, m, n_out, tile, tid, ds);
    __syncthreads();
    tile_product<NT>(xs, XS, f1, kg1, b1, H, wave, lane,
                     [&](int r, int c, float z) { h1s[r * LS + c] = z > 0.0f ? z : 0.0f; });
    if (tid < n_out)
#pragma unroll 8
      for (int r = 0; r < kRows; ++r) db3 += (double)ds[r * DS + tid];
    __syncthreads();
    tile_product<NT>(h1s, LS, f2, H / 8, b2, H, wave, lane,
                     [&](int r, int c, float z) { h2s[r * LS + c] = z > 0.0f ? z : 0.0f; });
    __syncthreads();
    wgrad<NTO, NT>(ds, DS, h2s, LS, wave, lane, w3acc);  // dW3[q][j] += sum_r dout[r][q] h2[r][j]
    {
      f32x16 acc[S::kMT];
      product<NT>(ds, DS, g3, kg3, wave, lane, 0.0f, acc);  // dh2 = dout W3
      __syncthreads();                                       // every wave has read h2 for dW3: the tile takes dz2
#pragma unroll
      for (int mm = 0; mm < S::kMT; ++mm)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          float *p = h2s + (32 * (S::mt0(wave) + mm) + acc_row(v, hh)) * LS + col;
          *p = *p > 0.0f ? acc[mm][v] : 0.0f;
        }
    }
    __syncthreads();
    wgrad<NT, NT>(h2s, LS, h1s, LS, wave, lane, w2acc);  // dW2[j][i] += sum_r dz2[r][j] h1[r][i]
    if (tid < H)
#pragma unroll 8
      for (int r = 0; r < kRows; ++r) db2 += (double)h2s[r * LS + tid];
    {
      f32x16 acc[S::kMT];
      product<NT>(h2s, LS, g2, H / 8, wave, lane, 0.0f, acc);  // dh1 = dz2 W2
      __syncthreads();                                          // every wave has read h1 for dW2: the tile takes dz1
#pragma unroll
      for (int mm = 0; mm < S::kMT; ++mm)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          float *p = h1s + (32 * (S::mt0(wave) + mm) + acc_row(v, hh)) * LS + col;
          *p = *p > 0.0f ? acc[mm][v] : 0.0f;
        }
    }
    __syncthreads();
    wgrad<NT, NTI>(h1s, LS, xs, XS, wave, lane, w1acc);  // dW1[j][c] += sum_r dz1[r][j] x[r][c]
    if (tid < H)
#pragma unroll 8
      for (int r = 0; r < kRows; ++r) db1 += (double)h1s[r * LS + tid];
    if (dx)
      tile_product<NTI>(h1s, LS, g1, H / 8, nullptr, 0, wave, lane, [&](int r, int c, float g) {
        const int64_t row = tile * kRows + r;
        if (row < m && c < d_in) dx[row * d_in + c] = g;
      });
  }

  // This workgroup's slab, in the gradient layout [dW1 | db1 | dW2 | db2 | dW3 | db3 | db3 low parts].
  const int o_b1 = H * d_in, o_w2 = o_b1 + H, o_b2 = o_w2 + H * H, o_w3 = o_b2 + H, o_b3 = o_w3 + n_out * H;
  float *slab = slabs + (int64_t)blockIdx.x * (o_b3 + 2 * n_out);
  store_wgrad<NT, NTI>(w1acc, wave, lane, slab, d_in, H, d_in);
  store_wgrad<NT, NT>(w2acc, wave, lane, slab + o_w2, H, H, H);
  store_wgrad<NTO, NT>(w3acc, wave, lane, slab + o_w3, H, n_out, H);
  if (tid < H) {
    slab[o_b1 + tid] = (float)db1;
    slab[o_b2 + tid] = (float)db2;
  }
  if (tid < n_out) {
    const float hi = (float)db3;
    slab[o_b3 + tid] = hi;
    slab[o_b3 + n_out + tid] = (float)(db3 - (double)hi);
  }
}

// grads[e] = sum over the slabs, in slab order, in fp64 (db3: high and low parts).
__global__ __launch_bounds__(kThreads) void mlp_narrow_wide_reduce_kernel(const float *__restrict__ slabs,
                                                                          int slab_count, int floats, int n_out,
                                                                          float *__restrict__ grads) {
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

inline int grid_for(int64_t m, int per_cu) {
  const int64_t tiles = (m + kRows - 1) / kRows, cap = (int64_t)kCUs * per_cu;
  return (int)(tiles < cap ? tiles : cap);
}

inline int launch_pack(hipStream_t s, const PackJobs &jobs, int count, float *dst) {
  int most = 0;
  for (int i = 0; i < count; ++i) most = jobs.job[i].kg * jobs.job[i].ntn > most ? jobs.job[i].kg * jobs.job[i].ntn : most;
  mlp_narrow_wide_pack_kernel<<<dim3(most, count), kThreads, 0, s>>>(jobs, dst);
  return launch_status();
}

struct ForwardArgs {
  hipStream_t s;
  const float *x;
  int64_t m;
  int d_in;
  const float *b1, *b2, *b3;
  int n_out;
  float *packs, *out;
  Packs at;
};
template <int H, int NTI, int NTO>
int launch_forward(const ForwardArgs &a) {
  using G = Geo<H, NTI, NTO>;
  constexpr auto *kernel = &mlp_narrow_wide_forward_kernel<H, NTI, NTO>;
  if (const int e = allow_dynamic_lds<kernel>((int)G::kForwardLds)) return e;
  kernel<<<grid_for(a.m, G::kForwardPerCU), kThreads, G::kForwardLds, a.s>>>(
      a.x, a.m, a.d_in, a.packs + a.at.f1, a.b1, a.packs + a.at.f2, a.b2, a.packs + a.at.f3, a.b3, a.n_out, a.out);
  return launch_status();
}

struct BackwardArgs {
  hipStream_t s;
  const float *x, *dout;
  int64_t m;
  int d_in;
  const float *b1, *b2;
  int n_out;
  float *packs, *slabs, *dx;
  Packs at;
};
template <int H, int NTI, int NTO>
int launch_backward(const BackwardArgs &a) {
  using G = Geo<H, NTI, NTO>;
  constexpr auto *kernel = &mlp_narrow_wide_backward_kernel<H, NTI, NTO>;
  if (const int e = allow_dynamic_lds<kernel>((int)G::kBackwardLds)) return e;
  kernel<<<grid_for(a.m, G::kBackwardPerCU), kThreads, G::kBackwardLds, a.s>>>(
      a.x, a.dout, a.m, a.d_in, a.packs + a.at.f1, a.b1, a.packs + a.at.f2, a.b2, a.packs + a.at.g3,
      a.packs + a.at.g2, a.packs + a.at.g1, a.n_out, a.slabs, a.dx);
  return launch_status();
}

template <int H, int NTI, int NTO>
struct Forward {
  static int run(const ForwardArgs &a) { return launch_forward<H, NTI, NTO>(a); }
  static int per_cu() { return Geo<H, NTI, NTO>::kForwardPerCU; }
  static int lds() { return (int)Geo<H, NTI, NTO>::kForwardLds; }
};
template <int H, int NTI, int NTO>
struct Backward {
  static int run(const BackwardArgs &a) { return launch_backward<H, NTI, NTO>(a); }
  static int per_cu() { return Geo<H, NTI, NTO>::kBackwardPerCU; }
  static int lds() { return (int)Geo<H, NTI, NTO>::kBackwardLds; }
};

// Calls f(L<H, NTI, NTO>{}) for the compiled class of (hidden, d_in, n_out).
template <template <int, int, int> class L, class F>
int dispatch(int hidden, int d_in, int n_out, F &&f) {
  const int ti = tiles32(d_in), to = tiles32(n_out);
#define RL8_NW_OUT(H, TI)                 \
  if (to == 1) return f(L<H, TI, 1>{});   \
  if (to == 2) return f(L<H, TI, 2>{});   \
  return f(L<H, TI, 4>{});
#define RL8_NW_IN(H)              \
  if (hidden == H) {              \
    if (ti == 1) { RL8_NW_OUT(H, 1) } \
    if (ti == 2) { RL8_NW_OUT(H, 2) } \
    RL8_NW_OUT(H, 4)              \
  }
  RL8_NW_IN(64)
  RL8_NW_IN(128)
#undef RL8_NW_IN
#undef RL8_NW_OUT
  return RL8_ESIZE;
}

inline int backward_grid(int64_t m, int hidden, int d_in, int n_out) {
  return dispatch<Backward>(hidden, d_in, n_out, [m](auto l) { return grid_for(m, decltype(l)::per_cu()); });
}

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace narrow_wide
}  // namespace rl8

using namespace rl8;
namespace nw = rl8::narrow_wide;

RL8_API int rl8_mlp_narrow_wide_supports(int hidden, int d_in, int n_out) {
  return (hidden == 64 || hidden == 128) && d_in >= 1 && d_in <= nw::kMaxSide && n_out >= 1 && n_out <= nw::kMaxSide &&
         (d_in > kMaxIn || n_out > kMaxOut);
}

RL8_API int rl8_mlp_narrow_wide_limits(int backward, int hidden, int d_in, int n_out, int *limits) {
  if (!limits) return RL8_ENULL;
  if (!rl8_mlp_narrow_wide_supports(hidden, d_in, n_out)) return RL8_ESIZE;
  if (backward != 0 && backward != 1) return RL8_ECONFIG;
  const auto fill = [limits](auto l) {
    limits[0] = decltype(l)::lds();
    limits[1] = decltype(l)::per_cu();
    return RL8_OK;
  };
  return backward ? nw::dispatch<nw::Backward>(hidden, d_in, n_out, fill) : nw::dispatch<nw::Forward>(hidden, d_in, n_out, fill);
}

RL8_API int64_t rl8_mlp_narrow_wide_workspace_bytes(int64_t m, int hidden, int d_in, int n_out, int backward) {
  if (m < 1 || !rl8_mlp_narrow_wide_supports(hidden, d_in, n_out)) return RL8_ESIZE;
  if (backward != 0 && backward != 1) return RL8_ECONFIG;
  int64_t floats = nw::pack_offsets(hidden, d_in, n_out, backward != 0).end;
  if (backward) floats += (int64_t)nw::backward_grid(m, hidden, d_in, n_out) * nw::slab_floats(hidden, d_in, n_out);
  return floats * (int64_t)sizeof(float);
}

RL8_API int rl8_mlp_narrow_wide_forward_f32(const float *x, int64_t m, int d_in, const float *w1, const float *b1,
                                            const float *w2, const float *b2, const float *w3, const float *b3,
                                            int n_out, int hidden, float *workspace, float *out, void *stream) {
  if (!x || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !workspace || !out) return RL8_ENULL;
  if (m < 1 || !rl8_mlp_narrow_wide_supports(hidden, d_in, n_out)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)w1, (const void *)b1, (const void *)w2, (const void *)b2,
                        (const void *)w3, (const void *)b3, (const void *)out})
    if (!nw::aligned4(p)) return RL8_EALIGN;
  if (!aligned16(workspace)) return RL8_EALIGN;
  const nw::Packs at = nw::pack_offsets(hidden, d_in, n_out, false);
  const int nt = hidden / 32, hg = hidden / 8;
  nw::PackJobs jobs{};
  jobs.job[0] = {w1, d_in, hidden, 1, d_in, nw::groups8(d_in), nt, at.f1};        // B[k][j] = W1[j][k]
  jobs.job[1] = {w2, hidden, hidden, 1, hidden, hg, nt, at.f2};                    // B[k][j] = W2[j][k]
  jobs.job[2] = {w3, hidden, n_out, 1, hidden, hg, nw::tiles32(n_out), at.f3};     // B[k][q] = W3[q][k]
  if (const int e = nw::launch_pack((hipStream_t)stream, jobs, 3, workspace)) return e;
  const nw::ForwardArgs a{(hipStream_t)stream, x, m, d_in, b1, b2, b3, n_out, workspace, out, at};
  return nw::dispatch<nw::Forward>(hidden, d_in, n_out, [&a](auto l) { return decltype(l)::run(a); });
}

RL8_API int rl8_mlp_narrow_wide_backward_f32(const float *x, const float *dout, int64_t m, int d_in, const float *w1,
                                             const float *b1, const float *w2, const float *b2, const float *w3,
                                             int n_out, int hidden, float *workspace, float *dx, void *stream) {
  if (!x || !dout || !w1 || !b1 || !w2 || !b2 || !w3 || !workspace) return RL8_ENULL;
  if (m < 1 || !rl8_mlp_narrow_wide_supports(hidden, d_in, n_out)) return RL8_ESIZE;
  for (const void *p : {(const void *)x, (const void *)dout, (const void *)w1, (const void *)b1, (const void *)w2,
                        (const void *)b2, (const void *)w3, (const void *)dx})
    if (!nw::aligned4(p)) return RL8_EALIGN;
  if (!aligned16(workspace)) return RL8_EALIGN;
  const nw::Packs at = nw::pack_offsets(hidden, d_in, n_out, true);
  const int nt = hidden / 32, hg = hidden / 8;
  nw::PackJobs jobs{};
  jobs.job[0] = {w1, d_in, hidden, 1, d_in, nw::groups8(d_in), nt, at.f1};
  jobs.job[1] = {w2, hidden, hidden, 1, hidden, hg, nt, at.f2};
  jobs.job[2] = {w3, n_out, hidden, hidden, 1, nw::groups8(n_out), nt, at.g3};   // B[q][j] = W3[q][j]
  jobs.job[3] = {w2, hidden, hidden, hidden, 1, hg, nt, at.g2};                   // B[j][i] = W2[j][i]
  jobs.job[4] = {w1, hidden, d_in, d_in, 1, hg, nw::tiles32(d_in), at.g1};        // B[j][c] = W1[j][c]
  if (const int e = nw::launch_pack((hipStream_t)stream, jobs, dx ? 5 : 4, workspace)) return e;
  const nw::BackwardArgs a{(hipStream_t)stream, x, dout, m, d_in, b1, b2, n_out, workspace, workspace + at.end, dx, at};
  return nw::dispatch<nw::Backward>(hidden, d_in, n_out, [&a](auto l) { return decltype(l)::run(a); });
}

RL8_API int rl8_mlp_narrow_wide_reduce_f32(const float *workspace, int64_t m, int hidden, int d_in, int n_out,
                                           float *grads_out, void *stream) {
  if (!workspace || !grads_out) return RL8_ENULL;
  if (m < 1 || !rl8_mlp_narrow_wide_supports(hidden, d_in, n_out)) return RL8_ESIZE;
  if (!aligned16(workspace) || !nw::aligned4(grads_out)) return RL8_EALIGN;
  const int floats = nw::grad_floats(hidden, d_in, n_out);
  nw::mlp_narrow_wide_reduce_kernel<<<(floats + nw::kThreads - 1) / nw::kThreads, nw::kThreads, 0, (hipStream_t)stream>>>(
      workspace + nw::pack_offsets(hidden, d_in, n_out, true).end, nw::backward_grid(m, hidden, d_in, n_out), floats,
      n_out, grads_out);
  return launch_status();
}
