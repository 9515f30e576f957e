// K6 rollout statistics, K5 minibatch gather, and the ABI housekeeping calls.
//
// K6 restates src/rl8/algorithms/_feedforward.py:411-436: per-env returns
// (sum over the horizon), min / max / mean / unbiased std of returns and of
// rewards, and std of the reversed discounted returns -- eight eager reductions
// and nine host syncs in the reference, one pass over 8 B per transition here.
// Raw fp64 moments are emitted (not means) so that env shards on several GPUs
// combine with plain SUM / MIN / MAX all-reduces.
//
// K5 restates src/rl8/_utils.py:211-225 (Batcher): index-gather of every buffer
// leaf for one minibatch, all leaves in one launch.
#include "common.hip.h"

namespace rl8 {

// partial columns: 0 sum(ret) 1 sum(ret^2) 2 min(ret) 3 max(ret)
//                  4 sum(r)   5 sum(r^2)   6 min(r)   7 max(r)
//                  8 sum(rdr) 9 sum(rdr^2)

// VEC == 4: time-major leaves (env_stride == 1): one lane walks 4 adjacent envs
// with 16-byte loads per column.  VEC == 1: any strides, one env per lane.
constexpr int kStatsBatch = 8;  // time steps whose loads are issued together

// min / max that keep a NaN, as torch.min / torch.max do (fminf, fmaxf and a bare `<` drop it): a NaN on either side
// comes out, infinities are ordinary extrema.  Every fold below -- lane, wave, block, last block -- goes through these,
// except the per-reward one of a lane, which keeps fminf / fmaxf and tracks a NaN beside them.
template <class T>
__device__ __forceinline__ T nan_min(T a, T b) { return (a < b || a != a) ? a : b; }
template <class T>
__device__ __forceinline__ T nan_max(T a, T b) { return (a > b || a != a) ? a : b; }
struct NanMinOp {
  __device__ __forceinline__ static double apply(double a, double b) { return nan_min(a, b); }
};
struct NanMaxOp {
  __device__ __forceinline__ static double apply(double a, double b) { return nan_max(a, b); }
};

template <int VEC, bool RDR>
__global__ __launch_bounds__(kBlock) void rollout_stats_kernel(
    const float *__restrict__ rewards, const float *__restrict__ rdr, int64_t n, int64_t h,
    int64_t env_stride, int64_t time_stride, double *__restrict__ partials,
    double *__restrict__ out) {
  __shared__ double smem[6 * kWavesPerBlock];
  double sums[6] = {0, 0, 0, 0, 0, 0};  // ret, ret^2, r, r^2, rdr, rdr^2
  double mins[2] = {INFINITY, INFINITY}, maxs[2] = {-INFINITY, -INFINITY};
  const int64_t stride = (int64_t)gridDim.x * kBlock * VEC;
  for (int64_t e = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC; e < n; e += stride) {
    float ret[VEC];  // torch.sum(rewards[:, :-1], dim=1) accumulates in f32
#pragma unroll
    for (int i = 0; i < VEC; ++i) ret[i] = 0.0f;
    float rmin = INFINITY, rmax = -INFINITY;
    // fminf / fmaxf drop a NaN (and fold two rewards per min3 / max3), so one is tracked beside them: the largest
    // (bits << 1) of the rewards, an unsigned max like the float ones, is above 0xff000000 iff one of them is a NaN
    uint32_t nan_key = 0u;
    // The sums are taken in ascending t whatever the batching below: a batch
    // only decides how many loads are in the air before the first add (one
    // load per wait leaves the pass at latency, 2.8 of 8 TB/s on cold rows).
    auto fetch = [&](const float *base, int64_t t, float(&v)[VEC]) {
      if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(base + t * time_stride + e);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        v[0] = base[e * env_stride + t * time_stride];
      }
    };
    auto fold = [&](const float(&r)[VEC], const float(&d)[VEC]) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        ret[i] = ret[i] + r[i];
        sums[2] += (double)r[i];
        sums[3] += (double)r[i] * (double)r[i];
        rmin = fminf(rmin, r[i]);
        rmax = fmaxf(rmax, r[i]);
        nan_key = max(nan_key, __float_as_uint(r[i]) << 1);
      }
      if constexpr (RDR) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          sums[4] += (double)d[i];
          sums[5] += (double)d[i] * (double)d[i];
        }
      }
    };
    int64_t t = 0;
    for (; t + kStatsBatch <= h; t += kStatsBatch) {
      float r[kStatsBatch][VEC], d[kStatsBatch][VEC];
#pragma unroll
      for (int b = 0; b < kStatsBatch; ++b) {
        fetch(rewards, t + b, r[b]);
        if constexpr (RDR) fetch(rdr, t + b + 1, d[b]);
      }
#pragma unroll
      for (int b = 0; b < kStatsBatch; ++b) fold(r[b], d[b]);
    }
    for (; t < h; ++t) {
      float r[VEC], d[VEC];
      fetch(rewards, t, r);
      if constexpr (RDR) fetch(rdr, t + 1, d);
      fold(r, d);
    }
    if (nan_key > 0xff000000u) rmin = rmax = NAN;
    mins[1] = nan_min((double)rmin, mins[1]);
    maxs[1] = nan_max((double)rmax, maxs[1]);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      sums[0] += (double)ret[i];
      sums[1] += (double)ret[i] * (double)ret[i];
      mins[0] = nan_min((double)ret[i], mins[0]);
      maxs[0] = nan_max((double)ret[i], maxs[0]);
    }
  }
  double a4[4] = {sums[0], sums[1], sums[2], sums[3]};
  block_reduce<4, SumOp>(a4, smem);
  double b2[2] = {sums[4], sums[5]};
  block_reduce<2, SumOp>(b2, smem);
  block_reduce<2, NanMinOp>(mins, smem);
  block_reduce<2, NanMaxOp>(maxs, smem);
  if (threadIdx.x == 0) {
    double *row = partials + (int64_t)blockIdx.x * kPartialWidth;
    const double vals[10] = {a4[0], a4[1], mins[0], maxs[0], a4[2], a4[3], mins[1], maxs[1],
                             b2[0], b2[1]};
#pragma unroll
    for (int c = 0; c < 10; ++c) publish_partial(row + c, vals[c]);
  }
  if (!last_block_arrives(ticket_word(partials))) return;
  // Last block: combine every row in order (fixed order => reproducible).
  for (int i = 0; i < 6; ++i) sums[i] = 0.0;
  mins[0] = mins[1] = INFINITY;
  maxs[0] = maxs[1] = -INFINITY;
  const int rows = (int)gridDim.x;
  const double nn = (double)n, nh = (double)n * (double)h;
  fold_partial_rows<10>(partials, rows, [&](const double(&row)[10]) {
    sums[0] += row[0]; sums[1] += row[1]; sums[2] += row[4];
    sums[3] += row[5]; sums[4] += row[8]; sums[5] += row[9];
    mins[0] = nan_min(row[2], mins[0]);
    maxs[0] = nan_max(row[3], maxs[0]);
    mins[1] = nan_min(row[6], mins[1]);
    maxs[1] = nan_max(row[7], maxs[1]);
  });
  block_reduce<6, SumOp>(sums, smem);
  block_reduce<2, NanMinOp>(mins, smem);
  block_reduce<2, NanMaxOp>(maxs, smem);
  if (threadIdx.x == 0) {
    out[0] = nn;  out[1] = sums[0]; out[2] = sums[1]; out[3] = mins[0]; out[4] = maxs[0];
    out[5] = nh;  out[6] = sums[2]; out[7] = sums[3]; out[8] = mins[1]; out[9] = maxs[1];
    out[10] = sums[4]; out[11] = sums[5];
    *ticket_word(partials) = 0u;
  }
}

struct GatherArgs {
  rl8_gather_field f[RL8_MAX_GATHER_FIELDS];
  int n_fields;
};

// One lane per (sample, field-element).  Reads are random 4/8-byte accesses
// (this is a shuffle), writes are dense.
__global__ __launch_bounds__(kBlock) void gather_minibatch_kernel(
    const int64_t *__restrict__ index, int64_t m, int64_t h, GatherArgs args) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) {
    const int64_t s = index ? index[i] : i;  // (index = NULL: every sample in order)
    const int64_t env = s / h, t = s - env * h;
#pragma unroll 1
    for (int f = 0; f < args.n_fields; ++f) {
      const rl8_gather_field &fd = args.f[f];
      const int64_t src0 = env * fd.env_stride + t * fd.time_stride;
      if (fd.elem_bytes == 4) {
        const uint32_t *src = static_cast<const uint32_t *>(fd.src) + src0;
        uint32_t *dst = static_cast<uint32_t *>(fd.dst) + i * fd.row_elems;
        for (int c = 0; c < fd.row_elems; ++c) dst[c] = src[c];
      } else {
        const uint64_t *src = static_cast<const uint64_t *>(fd.src) + src0;
        uint64_t *dst = static_cast<uint64_t *>(fd.dst) + i * fd.row_elems;
        for (int c = 0; c < fd.row_elems; ++c) dst[c] = src[c];
      }
    }
  }
}

// Whole sequences of seq_len samples (the recurrent algorithm's minibatches), leaves of 1-, 4- or 8-byte elements:
// sequence q = env * (h / seq_len) + s is samples q seq_len + j, j < seq_len, and row i seq_len + j of every
// destination receives src[env][s seq_len + j].  One lane per gathered row and field; a row of a byte-wide leaf (the
// bool[3] action mask: 3 bytes, no word alignment) moves byte by byte.
__global__ __launch_bounds__(kBlock) void gather_sequences_kernel(
    const int64_t *__restrict__ seq_index, int64_t rows, int seq_len, int64_t h, GatherArgs args) {
  const int64_t stride = (int64_t)gridDim.x * kBlock, per_env = h / seq_len;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
    const int64_t slot = i / seq_len, j = i - slot * seq_len;
    const int64_t q = seq_index ? seq_index[slot] : slot;  // (seq_index = NULL: every sequence in order)
    const int64_t env = q / per_env, t = (q - env * per_env) * seq_len + j;
#pragma unroll 1
    for (int f = 0; f < args.n_fields; ++f) {
      const rl8_gather_field &fd = args.f[f];
      const int64_t src0 = env * fd.env_stride + t * fd.time_stride;
      if (fd.elem_bytes == 4) {
        const uint32_t *src = static_cast<const uint32_t *>(fd.src) + src0;
        uint32_t *dst = static_cast<uint32_t *>(fd.dst) + i * fd.row_elems;
        for (int c = 0; c < fd.row_elems; ++c) dst[c] = src[c];
      } else if (fd.elem_bytes == 8) {
        const uint64_t *src = static_cast<const uint64_t *>(fd.src) + src0;
        uint64_t *dst = static_cast<uint64_t *>(fd.dst) + i * fd.row_elems;
        for (int c = 0; c < fd.row_elems; ++c) dst[c] = src[c];
      } else {
        const uint8_t *src = static_cast<const uint8_t *>(fd.src) + src0;
        uint8_t *dst = static_cast<uint8_t *>(fd.dst) + i * fd.row_elems;
        for (int c = 0; c < fd.row_elems; ++c) dst[c] = src[c];
      }
    }
  }
}

// Padded rolling windows (src/rl8/views.py:54-123, 240-321): cell j of a window of `size` ending at step t is step
// t' = t - (size - 1) + j of the same env, zeros and mask = 1 where t' < 0.  A field of size 1 is the plain gather (no
// mask), so the unwindowed leaves of a dict observation ride in the same launch.
struct WindowArgs {
  rl8_window_field f[RL8_MAX_GATHER_FIELDS];
  int n_fields;
};

// One window cell: `row_elems` elements to dst[cell], from src + src0 (elements) or zeros.
template <class T>
__device__ __forceinline__ void window_cell(const rl8_window_field &fd, int64_t cell, int64_t src0, bool padded) {
  T *dst = static_cast<T *>(fd.dst) + cell * fd.row_elems;
  if (padded) {
    for (int c = 0; c < fd.row_elems; ++c) dst[c] = T(0);
  } else {
    const T *src = static_cast<const T *>(fd.src) + src0;
    for (int c = 0; c < fd.row_elems; ++c) dst[c] = src[c];
  }
}

__device__ __forceinline__ void window_cell(const rl8_window_field &fd, int64_t cell, int64_t env, int64_t t) {
  const bool padded = t < 0;
  const int64_t src0 = env * fd.env_stride + t * fd.time_stride;
  if (fd.elem_bytes == 4) window_cell<uint32_t>(fd, cell, src0, padded);
  else if (fd.elem_bytes == 8) window_cell<uint64_t>(fd, cell, src0, padded);
  else window_cell<uint8_t>(fd, cell, src0, padded);  // (a bool[3] row: 3 bytes, no word alignment)
  if (fd.mask) fd.mask[cell] = padded ? 1 : 0;
}

// Training: one lane per gathered window cell, field after field: a sample's cells sit in neighbouring lanes, so the
// writes of a wave are one dense run and every cell's random read (this is a shuffle) is in flight at once; the index
// is re-read from cache by the lanes of a sample.
__global__ __launch_bounds__(kBlock) void gather_windows_kernel(
    const int64_t *__restrict__ index, int64_t m, int64_t h, WindowArgs args) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
#pragma unroll 1
  for (int f = 0; f < args.n_fields; ++f) {
    const rl8_window_field &fd = args.f[f];
    const int64_t cells = m * fd.size;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < cells; k += stride) {
      const int64_t i = k / fd.size, j = k - i * fd.size;
      const int64_t s = index ? index[i] : i;  // (index = NULL: every sample in order)
      const int64_t env = s / h, t = s - env * h;
      window_cell(fd, k, env, t - (fd.size - 1) + j);
    }
  }
}

// Rollout: the window ending at the given step of every env.  Lanes run over envs within one window cell j, so on a
// time-major slab each of the `size` source columns is read as one contiguous run.
__global__ __launch_bounds__(kBlock) void window_last_kernel(int64_t t, int64_t n, WindowArgs args) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
#pragma unroll 1
  for (int f = 0; f < args.n_fields; ++f) {
    const rl8_window_field &fd = args.f[f];
    const int64_t cells = n * fd.size;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < cells; k += stride) {
      const int64_t j = k / n, env = k - j * n;
      window_cell(fd, env * fd.size + j, env, t - (fd.size - 1) + j);
    }
  }
}

// K5b: packed sample rows.  A shuffled minibatch reads every field of a sample
// from a different random address: five 4/8-byte reads, five 32/64-byte sectors,
// ~12x the algorithmic bytes (PMC).  When a buffer is going to be shuffled
// several times (num_sgd_iters x num_minibatches gathers per step()), the fields
// of every sample are first laid side by side, once, in the reference's sample
// order s = env*H + t; a minibatch then reads ONE 16-byte-aligned row per
// sample.  pack: a tiled transposition through LDS (pack_samples_tiled_kernel).
// gather: each lane reads its own row and writes the dense outputs.
struct PackedArgs {
  rl8_gather_field f[RL8_MAX_GATHER_FIELDS];
  int n_fields;
  int row_words;
};

// pack_samples as a tiled transposition (round 4; VERDICT r3 weak #9: "a pure streaming transposition at 1.9 TB/s").  The
// lane-per-sample kernel it replaced (removed in round 5) read coalesced (lane = env of a time-major slab) and wrote each
// lane's own 32-byte row a kilobyte from its neighbour's.  Here a workgroup owns kPackEnvs environments x up to kPackSteps timesteps: every (field, word,
// timestep) is one 256-byte wave load into an LDS tile (rows padded to an odd number of words: lane = env writes hit 32
// banks), and the tile leaves as whole packed rows in memory order -- Tc x row bytes contiguous per environment, 1 KiB per
// wave store.  Any strides (an env-major buffer reads poorly and still writes well).
constexpr int kPackEnvs = 64, kPackSteps = 32;
constexpr int kMaxPackedVecsDecl = 8;  // (= kMaxPackedVecs below: rows of up to 128 bytes)
// DENSE (round 4; rl8_gather_minibatch with index = NULL): the same tiles leave as the DENSE per-field rows of a gather of
// every sample in order -- dst_f[(env h + t)] -- instead of packed rows: an env's `steps` rows of a field are contiguous.
template <bool DENSE>
__global__ __launch_bounds__(kBlock) void pack_samples_tiled_kernel(int64_t n, int64_t h, uint32_t *__restrict__ packed,
                                                                    PackedArgs args, int tile_steps) {
  extern __shared__ uint32_t tile[];  // [step][env][row_words + 1]
  const int rw = args.row_words, pitch = rw + 1;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  // where word w of a packed row comes from: its field's base (+ the word's offset in the element row) and strides, in
  // words; padding words (behind the last field) have no source and are written as zero
  __shared__ const uint32_t *word_src[4 * kMaxPackedVecsDecl];
  __shared__ int64_t word_es[4 * kMaxPackedVecsDecl], word_ts[4 * kMaxPackedVecsDecl];
  if (threadIdx.x < rw) {
    int off = 0, w = threadIdx.x;
    word_src[w] = nullptr;
    word_es[w] = word_ts[w] = 0;
    for (int f = 0; f < args.n_fields; ++f) {
      const rl8_gather_field &fd = args.f[f];
      const int ew = fd.elem_bytes / 4, words = fd.row_elems * ew;
      if (w >= off && w < off + words) {
        word_src[w] = static_cast<const uint32_t *>(fd.src) + (w - off);
        word_es[w] = fd.env_stride * ew;
        word_ts[w] = fd.time_stride * ew;
      }
      off += words;
    }
  }
  __syncthreads();
  const int64_t env_tiles = (n + kPackEnvs - 1) / kPackEnvs, step_tiles = (h + tile_steps - 1) / tile_steps;
  for (int64_t tile_id = blockIdx.x; tile_id < env_tiles * step_tiles; tile_id += gridDim.x) {
    const int64_t e0 = (tile_id % env_tiles) * kPackEnvs, t0 = (tile_id / env_tiles) * tile_steps;
    const int envs = (int)(n - e0 < kPackEnvs ? n - e0 : kPackEnvs), steps = (int)(h - t0 < tile_steps ? h - t0 : tile_steps);
    // a wave takes every fourth timestep of the tile, eight words of the row -- eight 256-byte loads -- in flight at a time
    for (int tl = wave; tl < steps; tl += kBlock / kWave) {
      for (int w0 = 0; w0 < rw; w0 += 8) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int w = w0 + u;
          v[u] = 0u;
          if (w < rw && lane < envs && word_src[w]) v[u] = word_src[w][(e0 + lane) * word_es[w] + (t0 + tl) * word_ts[w]];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (w0 + u < rw) tile[(tl * kPackEnvs + lane) * pitch + w0 + u] = v[u];
      }
    }
    __syncthreads();
    // out: env-major, this tile's `steps` rows of an env contiguous in memory -- a wave takes every fourth env and
    // writes its steps x row bytes front to back, 1 KiB per store instruction
    if constexpr (DENSE) {
      for (int el = wave; el < envs; el += kBlock / kWave) {
        int off = 0;
        for (int f = 0; f < args.n_fields; ++f) {
          const rl8_gather_field &fd = args.f[f];
          const int words = fd.row_elems * (fd.elem_bytes / 4), per_env = steps * words;
          uint32_t *out = static_cast<uint32_t *>(fd.dst) + ((e0 + el) * h + t0) * words;
          for (int i = lane; i < per_env; i += kWave) {
            const int tl = i / words, c = i - tl * words;
            out[i] = tile[(tl * kPackEnvs + el) * pitch + off + c];
          }
          off += words;
        }
      }
    } else {
      const int vecs = rw / 4, per_env = steps * vecs;
      for (int el = wave; el < envs; el += kBlock / kWave) {
        uint4 *out = reinterpret_cast<uint4 *>(packed + ((e0 + el) * h + t0) * rw);
        for (int i = lane; i < per_env; i += kWave) {
          const int tl = i / vecs, q = i - tl * vecs;
          const uint32_t *w = tile + (tl * kPackEnvs + el) * pitch + 4 * q;
          out[i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
      }
    }
    __syncthreads();
  }
}

template <int VECS>
__global__ __launch_bounds__(kBlock) void gather_packed_kernel(const int64_t *__restrict__ index,
                                                               int64_t m,
                                                               const uint32_t *__restrict__ packed,
                                                               PackedArgs args) {
  __shared__ float4 stage[kBlock * VECS];
  float4 *mine = stage + threadIdx.x * VECS;
  const uint32_t *words_of_mine = reinterpret_cast<const uint32_t *>(mine);
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) {
    const float4 *row = reinterpret_cast<const float4 *>(packed + index[i] * args.row_words);
#pragma unroll
    for (int v = 0; v < VECS; ++v) mine[v] = row[v];
    int off = 0;
#pragma unroll 1
    for (int f = 0; f < args.n_fields; ++f) {
      const rl8_gather_field &fd = args.f[f];
      const int words = fd.row_elems * (fd.elem_bytes / 4);
      uint32_t *dst = static_cast<uint32_t *>(fd.dst) + i * words;
      for (int c = 0; c < words; ++c) dst[c] = words_of_mine[off + c];
      off += words;
    }
  }
}

constexpr int kMaxPackedVecs = 8;  // rows of up to 128 bytes

static int dispatch_gather_packed(int grid, hipStream_t s, const int64_t *index, int64_t m, const uint32_t *packed,
                                  const PackedArgs &args) {
  switch (args.row_words / 4) {
    case 1: gather_packed_kernel<1><<<grid, kBlock, 0, s>>>(index, m, packed, args); break;
    case 2: gather_packed_kernel<2><<<grid, kBlock, 0, s>>>(index, m, packed, args); break;
    case 3: gather_packed_kernel<3><<<grid, kBlock, 0, s>>>(index, m, packed, args); break;
    case 4: gather_packed_kernel<4><<<grid, kBlock, 0, s>>>(index, m, packed, args); break;
    case 5: gather_packed_kernel<5><<<grid, kBlock, 0, s>>>(index, m, packed, args); break;
    case 6: gather_packed_kernel<6><<<grid, kBlock, 0, s>>>(index, m, packed, args); break;
    case 7: gather_packed_kernel<7><<<grid, kBlock, 0, s>>>(index, m, packed, args); break;
    case 8: gather_packed_kernel<8><<<grid, kBlock, 0, s>>>(index, m, packed, args); break;
    default: return RL8_ESIZE;
  }
  return launch_status();
}

// Wide rows (recurrent states: 1 KiB per layer): one wave per gathered row, 16 B
// per lane, so each row moves as whole 1-KiB wave instructions.
__global__ __launch_bounds__(kBlock) void gather_wide_rows_kernel(
    const int64_t *__restrict__ index, int64_t m, int64_t h, rl8_gather_field fd) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
  const int64_t waves = (int64_t)gridDim.x * kWavesPerBlock;
  const int vecs = (int)((int64_t)fd.row_elems * fd.elem_bytes / 16);
  for (int64_t i = wave0; i < m; i += waves) {
    const int64_t s = index ? index[i] : i;
    const int64_t env = s / h, t = s - env * h;
    const char *src = static_cast<const char *>(fd.src) +
                      (env * fd.env_stride + t * fd.time_stride) * fd.elem_bytes;
    char *dst = static_cast<char *>(fd.dst) + i * (int64_t)fd.row_elems * fd.elem_bytes;
    for (int c = lane; c < vecs; c += kWave)
      reinterpret_cast<float4 *>(dst)[c] = reinterpret_cast<const float4 *>(src)[c];
  }
}

}  // namespace rl8

using namespace rl8;

RL8_API int rl8_abi_version(char *arch, int arch_len) {
  if (arch && arch_len > 0) {
    const char *a = "gfx950";
    int i = 0;
    for (; a[i] && i < arch_len - 1; ++i) arch[i] = a[i];
    arch[i] = 0;
  }
  return RL8_ABI_VERSION;
}

RL8_API int64_t rl8_scratch_bytes(void) {
  // partial rows, then the arrival words: one top word and one per group of blocks, 4 KiB apart
  return (int64_t)RL8_MAX_PARTIALS * kPartialWidth * (int64_t)sizeof(double) +
         (int64_t)(1 + (RL8_MAX_PARTIALS + kTicketGroup - 1) / kTicketGroup) * kTicketWordPitch *
             (int64_t)sizeof(unsigned);
}

// The one place the statistics route is decided.  RL8_STATS_GRID_CAP (read once per process; at most the scratch's
// partial rows) lowers the four-envs-per-lane grid so that a small shape takes further trips through the env loop.
RL8_API int rl8_rollout_stats_plan(int64_t n, int64_t h, int64_t env_stride, int64_t time_stride, int aligned16_all,
                                   rl8_stats_plan_t *out) {
  if (!out) return RL8_ENULL;
  if (n <= 0 || h <= 0 || env_stride <= 0 || time_stride <= 0) return RL8_ESIZE;
  static const int cap_env = env_int("RL8_STATS_GRID_CAP");
  const int cap = cap_env > 0 && cap_env < kMaxGrid ? cap_env : kMaxGrid;
  const bool vec = env_stride == 1 && n % 4 == 0 && time_stride % 4 == 0 && aligned16_all != 0;
  const int per_lane = vec ? 4 : 1;
  out->route = vec ? RL8_STATS_VEC4 : RL8_STATS_VEC1;
  out->grid = vec ? grid_for(n, kBlock * 4, cap) : grid_for(n, kBlock);
  const int64_t per_trip = (int64_t)out->grid * kBlock * per_lane;
  out->trips = (n + per_trip - 1) / per_trip;
  return RL8_OK;
}

RL8_API int rl8_rollout_stats_f32(const float *rewards, const float *rdr, int64_t n, int64_t h,
                                  int64_t env_stride, int64_t time_stride, double *stats_out,
                                  void *scratch, void *stream) {
  if (!rewards || !stats_out || !scratch) return RL8_ENULL;
  rl8_stats_plan_t plan;
  if (const int bad = rl8_rollout_stats_plan(n, h, env_stride, time_stride, aligned16(rewards) && (!rdr || aligned16(rdr)),
                                             &plan))
    return bad;
  hipStream_t s = (hipStream_t)stream;
  double *partials = (double *)scratch;
  const bool vec = plan.route == RL8_STATS_VEC4;
  const dim3 grid = plan.grid;
  auto launch = [&](auto kernel) {
    kernel<<<grid, kBlock, 0, s>>>(rewards, rdr, n, h, env_stride, time_stride, partials,
                                   stats_out);
  };
  if (vec)
    rdr ? launch(rollout_stats_kernel<4, true>) : launch(rollout_stats_kernel<4, false>);
  else
    rdr ? launch(rollout_stats_kernel<1, true>) : launch(rollout_stats_kernel<1, false>);
  return launch_status();
}

static int packed_args(const rl8_gather_field *fields, int n_fields, int row_words, bool need_src, bool need_dst, PackedArgs *args);
template <bool DENSE>
static int launch_pack_tiled(const PackedArgs &args, int64_t n, int64_t h, uint32_t *packed, hipStream_t stream);

// The one place the routes of rl8_gather_minibatch are decided: per field GENERAL, WIDE_ROWS or TILED (and for TILED the
// group, a run of consecutive fields that share one tile launch), and the number of launches.
//   index = NULL (every sample in order, m = n h): a tiled transposition, each byte read and written once.  A tile's row
//     holds at most 4 kMaxPackedVecs words, so the fields go in groups that fit, in the order given; a field wider than
//     that closes the current group and takes the routes below with the implicit index i.
//   wide rows: whole 16-byte pieces, 256 bytes and up, every row start of source and destination 16-byte aligned.
//   general: everything else, all such fields in one launch.
RL8_API int rl8_gather_minibatch_plan(int indexed, int64_t m, int64_t h, const rl8_gather_field *fields, int n_fields,
                                      int *routes_out, int *groups_out, int *launches_out) {
  if (!fields || !routes_out || !groups_out || !launches_out) return RL8_ENULL;
  if (m <= 0 || h <= 0 || n_fields <= 0 || n_fields > RL8_MAX_GATHER_FIELDS) return RL8_ESIZE;
  if (!indexed && m % h) return RL8_ESIZE;
  constexpr int kTileWords = 4 * kMaxPackedVecsDecl;
  int groups = 0, words = 0, wide_fields = 0, general_fields = 0;  // (words: of the open tiled group; 0 = none open)
  for (int f = 0; f < n_fields; ++f) {
    const rl8_gather_field &fd = fields[f];
    if (!fd.src || !fd.dst) return RL8_ENULL;
    if (fd.elem_bytes != 4 && fd.elem_bytes != 8) return RL8_ECONFIG;
    if (fd.row_elems <= 0) return RL8_ESIZE;
    const int64_t row_bytes = (int64_t)fd.row_elems * fd.elem_bytes;
    if (!indexed && row_bytes <= 4 * kTileWords) {
      const int w = (int)(row_bytes / 4);
      if (words == 0 || words + w > kTileWords) ++groups, words = 0;
      words += w;
      routes_out[f] = RL8_GATHER_TILED;
      groups_out[f] = groups - 1;
      continue;
    }
    words = 0;  // (closes the open group: groups are runs of consecutive fields)
    const bool wide = row_bytes >= 256 && row_bytes % 16 == 0 && aligned16(fd.src) && aligned16(fd.dst) &&
                      (fd.env_stride * fd.elem_bytes) % 16 == 0 && (fd.time_stride * fd.elem_bytes) % 16 == 0;
    routes_out[f] = wide ? RL8_GATHER_WIDE_ROWS : RL8_GATHER_GENERAL;
    groups_out[f] = -1;
    wide ? ++wide_fields : ++general_fields;
  }
  *launches_out = groups + wide_fields + (general_fields > 0 ? 1 : 0);
  return RL8_OK;
}

RL8_API int rl8_gather_minibatch(const int64_t *index, int64_t m, int64_t h,
                                 const rl8_gather_field *fields, int n_fields, void *stream) {
  int routes[RL8_MAX_GATHER_FIELDS], groups[RL8_MAX_GATHER_FIELDS], launches = 0;
  if (const int bad = rl8_gather_minibatch_plan(index != nullptr, m, h, fields, n_fields, routes, groups, &launches))
    return bad;
  hipStream_t s = (hipStream_t)stream;
  GatherArgs args;
  args.n_fields = 0;
  for (int f = 0; f < n_fields;) {
    const rl8_gather_field &fd = fields[f];
    if (routes[f] == RL8_GATHER_TILED) {
      int stop = f, words = 0;
      for (; stop < n_fields && routes[stop] == RL8_GATHER_TILED && groups[stop] == groups[f]; ++stop)
        words += fields[stop].row_elems * (fields[stop].elem_bytes / 4);
      PackedArgs tiled;
      if (const int st = packed_args(fields + f, stop - f, (words + 3) / 4 * 4, true, true, &tiled)) return st;
      if (const int st = launch_pack_tiled<true>(tiled, m / h, h, nullptr, s)) return st;
      f = stop;
      continue;
    }
    if (routes[f] == RL8_GATHER_WIDE_ROWS) {
      gather_wide_rows_kernel<<<grid_for(m, kWavesPerBlock), kBlock, 0, s>>>(index, m, h, fd);
      if (const int st = launch_status()) return st;
    } else {
      args.f[args.n_fields++] = fd;
    }
    ++f;
  }
  if (args.n_fields > 0)
    gather_minibatch_kernel<<<grid_for(m, kBlock), kBlock, 0, s>>>(index, m, h, args);
  return launch_status();
}

RL8_API int rl8_gather_sequences(const int64_t *seq_index, int64_t num_seqs, int seq_len, int64_t h,
                                 const rl8_gather_field *fields, int n_fields, void *stream) {
  if (!fields) return RL8_ENULL;
  if (num_seqs <= 0 || seq_len <= 0 || h <= 0 || h % seq_len || n_fields <= 0 || n_fields > RL8_MAX_GATHER_FIELDS)
    return RL8_ESIZE;
  GatherArgs args;
  args.n_fields = n_fields;
  for (int f = 0; f < n_fields; ++f) {
    const rl8_gather_field &fd = fields[f];
    if (!fd.src || !fd.dst) return RL8_ENULL;
    if (fd.elem_bytes != 1 && fd.elem_bytes != 4 && fd.elem_bytes != 8) return RL8_ECONFIG;
    if (fd.row_elems <= 0) return RL8_ESIZE;
    const uintptr_t mask = (uintptr_t)fd.elem_bytes - 1;
    if ((reinterpret_cast<uintptr_t>(fd.src) & mask) || (reinterpret_cast<uintptr_t>(fd.dst) & mask)) return RL8_EALIGN;
    args.f[f] = fd;
  }
  const int64_t rows = num_seqs * seq_len;
  gather_sequences_kernel<<<grid_for(rows, kBlock), kBlock, 0, (hipStream_t)stream>>>(seq_index, rows, seq_len, h, args);
  return launch_status();
}

// Argument checks shared by the two window entries.
static int window_args(const rl8_window_field *fields, int n_fields, WindowArgs *args) {
  if (!fields) return RL8_ENULL;
  if (n_fields <= 0 || n_fields > RL8_MAX_GATHER_FIELDS) return RL8_ESIZE;
  args->n_fields = n_fields;
  for (int f = 0; f < n_fields; ++f) {
    const rl8_window_field &fd = fields[f];
    if (!fd.src || !fd.dst) return RL8_ENULL;
    if (fd.elem_bytes != 1 && fd.elem_bytes != 4 && fd.elem_bytes != 8) return RL8_ECONFIG;
    if (fd.row_elems <= 0 || fd.size < 1) return RL8_ESIZE;
    if (fd.size > 1 && !fd.mask) return RL8_ECONFIG;
    const uintptr_t low = (uintptr_t)fd.elem_bytes - 1;
    if ((reinterpret_cast<uintptr_t>(fd.src) & low) || (reinterpret_cast<uintptr_t>(fd.dst) & low)) return RL8_EALIGN;
    args->f[f] = fd;
    if (fd.size == 1) args->f[f].mask = nullptr;  // (a plain gather has no mask)
  }
  return RL8_OK;
}

RL8_API int rl8_gather_windows(const int64_t *index, int64_t m, int64_t h, const rl8_window_field *fields,
                               int n_fields, void *stream) {
  if (!fields) return RL8_ENULL;
  if (m <= 0 || h <= 0) return RL8_ESIZE;
  WindowArgs args;
  if (const int st = window_args(fields, n_fields, &args)) return st;
  int64_t cells = 0;  // the widest field sizes the grid; the others stride over it
  for (int f = 0; f < n_fields; ++f) cells = cells > m * args.f[f].size ? cells : m * args.f[f].size;
  gather_windows_kernel<<<grid_for(cells, kBlock), kBlock, 0, (hipStream_t)stream>>>(index, m, h, args);
  return launch_status();
}

RL8_API int rl8_window_last(int64_t t, int64_t n, const rl8_window_field *fields, int n_fields, void *stream) {
  if (!fields) return RL8_ENULL;
  if (t < 0 || n <= 0) return RL8_ESIZE;
  WindowArgs args;
  if (const int st = window_args(fields, n_fields, &args)) return st;
  int64_t cells = 0;  // the widest field sizes the grid; the others stride over it
  for (int f = 0; f < n_fields; ++f) cells = cells > n * args.f[f].size ? cells : n * args.f[f].size;
  window_last_kernel<<<grid_for(cells, kBlock), kBlock, 0, (hipStream_t)stream>>>(t, n, args);
  return launch_status();
}

static int packed_args(const rl8_gather_field *fields, int n_fields, int row_words, bool need_src,
                       bool need_dst, PackedArgs *args) {
  if (!fields) return RL8_ENULL;
  if (n_fields <= 0 || n_fields > RL8_MAX_GATHER_FIELDS) return RL8_ESIZE;
  int words = 0;
  for (int f = 0; f < n_fields; ++f) {
    const rl8_gather_field &fd = fields[f];
    if ((need_src && !fd.src) || (need_dst && !fd.dst)) return RL8_ENULL;
    if (fd.elem_bytes != 4 && fd.elem_bytes != 8) return RL8_ECONFIG;
    if (fd.row_elems <= 0) return RL8_ESIZE;
    words += fd.row_elems * (fd.elem_bytes / 4);
    args->f[f] = fd;
  }
  if (row_words < words || row_words % 4 || row_words > 4 * kMaxPackedVecs) return RL8_ESIZE;
  args->n_fields = n_fields;
  args->row_words = row_words;
  return RL8_OK;
}

// The launch shape of the tiled transposition, shared by rl8_pack_samples and rl8_gather_minibatch(index = NULL).
// timesteps per tile: 36 KiB of LDS (16 steps of 32-byte rows), four workgroups per CU -- measured at 2^20 x 32:
// 18 KiB 463 us, 36 KiB 471, 72 KiB (32 steps, two per CU) 632, the lane-per-sample kernel 967
RL8_API int rl8_pack_plan(int64_t n, int64_t h, int row_words, rl8_pack_plan_t *out) {
  if (!out) return RL8_ENULL;
  if (n <= 0 || h <= 0 || row_words <= 0 || row_words % 4 || row_words > 4 * kMaxPackedVecs) return RL8_ESIZE;
  const int per_step = kPackEnvs * (row_words + 1) * 4;
  static const int lds_kib = env_int("RL8_PACK_TILE_KIB") > 0 ? env_int("RL8_PACK_TILE_KIB") : 36;
  int tile_steps = (lds_kib * 1024 + per_step - 1) / per_step;
  tile_steps = tile_steps > kPackSteps ? kPackSteps : tile_steps < 1 ? 1 : tile_steps;
  if (tile_steps > h) tile_steps = (int)h;
  const int lds = tile_steps * per_step;
  const int per_cu = (160 * 1024) / (lds + 512) < 1 ? 1 : (160 * 1024) / (lds + 512);
  out->tile_steps = tile_steps;
  out->lds_bytes = lds;
  out->tiles = ((n + kPackEnvs - 1) / kPackEnvs) * ((h + tile_steps - 1) / tile_steps);
  out->grid = (int)(out->tiles < (int64_t)per_cu * kCUs ? out->tiles : (int64_t)per_cu * kCUs);
  return RL8_OK;
}

// The tiled transposition behind rl8_pack_samples (packed rows) and rl8_gather_minibatch(index = NULL) (dense fields).
template <bool DENSE>
static int launch_pack_tiled(const PackedArgs &args, int64_t n, int64_t h, uint32_t *packed, hipStream_t stream) {
  rl8_pack_plan_t plan;
  if (const int bad = rl8_pack_plan(n, h, args.row_words, &plan)) return bad;
  if (const int e = allow_dynamic_lds<&pack_samples_tiled_kernel<DENSE>>()) return e;
  pack_samples_tiled_kernel<DENSE><<<plan.grid, kBlock, plan.lds_bytes, stream>>>(n, h, packed, args, plan.tile_steps);
  return launch_status();
}

RL8_API int rl8_pack_samples(const rl8_gather_field *fields, int n_fields, int64_t n, int64_t h,
                             void *packed, int row_words, void *stream) {
  if (!packed) return RL8_ENULL;
  if (n <= 0 || h <= 0) return RL8_ESIZE;
  if (!aligned16(packed)) return RL8_EALIGN;
  PackedArgs args;
  const int st = packed_args(fields, n_fields, row_words, true, false, &args);
  if (st != RL8_OK) return st;
  return launch_pack_tiled<false>(args, n, h, static_cast<uint32_t *>(packed), (hipStream_t)stream);
}

RL8_API int rl8_gather_packed(const int64_t *index, int64_t m, const void *packed, int row_words,
                              const rl8_gather_field *fields, int n_fields, void *stream) {
  if (!index || !packed) return RL8_ENULL;
  if (m <= 0) return RL8_ESIZE;
  PackedArgs args;
  const int st = packed_args(fields, n_fields, row_words, false, true, &args);
  if (st != RL8_OK) return st;
  if (!aligned16(packed)) return RL8_EALIGN;
  return dispatch_gather_packed(grid_for(m, kBlock), (hipStream_t)stream, index, m, static_cast<const uint32_t *>(packed), args);
}
