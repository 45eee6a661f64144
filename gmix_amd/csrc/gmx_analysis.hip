// gmx_analysis.hip -- the analysis averages on the device (gmx_analysis.h; host side gmx_analysis.inc, DESIGN.md section
// 4.23).  A column's chain over a stream's bits is serial -- two dependent double operations per bit -- while the
// logistic, the clamp and log2f of the bits are independent, and so are the columns and the streams:
//
//   gmx_analysis_kernel        a block per stream and 64 neighbouring columns, tiles of 64 bits.  Per tile the block's four
//                              waves compute the tile's entropy floats, the lanes running ALONG a record (neighbouring
//                              columns read neighbouring slots of the prediction row), all loads of the tile ahead of
//                              the math, and lay them into LDS, a row per column (stride 65 words: the walk's read is
//                              conflict free).  Lane c of the first wave then walks its column: gmx_analysis_step per
//                              bit, and at a sample bit the average goes to the stream's rows area.  The counts are ragged; a stream with 0 bits sits
//                              the launch out.
//   gmx_analysis_reset_kernel  averages of a range of streams from a given vector or to zero, a lane per entry.
//   gmx_analysis_pack_kernel   the take: per stream the header line, the C averages, the captured rows and their labels,
//                              in whole 8-byte words into pinned host memory: what crosses the link is what was captured,
//                              not the areas' capacity.
//
// bits_seen, the rows captured and the frequency of every stream are the host's (its mirror is exact: they depend on
// the counts alone); they arrive with the counts in the launch's staged list.
#include <hip/hip_runtime.h>

#include "gmx_analysis.h"
#include "gmx_analysis_dev.h"

#define GMX_AN_STRIDE (GMX_AN_TILE + 1)
#define GMX_AN_THREADS 256
#define GMX_AN_ROWS (GMX_AN_TILE * GMX_AN_COLS / GMX_AN_THREADS)  // bits of a tile a thread computes at most

__global__ __launch_bounds__(GMX_AN_THREADS) void gmx_analysis_kernel(const GmxAnArgs a) {
  __shared__ float tile[GMX_AN_COLS * GMX_AN_STRIDE];
  __shared__ uint64_t exp_tab[32];   // the two tables' entries are picked per lane: from LDS, not from memory
  __shared__ double log_tab[16][2];
  const uint32_t s = blockIdx.x, S = (uint32_t)a.n_streams;
  const uint64_t n = a.list[GMX_AN_L_NBITS * S + s];
  if (n == 0) return;  // (block-uniform)
  if (threadIdx.x < 32u) {
    exp_tab[threadIdx.x] = gmx_exp2f_tab[threadIdx.x];
    log_tab[threadIdx.x >> 1][threadIdx.x & 1u] = gmx_log2f_tab[threadIdx.x >> 1][threadIdx.x & 1u];
  }
  __syncthreads();
  const uint32_t C = a.n_columns, c0 = blockIdx.y * GMX_AN_COLS;
  // The tile's entropy floats: the block's columns rounded up to a power of two go along the lanes, the bits across
  // what is left of the 256 threads, so that a block of 32 columns keeps every lane busy.  A thread has one column and
  // at most GMX_AN_ROWS bits of a tile.
  const uint32_t cb = C - c0 < (uint32_t)GMX_AN_COLS ? C - c0 : (uint32_t)GMX_AN_COLS;
  const uint32_t lg = cb > 1u ? 32u - (uint32_t)__clz((int)(cb - 1u)) : 0u;
  const uint32_t cl = threadIdx.x & ((1u << lg) - 1u), tr = threadIdx.x >> lg, tstep = GMX_AN_THREADS >> lg;
  const bool live = cl < cb;
  // where this thread's column comes from
  const float* src = nullptr;
  size_t stride = 0;
  bool is_prob = false;
  const uint32_t* mask = nullptr;
  uint32_t mask_bit = 0;
  if (live) {
    const uint32_t c = c0 + cl, kind = a.cols[2 * c], index = a.cols[2 * c + 1];
    is_prob = kind == GMX_AN_K_FINAL_P;
    if (a.values) {
      src = a.values + c;
      stride = C;
    } else if (kind == GMX_AN_K_INPUT) {
      src = a.pred + index;
      stride = a.n_pad;
      if (a.mask) {
        mask = a.mask + (index >> 5);
        mask_bit = index & 31u;
      }
    } else if (kind == GMX_AN_K_MIXER) {
      src = a.out + index;
      stride = a.m;
    } else {
      src = a.p;
      stride = 1;
    }
  }
  // the walk: lane l of the first wave has column c0 + l
  const uint32_t wc = c0 + threadIdx.x;
  const bool walker = threadIdx.x < cb;
  const uint64_t seen0 = a.list[GMX_AN_L_SEEN * S + s], F = a.list[GMX_AN_L_FREQ * S + s];
  uint64_t r = a.list[GMX_AN_L_ROWS * S + s], next = gmx_an_first(seen0, F);
  const size_t row0 = (size_t)s * a.pitch;
  double e = walker ? a.ema[(size_t)s * C + wc] : 0.0;
  for (uint64_t t0 = 0; t0 < n; t0 += GMX_AN_TILE) {
    const uint32_t cnt = (uint32_t)(n - t0 < (uint64_t)GMX_AN_TILE ? n - t0 : (uint64_t)GMX_AN_TILE);
    // every load of the tile goes out before the first logistic
    float v[GMX_AN_ROWS];
    uint32_t bits = 0u, silent = 0u;
#pragma unroll
    for (uint32_t k = 0; k < GMX_AN_ROWS; ++k) {
      const uint32_t t = tr + k * tstep;
      v[k] = 0.0f;
      if (live && t < cnt) {
        const size_t row = row0 + t0 + t;
        v[k] = src[row * stride];
        bits |= (a.bits[row] ? 1u : 0u) << k;
        if (mask) silent |= (~(mask[row * a.mask_words] >> mask_bit) & 1u) << k;
      }
    }
#pragma unroll 2
    for (uint32_t k = 0; k < GMX_AN_ROWS; ++k) {
      const uint32_t t = tr + k * tstep;
      if (live && t < cnt) {
        const float x = (silent >> k) & 1u ? 0.0f : v[k];  // a silent model left Predict's zero
        const float prob = is_prob ? x : gmx_logistic_tab(x, exp_tab);
        tile[cl * GMX_AN_STRIDE + t] = gmx_analysis_entropy_of_prob_from(prob, (int)((bits >> k) & 1u), log_tab);
      }
    }
    __syncthreads();
    if (walker) {
      for (uint32_t i = 0; i < cnt; ++i) {
        e = gmx_analysis_step(e, tile[threadIdx.x * GMX_AN_STRIDE + i]);
        if (t0 + i == next) {  // RunAnalysis's row, labelled bits_seen
          if (r < a.max_samples) {
            a.rows[((size_t)s * a.max_samples + r) * C + wc] = e;
            if (wc == 0) a.labels[(size_t)s * a.max_samples + r] = seen0 + next;
          }
          ++r;
          next = F > ~0ull - next ? ~0ull : next + F;
        }
      }
    }
    __syncthreads();
  }
  if (walker) a.ema[(size_t)s * C + wc] = e;
}

__global__ __launch_bounds__(256) void gmx_analysis_reset_kernel(double* ema, const double* __restrict__ src, int s0,
                                                                 uint64_t n_entries, uint32_t n_columns) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_entries) return;
  ema[(size_t)s0 * n_columns + i] = src ? src[i % n_columns] : 0.0;
}

__global__ __launch_bounds__(256) void gmx_analysis_pack_kernel(const GmxAnPackArgs a) {
  const uint32_t s = blockIdx.x, S = (uint32_t)a.n_streams, C = a.n_columns;
  const uint64_t seen = a.list[s], n_rows = a.list[S + s], off = a.list[2 * S + s];
  const uint64_t k = n_rows < a.max_samples ? n_rows : a.max_samples;
  if (threadIdx.x == 0) {
    uint64_t* line = (uint64_t*)(a.packed + (size_t)s * GMX_AN_HEAD);
    line[0] = seen;
    line[1] = k;
  }
  double* dst = (double*)(a.packed + a.body_off + off);
  const double* ema = a.ema + (size_t)s * C;
  for (uint32_t i = threadIdx.x; i < C; i += 256u) dst[i] = ema[i];
  const double* rows = a.rows + (size_t)s * a.max_samples * C;
  const uint64_t n = k * C;
  for (uint64_t i = threadIdx.x; i < n; i += 256u) dst[C + i] = rows[i];
  uint64_t* lab = (uint64_t*)(dst + C + n);
  const uint64_t* labels = a.labels + (size_t)s * a.max_samples;
  for (uint64_t i = threadIdx.x; i < k; i += 256u) lab[i] = labels[i];
}

extern "C" hipError_t gmx_launch_analysis(const GmxAnArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  if (a->n_streams < 1 || a->n_columns < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_analysis_kernel, dim3((unsigned)a->n_streams, (a->n_columns + GMX_AN_COLS - 1) / GMX_AN_COLS),
                     dim3(GMX_AN_THREADS), 0, stream, *a);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_analysis_reset(double* ema, const double* src, int s0, int n, uint32_t n_columns,
                                                hipStream_t stream) {
  (void)hipGetLastError();
  if (n < 1 || s0 < 0 || n_columns < 1) return hipErrorInvalidValue;
  const uint64_t entries = (uint64_t)n * n_columns;
  hipLaunchKernelGGL(gmx_analysis_reset_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, stream, ema, src, s0,
                     entries, n_columns);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_analysis_pack(const GmxAnPackArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  if (a->n_streams < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_analysis_pack_kernel, dim3((unsigned)a->n_streams), dim3(256), 0, stream, *a);
  return hipGetLastError();
}
