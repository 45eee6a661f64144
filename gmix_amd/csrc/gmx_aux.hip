// gmx_aux.hip -- small gfx950 kernels around the hot path: the synthetic record generator
// of the benchmark, the device-side math probes of the parity tests, bank initialisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmx_coder.h"
#include "gmx_internal.h"
#include "gmx_math.h"
#include "gmx_step_dev.h"

// ---------------------------------------------------------------------------------------
// Synthetic record generator (BASELINE.json configs[1]; definition in oracle/gmx_synth.h,
// restated here for the device): one thread walks one stream's xorshift64 sequence.
// ---------------------------------------------------------------------------------------
struct GmxSynthArgs {
  float* pred;        // [S][rec_stride][n_pad]
  uint32_t* mask;     // [S][rec_stride][mask_words] or null
  uint32_t* ctx;      // [S][rec_stride][m]
  uint8_t* bits;      // [S][rec_stride]
  uint64_t* rng;      // [S] persistent xorshift state
  uint64_t* tcount;   // [S] bits generated so far (for the every-8th-bit context modes)
  float* pstate;      // [S][n_pad] persistent prediction slots
  uint32_t* cstate;   // [S][m] persistent contexts
  uint64_t rec_stride, n_bits, seed;
  int32_t n, n_pad, m, mask_words, n_streams, restart, ctx_mode, bit_mode;
  uint32_t ctx_mod, zero_mod;
};

// bit j set = gate context j is redrawn every bit in ctx_mode 4/5 (GMX_SYNTH_BITLEVEL)
constexpr uint64_t kSynthBitLevel = (1ull << 2) | (1ull << 11) | (1ull << 26) | (1ull << 29);

__device__ __forceinline__ uint32_t gmx_xs64(uint64_t& s) {
  s ^= s << 13;
  s ^= s >> 7;
  s ^= s << 17;
  return (uint32_t)(s >> 11);
}

__global__ void __launch_bounds__(64) gmx_synth_kernel(const GmxSynthArgs a) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.n_streams) return;
  float* pst = a.pstate + (uint64_t)s * a.n_pad;
  uint32_t* cst = a.cstate + (uint64_t)s * a.m;
  uint64_t st, tc;
  if (a.restart) {
    st = a.seed + (uint64_t)s * 0x9E3779B97F4A7C15ull;
    if (st == 0) st = 0x9E3779B97F4A7C15ull;
    tc = 0;
    for (int i = 0; i < a.n_pad; ++i) pst[i] = 0.f;
    for (int j = 0; j < a.m; ++j) cst[j] = 0u;
  } else {
    st = a.rng[s];
    tc = a.tcount[s];
  }
  const uint32_t cmod = a.ctx_mod ? a.ctx_mod : 1u;
  for (uint64_t t = 0; t < a.n_bits; ++t) {
    float* pr = a.pred + ((uint64_t)s * a.rec_stride + t) * a.n_pad;
    uint32_t* mk = a.mask ? a.mask + ((uint64_t)s * a.rec_stride + t) * a.mask_words : nullptr;
    uint32_t* cx = a.ctx + ((uint64_t)s * a.rec_stride + t) * a.m;
    uint32_t mword = 0;
    for (int i = 0; i < a.n; ++i) {
      bool act = false;
      bool silent = false;
      if (a.zero_mod) {
        const uint32_t dr = gmx_xs64(st);
        silent = (dr % a.zero_mod) == 0;
      }
      if (!silent) {
        const float x = (float)((int)(gmx_xs64(st) % 2001u) - 1000) / 250.0f;
        pst[i] = x;
        act = (x != 0.0f);
      }
      pr[i] = pst[i];
      if (act) mword |= 1u << (i & 31);
      if ((i & 31) == 31 || i == a.n - 1) {
        if (mk) mk[i >> 5] = mword;
        mword = 0;
      }
    }
    for (int i = a.n; i < a.n_pad; ++i) pr[i] = 0.f;
    const bool redraw = (a.ctx_mode < 2) || ((tc & 7u) == 0);
    if (redraw) {
      for (int j = 0; j < a.m; ++j) {
        uint32_t c = gmx_xs64(st);
        if (a.ctx_mode & 1) c %= cmod;
        cst[j] = c;
      }
    } else if (a.ctx_mode >= 4) {
      for (int j = 0; j < a.m && j < 64; ++j) {
        if (!((kSynthBitLevel >> j) & 1)) continue;
        uint32_t c = gmx_xs64(st);
        if (a.ctx_mode & 1) c %= cmod;
        cst[j] = c;
      }
    }
    for (int j = 0; j < a.m; ++j) cx[j] = cst[j];
    ++tc;
    const uint32_t r = gmx_xs64(st);
    uint32_t bit = r & 1u;
    if (a.bit_mode == 1) bit = (uint32_t)((pst[0] > 0.0f) ^ ((r & 7u) == 0));
    a.bits[(uint64_t)s * a.rec_stride + t] = (uint8_t)bit;
  }
  a.rng[s] = st;
  a.tcount[s] = tc;
}

extern "C" hipError_t gmx_launch_synth_kernel(const GmxSynthArgs* args, hipStream_t stream) {
  const int blocks = (args->n_streams + 63) / 64;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_synth_kernel, dim3(blocks), dim3(64), 0, stream, *args);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Synthetic records for the Indirect models (definition in oracle/gmx_ind_synth.h, restated
// here for the device): byte-structured contexts, one thread per stream.
// ---------------------------------------------------------------------------------------
struct GmxIndSynthArgs {
  uint32_t* ctx;      // [S][rec_stride][k]
  uint32_t* bc;       // [S][rec_stride]
  uint8_t* bits;      // [S][rec_stride]
  uint64_t* rng;      // [S]
  uint32_t* recent;   // [S] recent_bits
  uint32_t* cstate;   // [S][k] contexts of the current byte
  uint64_t rec_stride, n_bits, seed;
  int32_t k, n_streams, restart;
  uint32_t ctx_mod[4];
};

__global__ void __launch_bounds__(64) gmx_ind_synth_kernel(const GmxIndSynthArgs a) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.n_streams) return;
  uint32_t* cst = a.cstate + (uint64_t)s * a.k;
  uint64_t st;
  uint32_t recent;
  if (a.restart) {
    st = a.seed + (uint64_t)s * 0x9E3779B97F4A7C15ull;
    if (st == 0) st = 0x9E3779B97F4A7C15ull;
    recent = 1;
    for (int j = 0; j < a.k; ++j) cst[j] = 0u;
  } else {
    st = a.rng[s];
    recent = a.recent[s];
  }
  for (uint64_t t = 0; t < a.n_bits; ++t) {
    uint32_t* cx = a.ctx + ((uint64_t)s * a.rec_stride + t) * a.k;
    if (recent == 1) {  // byte boundary: every context is redrawn
      for (int j = 0; j < a.k; ++j) {
        uint32_t c = gmx_xs64(st);
        const uint32_t m = a.ctx_mod[j & 3];
        if (m) c %= m;
        cst[j] = c;
      }
    }
    for (int j = 0; j < a.k; ++j) cx[j] = cst[j];
    const uint32_t bcx = recent - 1;
    a.bc[(uint64_t)s * a.rec_stride + t] = bcx;
    const uint32_t r = gmx_xs64(st);
    const uint32_t bit = ((cst[0] ^ (bcx * 7u)) & 1u) ^ (uint32_t)((r % 5u) == 0);
    a.bits[(uint64_t)s * a.rec_stride + t] = (uint8_t)bit;
    recent = recent * 2 + bit;
    if (recent >= 256) recent = 1;
  }
  a.rng[s] = st;
  a.recent[s] = recent;
}

extern "C" hipError_t gmx_launch_ind_synth_kernel(const GmxIndSynthArgs* args, hipStream_t stream) {
  const int blocks = (args->n_streams + 63) / 64;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ind_synth_kernel, dim3(blocks), dim3(64), 0, stream, *args);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// Device-side math probes for the parity tests (the same gmx_math.h the kernels use).
// ---------------------------------------------------------------------------------------
// what: 0 expf, 1 logistic, 2 squash-clamp; then what the LSTM byte model calls (gmx_lstm.hip): 5 logf, 6 logit,
// 7 expm1f, 8 tanhf, 9 the logistic with the 2^(i/32) table in LDS as that kernel holds it, 10 the layer-norm
// scale of a sum of squares, 11 Adam's step on tuples of six operands; 12 and 13 the byte graphs' two functions
// (gmx_coder.h) on tuples of 32-bit words carried as floats: the arithmetic decoder's bit, ModPPMD's range walk.
__device__ __forceinline__ float gmx_math_unary(float v, int what, const uint64_t* lds_tab) {
  switch (what) {
    case 0: return gmx_expf(v);
    case 1: return gmx_logistic(v);
    case 5: return gmx_logf(v);
    case 6: return gmx_logit(v);
    case 7: return gmx_expm1f(v);
    case 8: return gmx_tanhf(v);
    case 9: return gmx_logistic_tab(v, lds_tab);
    case 10: return gmx_lstm_norm_scale(v, (float)GMX_L_NC);
    default: return gmx_squash_clamp(v);
  }
}

#define GMX_PROBE_WALK_SENTINEL 0xc2f60000u  // -123.0f, as tests/cpp/test_coder.cpp presets its slot
__global__ void gmx_math_probe_kernel(const float* x, float* y, uint64_t n, int what) {
  __shared__ uint64_t tab[32];
  if (threadIdx.x < 32) tab[threadIdx.x] = gmx_exp2f_tab[threadIdx.x];
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (what == 11) {
    // x[6j .. 6j+5] = (weight, alpha, m, d1, v, d2) of tuple j, the result goes to y[6j] (the rest of y is 0)
    const bool head = i % 6 == 0 && i + 5 < n;
    y[i] = head ? gmx_lstm_adam_step(x[i], x[i + 1], x[i + 2], x[i + 3], x[i + 4], x[i + 5]) : 0.0f;
    return;
  }
  if (what == 12) {
    // x[8j .. 8j+7] = {x1, x2, x, p, next4, avail, 0, 0}: next4 holds the next four input bytes, the first in its
    // low byte, of which the input has only `avail` (0 .. 4).  y[8j .. 8j+7] = {bit, x1, x2, x, consumed, pr, 0, 0}.
    if (i % 8 != 0) return;  // (the tuple's first thread writes all of it)
    if (i + 7 >= n) {
      for (uint64_t k = i; k < n; ++k) y[k] = 0.0f;
      return;
    }
    const uint32_t next4 = gmx_f2u(x[i + 4]), avail = gmx_f2u(x[i + 5]);
    uint8_t in[4];
    for (int k = 0; k < 4; ++k) in[k] = (uint8_t)(next4 >> (8 * k));
    GmxCoderState st = {gmx_f2u(x[i]), gmx_f2u(x[i + 1]), gmx_f2u(x[i + 2]), 0u};
    const float p = x[i + 3];
    const uint32_t bit = gmx_coder_decode(&st, p, in, avail < 4u ? avail : 4u);
    const uint32_t out[8] = {bit, st.x1, st.x2, st.x, st.pos, gmx_coder_discretize(p), 0u, 0u};
    for (int k = 0; k < 8; ++k) y[i + k] = gmx_u2f(out[k]);
    return;
  }
  if (what == 13) {
    // x[260j .. 260j+259] = {top, bot, 0, 0, ppm[256]} with 0 <= bot <= top <= 255 (anything else answers nothing).
    // y[260j .. 260j+2] = {wrote, slot, active}, the rest of y is 0; slot and active start from sentinels, so a
    // walk that writes nothing shows them.
    const uint64_t k = i % 260;
    const bool whole = i - k + 259 < n;
    if (whole && k >= 1 && k <= 2) return;  // (the case's first thread writes them)
    if (!whole || k != 0) {
      y[i] = 0.0f;
      return;
    }
    const GmxCoderWalk w = {(int32_t)gmx_f2u(x[i]), (int32_t)gmx_f2u(x[i + 1])};
    float slot = gmx_u2f(GMX_PROBE_WALK_SENTINEL);
    bool active = true, wrote = false;
    if (w.bot >= 0 && w.bot <= w.top && w.top <= 255) wrote = gmx_coder_walk_predict(&w, x + i + 4, &slot, &active);
    y[i] = gmx_u2f(wrote ? 1u : 0u);
    y[i + 1] = slot;
    y[i + 2] = gmx_u2f(active ? 1u : 0u);
    return;
  }
  y[i] = gmx_math_unary(x[i], what, tab);
}

// Compare device gmx_expf / gmx_logistic over a whole range of float bit patterns against a
// host-computed table is too slow over PCIe; instead the device checksums its results and
// the host checksums its own: out[0] = xor-fold, out[1] = sum of the result bit patterns.
__global__ void gmx_math_range_kernel(uint64_t lo, uint64_t count, int what,
                                      unsigned long long* out) {
  __shared__ uint64_t tab[32];
  if (threadIdx.x < 32) tab[threadIdx.x] = gmx_exp2f_tab[threadIdx.x];
  __syncthreads();
  unsigned long long x = 0, sacc = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t u = (uint32_t)(lo + i);
    const float v = gmx_u2f(u);
    float r;
    if (what == 3) {
      // the wave-level logistic of gmx_stock.hip (short way where a whole wave has |v| < 64): the caller
      // compares the checksums with those of what == 1
      r = gmx_wave_logistic(v, gmx_exp2f_tab);
    } else if (what == 4) {
      // the short row-age division against the general one on a pair of counters below 2^32 made from i:
      // small pairs exhaustively (i < 2^24: 4096 x 4096), then hashed ones with the edges mixed in; the
      // checksums count the differing bit patterns
      const uint64_t i64 = lo + i;
      uint32_t ca, cb;
      if (i64 < (1ull << 24)) {
        ca = (uint32_t)(i64 & 4095u);
        cb = (uint32_t)(i64 >> 12) + 1u;
      } else {
        uint64_t h = i64 * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 32;
        cb = (uint32_t)h >> ((h >> 59) & 31u);
        if (cb == 0) cb = 0xffffffffu;
        ca = (uint32_t)(h >> 32) >> ((h >> 54) & 31u);
        if ((i64 & 7u) == 0) ca = ca % cb;          // the reference's case: row.steps <= max_steps_
        if ((i64 & 1023u) == 1) ca = cb;
        if ((i64 & 1023u) == 2) ca = cb - 1u;
      }
      const double q_short = gmx_row_age_short(ca, cb), q_gen = (double)ca / (double)cb;
      const bool bad = gmx_d2u(q_short) != gmx_d2u(q_gen);
      x ^= bad ? i64 + 1 : 0;
      sacc += bad ? 1 : 0;
      continue;
    } else {
      r = gmx_math_unary(v, what, tab);  // 0 .. 2, and 5 .. 10: the LSTM's functions
    }
    uint32_t rb = gmx_f2u(r);
    if (r != r) rb = 0x7fc00000u;  // all NaNs alike
    x ^= (unsigned long long)rb * 0x9E3779B97F4A7C15ull + u;
    sacc += rb;
  }
  atomicXor(&out[0], x);
  atomicAdd(&out[1], sacc);
}

extern "C" hipError_t gmx_launch_math_probe(const float* x, float* y, uint64_t n, int what,
                                            hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     x, y, n, what);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_math_range(uint64_t lo, uint64_t count, int what,
                                            unsigned long long* out, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_math_range_kernel, dim3(2048), dim3(256), 0, stream, lo, count, what, out);
  return hipGetLastError();
}

// Constructed state of every Mixer: steps_ = 0, max_steps_ = 1, contexts_seen_ = 0
// (mixer.cpp:8-9, mixer.h:38); the tables themselves are zero-filled by the host side.
__global__ void gmx_init_scal_kernel(uint8_t* banks, uint64_t bank_bytes, uint64_t scal_off, int m,
                                     int n_streams) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m * n_streams) return;
  const int s = i / m, j = i % m;
  uint64_t* sc = (uint64_t*)(banks + (uint64_t)s * bank_bytes + scal_off) + 3 * j;
  sc[0] = 0;
  sc[1] = 1;
  sc[2] = 0;
}

extern "C" hipError_t gmx_launch_init_scal(uint8_t* banks, uint64_t bank_bytes, uint64_t scal_off,
                                           int m, int n_streams, hipStream_t stream) {
  const int n = m * n_streams;
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_init_scal_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, banks,
                     bank_bytes, scal_off, m, n_streams);
  return hipGetLastError();
}

// ---- the bit-count factor of the learning-rate decay, for many different bit counts ---------
// float(0.9 / pow(1e-7 * steps_ + 0.8, 0.8)) (mixer.cpp:111) is a function of the bit count only;
// streams that stand at the same count share one table row, which the host fills with the libm the
// reference calls.  When a launch covers streams at MANY different counts that loop would dwarf
// the kernel, so the table is made here -- and stays the reference's, bit for bit, without
// restating glibc's pow: the value needed is a FLOAT.  This device's pow and glibc's both lie
// within a few ulp (of double) of the true value; if every double within 64 ulp of ours rounds to
// the same float, that float is glibc's too.  The rare entry where it does not (a double within
// 2^-46 of a float rounding boundary: about one in 2^22) is reported and the host computes it.
struct GmxDecayArgs {
  const uint64_t* steps0;  // [U] bit count of row u at t = 0
  float* table;            // [U][T]
  uint32_t* amb;           // [0]: count of unsettled entries, [1 .. cap]: their flat indices
  uint32_t amb_cap, U;
  uint64_t T;
};

__global__ void __launch_bounds__(256) gmx_decay_kernel(const GmxDecayArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= (uint64_t)a.U * a.T) return;
  const uint64_t steps = a.steps0[i / a.T] + i % a.T;
  const double x = 0.0000001 * (double)steps + 0.8;
  const double d = 0.9 / pow(x, 0.8);
  const double margin = d * 0x1p-46;
  const float f = (float)d, lo = (float)(d - margin), hi = (float)(d + margin);
  a.table[i] = f;
  if (lo != hi) {
    const uint32_t k = atomicAdd(&a.amb[0], 1u);
    if (k < a.amb_cap) a.amb[1 + k] = (uint32_t)i;
  }
}

extern "C" hipError_t gmx_launch_decay_kernel(const GmxDecayArgs* args, hipStream_t stream) {
  (void)hipGetLastError();
  const uint64_t n = (uint64_t)args->U * args->T;
  hipLaunchKernelGGL(gmx_decay_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *args);
  return hipGetLastError();
}


// ---------------------------------------------------------------------------------------
// 16-byte words from one place to another -- the lock-step chain's record upload (gmx_chainstep.inc): pinned host
// memory, read across the link by the device itself, to device memory.  A kernel node instead of a memcpy node in
// the step's hipGraph: the graph's copies of 50-200 KB cost 9-11 us each, this one 2-4.
__global__ void __launch_bounds__(256) gmx_copy16_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, uint64_t n16) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}
// The head of a lock-step step as a launch of its own (chains whose first kernel is not the Indirect models'): block s
// brings stream s's inputs in.
__global__ void __launch_bounds__(64) gmx_step_upload_kernel(const GmxStepUpload u) {
  gmx_step_upload(u, (int)blockIdx.x, (int)threadIdx.x);
}
extern "C" hipError_t gmx_launch_step_upload(const GmxStepUpload* u, int n_streams, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_step_upload_kernel, dim3(n_streams), dim3(64), 0, stream, *u);
  return hipGetLastError();
}
extern "C" hipError_t gmx_launch_copy16(void* dst, const void* src, uint64_t n16, hipStream_t stream) {
  (void)hipGetLastError();
  if (n16 == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((n16 + 255) / 256 < 256 ? (n16 + 255) / 256 : 256);
  hipLaunchKernelGGL(gmx_copy16_kernel, dim3(blocks), dim3(256), 0, stream, (uint4*)dst, (const uint4*)src, n16);
  return hipGetLastError();
}
