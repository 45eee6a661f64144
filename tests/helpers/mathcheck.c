/* mathcheck.c -- test helper: the product's scalar math (gmix_amd/csrc/gmx_math.h, host
 * compile) against the machine's libm, which is what the reference links
 * (mixer/sigmoid.cpp:5).  Built by tests/test_math.py with gcc -O2 -ffp-contract=off -fopenmp. */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../gmix_amd/csrc/gmx_math.h"

/* Compare gmx_expf with libm expf for every float whose bit pattern lies in [lo, hi]
 * (NaN results compare equal when both are NaN).  Returns the mismatch count; the first
 * few offending bit patterns go to bad[0..nbad). */
uint64_t gmx_check_expf_range(uint64_t lo, uint64_t hi, uint32_t* bad, int nbad) {
  uint64_t mism = 0;
#pragma omp parallel for reduction(+ : mism) schedule(static)
  for (uint64_t u = lo; u <= hi; ++u) {
    float x = gmx_u2f((uint32_t)u);
    float a = gmx_expf(x), b = expf(x);
    int same = (gmx_f2u(a) == gmx_f2u(b)) || (a != a && b != b);
    if (!same) {
      uint64_t k;
#pragma omp atomic capture
      k = mism++;
      if ((int)k < nbad) bad[k] = (uint32_t)u;
    }
  }
  return mism;
}

/* Same for the whole squash: 1/(1+expf(-p)) against the libm form. */
uint64_t gmx_check_logistic_range(uint64_t lo, uint64_t hi, uint32_t* bad, int nbad) {
  uint64_t mism = 0;
#pragma omp parallel for reduction(+ : mism) schedule(static)
  for (uint64_t u = lo; u <= hi; ++u) {
    float x = gmx_u2f((uint32_t)u);
    float a = gmx_logistic(x), b = 1 / (1 + expf(-x));
    int same = (gmx_f2u(a) == gmx_f2u(b)) || (a != a && b != b);
    if (!same) {
      uint64_t k;
#pragma omp atomic capture
      k = mism++;
      if ((int)k < nbad) bad[k] = (uint32_t)u;
    }
  }
  return mism;
}

/* Sigmoid::Logit (mixer/sigmoid.cpp:7-13) on libm: double comparisons and clamps, float divide. */
static float libm_logit(float p) {
  if (p < 0.0001) p = 0.0001;
  else if (p > 0.9999) p = 0.9999;
  return logf(p / (1 - p));
}

void gmx_host_logistic_array(const float* x, float* y, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) y[i] = gmx_logistic(x[i]);
}
void gmx_host_squash_array(const float* x, float* y, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) y[i] = gmx_squash_clamp(x[i]);
}


/* The LSTM's functions against libm: logf, expm1f (the core of tanhf), tanhf. */
#define GMX_CHECK_RANGE(NAME, OURS, LIBM)                                              \
  uint64_t NAME(uint64_t lo, uint64_t hi, uint32_t* bad, int nbad) {                    \
    uint64_t mism = 0;                                                                  \
    _Pragma("omp parallel for reduction(+ : mism) schedule(static)")                    \
    for (uint64_t u = lo; u <= hi; ++u) {                                               \
      float x = gmx_u2f((uint32_t)u);                                                   \
      float a = OURS(x), b = LIBM(x);                                                   \
      int same = (gmx_f2u(a) == gmx_f2u(b)) || (a != a && b != b);                      \
      if (!same) {                                                                      \
        uint64_t k;                                                                     \
        _Pragma("omp atomic capture")                                                   \
        k = mism++;                                                                     \
        if ((int)k < nbad) bad[k] = (uint32_t)u;                                        \
      }                                                                                 \
    }                                                                                   \
    return mism;                                                                        \
  }
GMX_CHECK_RANGE(gmx_check_logf_range, gmx_logf, logf)
GMX_CHECK_RANGE(gmx_check_expm1f_range, gmx_expm1f, expm1f)
GMX_CHECK_RANGE(gmx_check_tanhf_range, gmx_tanhf, tanhf)
GMX_CHECK_RANGE(gmx_check_logit_range, gmx_logit, libm_logit)

/* ---- references for the device probes of the LSTM's math (tests/test_gpu_math.py): libm and the compiler's
 * correctly rounded divide / sqrtf alone, nothing of gmx_math.h ------------------------------------------ */
void gmx_libm_lstm_array(const float* x, float* y, uint64_t n, int what) {
#pragma omp parallel for schedule(static)
  for (uint64_t i = 0; i < n; ++i) {
    const float v = x[i];
    float r;
    switch (what) {
      case 5: r = logf(v); break;
      case 6: r = libm_logit(v); break;
      case 7: r = expm1f(v); break;
      case 8: r = tanhf(v); break;
      case 9: r = 1 / (1 + expf(-v)); break;
      default: r = 1.0f / sqrtf((v / 50.0f) + 1e-5f); break; /* 10: layer-norm scale, 50 cells */
    }
    y[i] = r;
  }
}

/* Adam's scalars of step t as the library's host side makes them for the kernel (gmx_lstm.inc, lstm_stage_rows;
 * lstm-layer.cpp:15-21, :27-32): row = {alpha, 1 - beta1^t, 1 - beta2^t}. */
static void adam_row(unsigned t, float row[3]) {
  const float beta1 = 0.025, beta2 = 0.9999, learning_rate = 0.03f;
  const unsigned long long limit = 3000;
  const float tf = (float)t;
  if (tf < limit) {
    row[0] = learning_rate * 0.1f / sqrtf(5e-5f * tf + 1.0f);
    row[1] = (float)(1.0f - powf(beta1, tf));
    row[2] = (float)(1.0f - powf(beta2, tf));
  } else {
    row[0] = learning_rate * 0.1f / sqrtf(5e-5f * limit + 1.0f);
    row[1] = (float)(1.0f - powf(beta1, limit));
    row[2] = (float)(1.0f - powf(beta2, limit));
  }
}

static uint64_t mix64(uint64_t h) {
  h *= 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  h *= 0x94D049BB133111EBull;
  h ^= h >> 31;
  return h;
}
static float f_of(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

/* Operand tuples (weight, alpha, m, d1, v, d2) number lo .. lo + n - 1 of Adam's step, six floats each.
 * The first GMX_ADAM_GRID tuples are a grid -- every step count t = 1 .. 3000 x second moments from 0 through the
 * subnormals to 1e30 x first moments of both signs x a few weights --, the rest are hashed: t uniform in 1 .. 3000,
 * v and |m| with exponents spread over the whole range of finite non-negative floats (v) / finite floats (m),
 * the weight a float of magnitude below 4. */
static const uint32_t kAdamV[] = {0x00000000u, 0x00000001u, 0x00000002u, 0x00400000u, 0x007fffffu, 0x00800000u, 0x00800001u,
                                  0x0da24260u /* 1e-30 */, 0x2b8cbccc /* 1e-12 */, 0x358637bd /* 1e-6 */,
                                  0x3a83126f /* 1e-3 */, 0x3f800000u, 0x501502f9 /* 1e10 */, 0x60ad78ec /* 1e20 */,
                                  0x7149f2ca /* 1e30 */};
static const uint32_t kAdamM[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x807fffffu, 0x00800000u, 0x8da24260u, 0x2b8cbccc,
                                  0xba83126f, 0x3f800000u, 0xc1200000u /* -10 */, 0x501502f9, 0xe0ad78ec};
static const uint32_t kAdamW[] = {0x00000000u, 0x3dcccccdu /* 0.1 */, 0xbf800000u, 0x00000001u};
enum { NV = sizeof kAdamV / 4, NM = sizeof kAdamM / 4, NW = sizeof kAdamW / 4 };
uint64_t gmx_adam_grid_size(void) { return (uint64_t)3000 * NV * NM * NW; }

void gmx_adam_tuples(uint64_t lo, uint64_t n, float* x) {
  static float rows[3001][3];
  for (unsigned t = 1; t <= 3000; ++t) adam_row(t, rows[t]);
  const uint64_t grid = gmx_adam_grid_size();
#pragma omp parallel for schedule(static)
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = lo + k;
    float* o = x + 6 * k;
    unsigned t;
    if (i < grid) {
      uint64_t r = i;
      o[0] = f_of(kAdamW[r % NW]); r /= NW;
      o[2] = f_of(kAdamM[r % NM]); r /= NM;
      o[4] = f_of(kAdamV[r % NV]); r /= NV;
      t = 1 + (unsigned)r;
    } else {
      const uint64_t h = mix64(i), h2 = mix64(i ^ 0x5555555555555555ull);
      t = 1 + (unsigned)(h % 3000u);
      o[4] = f_of((uint32_t)(h >> 32) % 0x7f800000u);                         /* v: any finite float >= 0 */
      o[2] = f_of(((uint32_t)h2 % 0x7f800000u) | ((uint32_t)(h2 >> 63) << 31)); /* m: any finite float */
      o[0] = f_of(((uint32_t)(h2 >> 32) % 0x40800000u) | ((uint32_t)(h2 >> 62) << 31 & 0x80000000u));
    }
    o[1] = rows[t][0];
    o[3] = rows[t][1];
    o[5] = rows[t][2];
  }
}

/* the reference of the probe's what = 11: y[6j] from x[6j .. 6j + 5], 0 elsewhere */
void gmx_libm_adam_array(const float* x, float* y, uint64_t n_tuples) {
#pragma omp parallel for schedule(static)
  for (uint64_t j = 0; j < n_tuples; ++j) {
    const float* o = x + 6 * j;
    const float eps = 1e-6f;
    y[6 * j] = o[0] - o[1] * ((o[2] / o[3]) / (sqrtf(o[4] / o[5] + eps)));
    for (int k = 1; k < 6; ++k) y[6 * j + k] = 0.0f;
  }
}
