/* rangecheck.c -- host twin of gmx_math_range_kernel (gmix_amd/csrc/gmx_kernels.hip): folds
 * gmx_expf / gmx_logistic / gmx_squash_clamp (what = 0 .. 2) and the LSTM's functions (what = 5 .. 10) over a range
 * of float bit patterns into {xor-fold, sum} so that device and host can be compared over all 2^32 inputs. */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../gmix_amd/csrc/gmx_math.h"

/* what = 5 .. 10, the LSTM byte model's functions: the reference here is the machine's libm and the compiler's
 * correctly rounded divide and sqrtf, never gmx_math.h (that is the code under test on the device). */
static float libm_logit(float p) { /* Sigmoid::Logit: double comparisons and clamps, float divide */
  if (p < 0.0001) p = 0.0001;
  else if (p > 0.9999) p = 0.9999;
  return logf(p / (1 - p));
}
static float libm_lstm_unary(float v, int what) {
  switch (what) {
    case 5: return logf(v);
    case 6: return libm_logit(v);
    case 7: return expm1f(v);
    case 8: return tanhf(v);
    case 9: return 1 / (1 + expf(-v));
    default: return 1.0f / sqrtf((v / 50.0f) + 1e-5f); /* 10: the layer-norm scale over 50 cells */
  }
}

void gmx_host_math_range(uint64_t lo, uint64_t count, int what, unsigned long long out[2]) {
  unsigned long long x = 0, s = 0;
#pragma omp parallel for reduction(^ : x) reduction(+ : s) schedule(static)
  for (uint64_t i = 0; i < count; ++i) {
    const uint32_t u = (uint32_t)(lo + i);
    float v, r;
    memcpy(&v, &u, 4);
    if (what >= 5) r = libm_lstm_unary(v, what);
    else r = what == 0 ? gmx_expf(v) : (what == 1 ? gmx_logistic(v) : gmx_squash_clamp(v));
    uint32_t rb;
    memcpy(&rb, &r, 4);
    if (r != r) rb = 0x7fc00000u;
    x ^= (unsigned long long)rb * 0x9E3779B97F4A7C15ull + u;
    s += rb;
  }
  out[0] = x;
  out[1] = s;
}
