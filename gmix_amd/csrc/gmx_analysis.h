// gmx_analysis.h -- the reference's analysis averages (predictor.cpp:439-469, UpdateEntropy) as pure functions for host
// and device alike (GMX_HD, as gmx_math.h, whose Logistic they share).  No HIP in here: tests/cpp/analysis_check.cpp
// builds it for the host, gmx_analysis.hip runs it, scripts/analysis_host_leg.cpp times it on host threads.
//
// UpdateEntropy keeps, per analysed model or mixer, a double exponential average of a FLOAT: log2 of the float
// probability resolves to the float overload, log2f.  Nothing here may be contracted beyond the gmx_fma()s spelled out
// (the library's -ffp-contract=off): gmx_analysis_step is two rounded multiplies and one rounded add.
#ifndef GMX_ANALYSIS_H_
#define GMX_ANALYSIS_H_

#include "gmx_math.h"

// log2f: glibc >= 2.28 (sysdeps/ieee754/flt-32/e_log2f.c, Arm Optimized Routines).  x = 2^k z with z in
// [0x1.66p-1, 0x1.66p0) split in 16 intervals exactly as gmx_logf splits it; r = z*invc - 1 from the published table of
// (1/c, log2 c) (log2f_data.c), a quartic in r, all in double, one final rounding.  The contractions are those of the
// FMA build, as in gmx_logf; tests/test_analysis_math.py compares it with the machine's log2f over every positive
// normal float.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__
#endif
static const double gmx_log2f_tab[16][2] = {  // {invc, logc}
    {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2}, {0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2},
    {0x1.49539f0f010bp+0, -0x1.7418b0a1fb77bp-2},  {0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2},
    {0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2}, {0x1.25e227b0b8eap+0, -0x1.97c1d1b3b7afp-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3}, {0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4},
    {0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4},  {0x1.ca4b31f026aap-1, 0x1.476a9543891bap-3},
    {0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2},
    {0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2},  {0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2}};

// (`tab` is gmx_log2f_tab or a copy of it)
GMX_HD float gmx_log2f_from(float x, const double (*tab)[2]) {
  const double kA0 = -0x1.712b6f70a7e4dp-2, kA1 = 0x1.ecabf496832ep-2, kA2 = -0x1.715479ffae3dep-1,
               kA3 = 0x1.715475f35c8b8p0;
  uint32_t ix = gmx_f2u(x);
  if (ix == 0x3f800000u) return 0.0f;
  if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
    if (ix * 2u == 0) return gmx_u2f(0xff800000u);                                  // log2(+-0) = -inf
    if (ix == 0x7f800000u) return x;                                                // log2(inf) = inf
    if ((ix & 0x80000000u) || ix * 2u >= 0xff000000u) return gmx_u2f(0x7fc00000u) + (x != x ? x : 0.0f);  // NaN
    ix = gmx_f2u(x * 0x1p23f);                                                      // subnormal: normalise
    ix -= 23u << 23;
  }
  const uint32_t tmp = ix - 0x3f330000u;
  const uint32_t i = (tmp >> 19) & 15u;
  const int32_t k = (int32_t)tmp >> 23;
  const uint32_t iz = ix - (tmp & 0xff800000u);
  const double invc = tab[i][0], logc = tab[i][1];
  const double z = (double)gmx_u2f(iz);
  const double r = gmx_fma(z, invc, -1.0);
  const double y0 = logc + (double)k;
  const double r2 = r * r;
  double y = gmx_fma(kA1, r, kA2);
  y = gmx_fma(kA0, r2, y);
  const double p = gmx_fma(kA3, r, y0);
  y = gmx_fma(y, r2, p);
  return (float)y;
}

GMX_HD float gmx_log2f(float x) { return gmx_log2f_from(x, gmx_log2f_tab); }

// UpdateEntropy behind its Logistic: the float clamp to [0.01f, 1 - 0.01f] and log2f of the coded bit's probability.
GMX_HD float gmx_analysis_entropy_of_prob_from(float prob, int bit, const double (*tab)[2]) {
  const float eps = 0.01f;
  if (prob < eps)
    prob = eps;
  else if (prob > 1 - eps)
    prob = 1 - eps;
  return gmx_log2f_from(bit ? prob : 1 - prob, tab);
}
GMX_HD float gmx_analysis_entropy_of_prob(float prob, int bit) {
  return gmx_analysis_entropy_of_prob_from(prob, bit, gmx_log2f_tab);
}

// ... and with it: `logit` is a blackboard value or a mixer's output.
GMX_HD float gmx_analysis_entropy(float logit, int bit) { return gmx_analysis_entropy_of_prob(gmx_logistic(logit), bit); }

// entropy[index] = (1 - alpha) * entropy[index] + alpha * entropy, in double.
GMX_HD double gmx_analysis_step(double e, float entropy) {
  const double alpha = 0.00001;
  const double keep = (1 - alpha) * e;
  const double add = alpha * (double)entropy;
  return keep + add;
}

#endif  // GMX_ANALYSIS_H_
