// analysis_check.cpp -- gmix_amd/csrc/gmx_analysis.h built for the host, as a small shared library the analysis tests
// load (tests/analysis_common.py): the functions themselves, sweeps of them against this machine's libm, the clamp
// thresholds by bisection, and the checker of the device object -- the per-stream walk of DESIGN.md section 4.23 in plain
// C++ on the header's functions.  Strict floats: built with -ffp-contract=off.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "gmx_analysis.h"

static bool same_f(float a, float b) { return gmx_f2u(a) == gmx_f2u(b) || (a != a && b != b); }

// UpdateEntropy's arithmetic behind the Logistic, spelled out with libm (gmx::BatchedCompressor::AverageOfProb)
static float libm_entropy_of_prob(float prob, int bit) {
  float eps = 0.01;
  if (prob < eps)
    prob = eps;
  else if (prob > 1 - eps)
    prob = 1 - eps;
  float entropy;
  if (bit)
    entropy = log2f(prob);
  else
    entropy = log2f(1 - prob);
  return entropy;
}

template <class F>
static uint64_t sweep(uint32_t lo, uint32_t hi, int threads, uint32_t* first_bad, F bad) {
  std::atomic<uint64_t> n_bad{0};
  std::atomic<uint32_t> first{0xffffffffu};
  std::vector<std::thread> pool;
  const uint64_t span = ((uint64_t)hi - lo + threads - 1) / threads;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t] {
      const uint64_t a = lo + span * t, b = a + span < hi ? a + span : hi;
      uint64_t mine = 0;
      uint32_t mine_first = 0xffffffffu;
      for (uint64_t u = a; u < b; ++u)
        if (bad((uint32_t)u)) {
          if (!mine++) mine_first = (uint32_t)u;
        }
      n_bad += mine;
      uint32_t cur = first.load();
      while (mine_first < cur && !first.compare_exchange_weak(cur, mine_first)) {
      }
    });
  for (auto& th : pool) th.join();
  if (first_bad) *first_bad = first.load();
  return n_bad.load();
}

extern "C" {

float an_log2f(float x) { return gmx_log2f(x); }
float an_entropy(float logit, int bit) { return gmx_analysis_entropy(logit, bit); }
float an_entropy_of_prob(float prob, int bit) { return gmx_analysis_entropy_of_prob(prob, bit); }
double an_step(double e, float entropy) { return gmx_analysis_step(e, entropy); }
float an_logistic(float x) { return gmx_logistic(x); }

// gmx_log2f against libm's log2f on the floats of the bit patterns [lo, hi): the count of mismatches
uint64_t an_sweep_log2f(uint32_t lo, uint32_t hi, int threads, uint32_t* first_bad) {
  return sweep(lo, hi, threads, first_bad, [](uint32_t u) {
    const float x = gmx_u2f(u);
    return !same_f(gmx_log2f(x), log2f(x));
  });
}
// gmx_analysis_entropy_of_prob against the libm spelling, both bits
uint64_t an_sweep_prob(uint32_t lo, uint32_t hi, int threads, uint32_t* first_bad) {
  return sweep(lo, hi, threads, first_bad, [](uint32_t u) {
    const float x = gmx_u2f(u);
    return !same_f(gmx_analysis_entropy_of_prob(x, 0), libm_entropy_of_prob(x, 0)) ||
           !same_f(gmx_analysis_entropy_of_prob(x, 1), libm_entropy_of_prob(x, 1));
  });
}

// Where Logistic(x) crosses the clamps: out = {the last x below 0.01f, the first x not below, the last x not above
// 1 - 0.01f, the first x above}.
void an_thresholds(float out[4]) {
  const float eps = 0.01f;
  float a = -8.0f, b = 0.0f;  // Logistic(a) < eps <= Logistic(b)
  while (nextafterf(a, b) != b) {
    const float m = 0.5f * a + 0.5f * b;
    (gmx_logistic(m) < eps ? a : b) = m;
  }
  out[0] = a;
  out[1] = b;
  a = 0.0f, b = 8.0f;  // Logistic(a) <= 1 - eps < Logistic(b)
  while (nextafterf(a, b) != b) {
    const float m = 0.5f * a + 0.5f * b;
    (gmx_logistic(m) > 1 - eps ? b : a) = m;
  }
  out[2] = a;
  out[3] = b;
}

// One stream's walk: per bit update every column, capture at bits_seen > 0 && bits_seen % F == 0, ++bits_seen.
// values [n][C]: a logit per column, a probability where is_prob[c].  trail (or NULL) [n][C]: the averages after every
// bit.  Returns the rows captured (at most max_rows are stored).
uint64_t an_run(double* ema, uint64_t* bits_seen, uint64_t F, const float* values, const uint8_t* is_prob,
                const uint8_t* bits, uint64_t n, uint32_t C, double* rows, uint64_t* labels, uint64_t max_rows,
                double* trail) {
  uint64_t n_rows = 0;
  for (uint64_t t = 0; t < n; ++t) {
    const int bit = bits[t] ? 1 : 0;
    for (uint32_t c = 0; c < C; ++c) {
      const float v = values[t * C + c];
      const float e = is_prob[c] ? gmx_analysis_entropy_of_prob(v, bit) : gmx_analysis_entropy(v, bit);
      ema[c] = gmx_analysis_step(ema[c], e);
    }
    if (trail) memcpy(trail + t * C, ema, (size_t)C * 8);
    if (F > 0 && *bits_seen > 0 && *bits_seen % F == 0) {
      if (n_rows < max_rows) {
        memcpy(rows + n_rows * C, ema, (size_t)C * 8);
        labels[n_rows] = *bits_seen;
      }
      ++n_rows;
    }
    ++*bits_seen;
  }
  return n_rows;
}
}
