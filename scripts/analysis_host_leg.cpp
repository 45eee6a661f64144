// analysis_host_leg.cpp -- leg A of scripts/bench_analysis.py: what gmx::BatchedCompressor::Drain does per bit with
// analysis on, gmx_analysis_entropy / gmx_analysis_step of gmix_amd/csrc/gmx_analysis.h over values [S][n_bits][C]
// (logits; the last column a probability) and bits [S][n_bits] on n_threads host threads, streams dealt out in
// contiguous shares.  ema [S][C] is updated in place; out_ns receives the wall time.
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>

#include "gmx_analysis.h"

extern "C" void gmx_host_leg_analysis(const float* values, const uint8_t* bits, uint64_t S, uint64_t n_bits, uint32_t C,
                                      int n_threads, double* ema, double* out_ns) {
  const auto t0 = std::chrono::steady_clock::now();
  auto work = [&](int k) {
    const uint64_t lo = S * (uint64_t)k / (uint64_t)n_threads, hi = S * (uint64_t)(k + 1) / (uint64_t)n_threads;
    for (uint64_t s = lo; s < hi; ++s) {
      double* e = ema + s * C;
      for (uint64_t t = 0; t < n_bits; ++t) {
        const float* v = values + (s * n_bits + t) * C;
        const int bit = bits[s * n_bits + t] ? 1 : 0;
        for (uint32_t c = 0; c + 1 < C; ++c) e[c] = gmx_analysis_step(e[c], gmx_analysis_entropy(v[c], bit));
        e[C - 1] = gmx_analysis_step(e[C - 1], gmx_analysis_entropy_of_prob(v[C - 1], bit));
      }
    }
  };
  if (n_threads == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (int k = 0; k < n_threads; ++k) th.emplace_back(work, k);
    for (auto& t : th) t.join();
  }
  *out_ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
}
