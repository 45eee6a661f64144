// encoder_host_leg.cpp -- leg A of scripts/bench_encoder.py: gmx_encoder_bit of gmix_amd/csrc/gmx_encoder.h over
// p [S][pitch], bits [S][pitch] on n_threads host threads, streams dealt out in contiguous shares.  Returns the bytes
// produced (flushes included); out_ns receives the wall time.
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>

#include "gmx_encoder.h"

extern "C" uint64_t gmx_host_leg_encode(const float* p, const uint8_t* bits, uint64_t S, uint64_t pitch, uint64_t n_bits,
                                        int n_threads, uint8_t* scratch /* [S][4 * n_bits + 5] */, double* out_ns) {
  std::vector<uint64_t> produced((size_t)n_threads, 0);
  const auto t0 = std::chrono::steady_clock::now();
  auto work = [&](int k) {
    const uint64_t lo = S * (uint64_t)k / (uint64_t)n_threads, hi = S * (uint64_t)(k + 1) / (uint64_t)n_threads;
    uint64_t total = 0;
    for (uint64_t s = lo; s < hi; ++s) {
      GmxEncoderState st = {0u, 0xffffffffu};
      uint8_t* out = scratch + s * (4 * n_bits + 5);
      const float* ps = p + s * pitch;
      const uint8_t* bs = bits + s * pitch;
      for (uint64_t t = 0; t < n_bits; ++t) out += gmx_encoder_bit(&st, bs[t], ps[t], out);
      out += gmx_encoder_flush(&st, out);
      total += (uint64_t)(out - (scratch + s * (4 * n_bits + 5)));
    }
    produced[(size_t)k] = total;
  };
  if (n_threads == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (int k = 0; k < n_threads; ++k) th.emplace_back(work, k);
    for (auto& t : th) t.join();
  }
  *out_ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
  uint64_t sum = 0;
  for (uint64_t v : produced) sum += v;
  return sum;
}
