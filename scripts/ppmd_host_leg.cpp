// ppmd_host_leg.cpp -- leg A of scripts/bench_ppmd.py: gmix_amd/csrc/gmx_ppmd.h built for the host (the restatement,
// NOT the reference's own build) over S streams on `threads` threads, a model and an arena per stream, as batch
// records.  Returns the wall time of the records alone in nanoseconds; models are made before the clock starts.
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "gmx_ppmd.h"

extern "C" double gmx_host_leg_ppmd(const uint8_t* bytes, uint64_t S, uint64_t n, int order, int arena_mb, int threads,
                                    float* last_ppm /* [S][256] */) {
  const uint64_t arena = (uint64_t)arena_mb << 20;
  std::vector<GmxPpmdState*> st(S);
  std::vector<uint8_t*> heap(S);
  for (uint64_t s = 0; s < S; ++s) {
    st[s] = (GmxPpmdState*)calloc(1, sizeof(GmxPpmdState));
    heap[s] = (uint8_t*)calloc(arena, 1);
    if (!st[s] || !heap[s]) return -1.0;
    gmx_ppmd_init(st[s], heap[s], order, arena);
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t]() {
      for (uint64_t s = (uint64_t)t; s < S; s += (uint64_t)threads)
        for (uint64_t i = 0; i < n; ++i) gmx_ppmd_record(st[s], heap[s], bytes[s * n + i], last_ppm + 256 * s);
    });
  for (auto& th : pool) th.join();
  const auto t1 = std::chrono::steady_clock::now();
  for (uint64_t s = 0; s < S; ++s) {
    free(st[s]);
    free(heap[s]);
  }
  return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
}
