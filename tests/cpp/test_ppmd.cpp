// test_ppmd.cpp -- gmix_amd/csrc/gmx_ppmd.h built for the host (strict floats: -ffp-contract=off).  Two uses:
//   - as a shared library (tests/ppmd_common.py: HostModel), the checker of the CPU tests against the reference's
//     recorded fixture and of the GPU tests against the kernel; with -DGMX_PPMD_CENSUS it counts the model's branches;
//   - as a stand-alone program, which the CPU test also builds with -fsanitize=address,undefined:
//       test_ppmd <bytes.bin> <order> <arena MB> <expect.bin>
//     expect.bin holds per byte {uint64 used, uint64 running hash}; every one must match.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "gmx_coder.h"
#include "gmx_ppmd.h"

struct Host {
  GmxPpmdState st;
  uint8_t* arena = nullptr;
  uint64_t hash = 14695981039346656037ull;
};

extern "C" {

Host* ppmd_host_create(int order, int arena_mb) {
  if (order < GMX_PPMD_MIN_ORDER || order > GMX_PPMD_MAX_ORDER || arena_mb < 1 || arena_mb > GMX_PPMD_MAX_ARENA_MB)
    return nullptr;
  Host* h = new Host();
  memset(&h->st, 0, sizeof h->st);
  const uint64_t bytes = (uint64_t)arena_mb << 20;
  h->arena = (uint8_t*)calloc(bytes, 1);
  if (!h->arena) {
    delete h;
    return nullptr;
  }
  gmx_ppmd_init(&h->st, h->arena, order, bytes);
  return h;
}

void ppmd_host_destroy(Host* h) {
  if (!h) return;
  free(h->arena);
  delete h;
}

// n bytes.  records == 0: every byte is the byte coded LAST (ModPPMD::Predict at a byte boundary, the bank's per-byte
// surface); pred holds the model's slot at bit 0 alone.  records != 0: the bank's batch records (gmx_ppmd_record), pred
// and active the walk along the record's own byte.  Out: ppm [n][256] bit patterns (or NULL), pred [n][8] and
// active [n][8], 16 + used memory, and the running FNV-1a over all ppm bytes.
void ppmd_host_run(Host* h, const uint8_t* d, uint64_t n, int records, uint32_t* ppm, uint32_t* pred, uint8_t* active,
                   uint64_t* used, uint64_t* hash) {
  float row[256];
  for (uint64_t i = 0; i < n; ++i) {
    if (records)
      gmx_ppmd_record(&h->st, h->arena, d[i], row);
    else
      gmx_ppmd_byte(&h->st, h->arena, d[i], row);
    if (ppm) memcpy(ppm + 256 * i, row, 1024);
    const uint8_t* b = (const uint8_t*)row;
    for (int k = 0; k < 1024; ++k) h->hash = (h->hash ^ b[k]) * 1099511628211ull;
    if (hash) hash[i] = h->hash;
    if (used) used[i] = 16 + gmx_ppmd_used_memory(&h->st);
    if (pred) {
      GmxCoderWalk w;
      gmx_coder_walk_open(&w);
      for (int j = 0; j < (records ? 8 : 1); ++j) {
        float slot = 0.0f;
        bool act = false;
        if (j) gmx_coder_walk_bit(&w, (d[i] >> (8 - j)) & 1u);
        gmx_coder_walk_predict(&w, row, &slot, &act);
        memcpy(pred + 8 * i + j, &slot, 4);
        active[8 * i + j] = act ? 1 : 0;
      }
      for (int j = records ? 8 : 1; j < 8; ++j) {
        pred[8 * i + j] = 0;
        active[8 * i + j] = 0;
      }
    }
  }
}

uint32_t ppmd_host_restores(Host* h) { return h->st.restores; }
uint64_t ppmd_host_memory_usage(Host* h) { return 16 + gmx_ppmd_used_memory(&h->st); }

int ppmd_host_census(uint64_t* c, uint64_t* ns) {
#if defined(GMX_PPMD_CENSUS)
  memcpy(c, gmx_ppmd_census, sizeof gmx_ppmd_census);
  memcpy(ns, gmx_ppmd_census_ns, sizeof gmx_ppmd_census_ns);
  return GMX_PC_COUNT;
#else
  (void)c;
  (void)ns;
  return 0;
#endif
}

}  // extern "C"

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s bytes.bin order arena_mb expect.bin\n", argv[0]);
    return 2;
  }
  std::vector<uint8_t> d;
  std::vector<uint64_t> e;
  {
    std::ifstream f(argv[1], std::ios::binary);
    d.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    std::ifstream g(argv[4], std::ios::binary);
    uint64_t v;
    while (g.read(reinterpret_cast<char*>(&v), 8)) e.push_back(v);
  }
  if (d.empty() || e.size() != 2 * d.size()) {
    fprintf(stderr, "%zu bytes, %zu expectations\n", d.size(), e.size());
    return 3;
  }
  Host* h = ppmd_host_create(atoi(argv[2]), atoi(argv[3]));
  if (!h) return 4;
  std::vector<uint64_t> used(d.size()), hash(d.size());
  ppmd_host_run(h, d.data(), d.size(), 0, nullptr, nullptr, nullptr, used.data(), hash.data());
  for (size_t i = 0; i < d.size(); ++i)
    if (used[i] != e[2 * i] || hash[i] != e[2 * i + 1]) {
      printf("FAIL: byte %zu used %llu (expected %llu) hash %016llx (expected %016llx)\n", i, (unsigned long long)used[i],
             (unsigned long long)e[2 * i], (unsigned long long)hash[i], (unsigned long long)e[2 * i + 1]);
      return 1;
    }
  printf("ok: %zu bytes, %u restores\n", d.size(), ppmd_host_restores(h));
  ppmd_host_destroy(h);
  return 0;
}
