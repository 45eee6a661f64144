// ref_ppmd_harness.cpp -- the reference's own ModPPMD (models/mod_ppmd.cpp, compiled where it lies) driven through
// Model's interface: recent_bits = 1, last_byte = d[i], Predict.  Built and run by tests/golden/make_ppmd_golden.py
// (build container only); the fixture it writes holds recorded results only.
//
//   ref_ppmd_harness <bytes.bin> <order> <arena MB> <out.bin>
//
// out.bin: per input byte one record {uint32 ppm[256] (bit patterns of ppm_predictions), uint32 slot (the model's logit
// at bit 0), uint32 0, uint64 GetMemoryUsage, uint64 running FNV-1a over the ppm bytes so far}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "memory/long-term-memory.h"
#include "memory/short-term-memory.h"
#include "models/mod_ppmd.h"

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s bytes.bin order arena_mb out.bin\n", argv[0]);
    return 2;
  }
  std::vector<unsigned char> d;
  {
    std::ifstream f(argv[1], std::ios::binary);
    d.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  }
  ShortTermMemory* stm = new ShortTermMemory();
  LongTermMemory* ltm = new LongTermMemory();
  // never deleted: the model's class is private to its translation unit
  PPMD::ModPPMD* m = new PPMD::ModPPMD(*stm, *ltm, atoi(argv[2]), atoi(argv[3]), false);
  stm->predictions.resize(stm->num_predictions, 0.0f);
  std::ofstream out(argv[4], std::ios::binary);
  uint64_t h = 14695981039346656037ull;
  for (size_t i = 0; i < d.size(); ++i) {
    stm->recent_bits = 1;
    stm->last_byte = d[i];
    stm->active_models.clear();
    m->Predict(*stm, *ltm);
    uint32_t rec[262];
    for (int c = 0; c < 256; ++c) {
      const float v = stm->ppm_predictions[c];
      memcpy(&rec[c], &v, 4);
    }
    const unsigned char* b = reinterpret_cast<const unsigned char*>(rec);
    for (int k = 0; k < 1024; ++k) h = (h ^ b[k]) * 1099511628211ull;
    const float slot = stm->predictions[0];
    memcpy(&rec[256], &slot, 4);
    rec[257] = 0;
    const uint64_t used = m->GetMemoryUsage(*stm, *ltm);
    memcpy(&rec[258], &used, 8);
    memcpy(&rec[260], &h, 8);
    out.write(reinterpret_cast<const char*>(rec), sizeof rec);
  }
  return out.good() ? 0 : 5;
}
