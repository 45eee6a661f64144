// ref_analysis_harness.cpp -- the reference's own Predictor with analysis on (predictor.cpp: Predict, RunAnalysis,
// UpdateEntropy), compiled against the reference where it lies.  Built and run by tests/golden/make_analysis_golden.py
// (build container only), in a temporary directory because EnableAnalysis creates analysis/ where it runs; the fixture
// it writes holds inputs and recorded results.
//
//   ref_analysis_harness trace <input file> <n_bytes> <all columns 0|1> <out file>
//     One stock Predictor over the file's first bytes as runner_utils::Compress drives it.  Header: n, M, C, the C
//     analysed indexes (uint32) and their descriptions (uint32 length, characters).  Per bit: predictions[n] as the blackboard holds them (float), active[n] (uint8),
//     the M gate contexts (uint32), the M mixer outputs (float), p (float), the bit (uint8), bits_seen at Perceive
//     (uint64) and entropy[] of the C analysed columns after Perceive (raw doubles).
//   ref_analysis_harness operands <in file> <out file>
//     in: records {float x; uint32 bit}.  Per record UpdateEntropy(bit, .) on the blackboard value x from the start
//     values 0 and -1, and as the next step of a running chain: three raw doubles.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#define private public  // UpdateEntropy and the memories are private in the reference
#include "mixer/mixer.h"
#include "predictor.h"
#undef private

template <typename T>
static void Put(std::ofstream& f, const T& v) {
  f.write(reinterpret_cast<const char*>(&v), sizeof(v));
}

static int Trace(const char* input, uint64_t n_bytes, bool all, const char* out) {
  std::ifstream is(input, std::ios::binary);
  if (!is.is_open()) return 1;
  std::vector<unsigned char> text(n_bytes);
  is.read(reinterpret_cast<char*>(text.data()), n_bytes);
  if ((uint64_t)is.gcount() != n_bytes) return 1;
  srand(0xDEADBEEF);  // runner.cpp:37
  Predictor p;
  ShortTermMemory& stm = p.short_term_memory_;
  if (all)
    for (size_t i = 0; i < stm.model_enable_analysis.size(); ++i) stm.model_enable_analysis[i] = true;
  p.EnableAnalysis(1 << 30);  // (no row of entropy.tsv: the averages are read from the memory)
  std::vector<Mixer*> mixers;
  for (auto& m : p.models_)
    if (Mixer* mx = dynamic_cast<Mixer*>(m.get())) mixers.push_back(mx);
  const uint32_t n = stm.num_predictions, M = mixers.size();
  std::vector<uint32_t> cols;
  for (size_t i = 0; i < stm.model_enable_analysis.size(); ++i)
    if (stm.model_enable_analysis[i]) cols.push_back((uint32_t)i);
  if (stm.entropy.size() != stm.model_enable_analysis.size()) return 6;
  std::ofstream f(out, std::ios::binary);
  Put(f, n);
  Put(f, M);
  Put(f, (uint32_t)cols.size());
  for (uint32_t c : cols) Put(f, c);
  for (uint32_t c : cols) {  // ... and their names, as entropy.tsv's header line has them
    const std::string& d = stm.model_descriptions[c];
    Put(f, (uint32_t)d.size());
    f.write(d.data(), d.size());
  }
  std::vector<uint8_t> act(n);
  for (uint64_t pos = 0; pos < n_bytes; ++pos) {
    for (int j = 7; j >= 0; --j) {
      const int bit = (text[pos] >> j) & 1;
      const float prob = p.Predict();
      f.write(reinterpret_cast<const char*>(&stm.predictions[0]), 4 * n);
      memset(act.data(), 0, n);
      for (int i : stm.active_models) act[i] = 1;
      f.write(reinterpret_cast<const char*>(act.data()), n);
      for (Mixer* mx : mixers) Put(f, (uint32_t)mx->context_);
      for (int k = 0; k < stm.num_layer0_mixers; ++k) Put(f, (float)stm.mixer_layer0_outputs[k]);
      for (int k = 0; k < stm.num_layer1_mixers; ++k) Put(f, (float)stm.mixer_layer1_outputs[k]);
      Put(f, (float)stm.final_mixer_output);
      Put(f, prob);
      Put(f, (uint8_t)bit);
      Put(f, (uint64_t)stm.bits_seen);
      p.Perceive(bit);
      for (uint32_t c : cols) Put(f, (double)stm.entropy[c]);
      p.Learn();
    }
  }
  return f.good() ? 0 : 5;
}

static int Operands(const char* in, const char* out) {
  struct Rec {
    float x;
    uint32_t bit;
  };
  std::vector<Rec> recs;
  {
    std::ifstream f(in, std::ios::binary);
    Rec r;
    while (f.read(reinterpret_cast<char*>(&r), sizeof r)) recs.push_back(r);
  }
  srand(0xDEADBEEF);
  Predictor p;
  ShortTermMemory& stm = p.short_term_memory_;
  if (stm.num_predictions < 2) return 6;
  std::ofstream f(out, std::ios::binary);
  stm.entropy[1] = 0;
  for (const Rec& r : recs) {
    stm.predictions[0] = r.x;
    stm.predictions[1] = r.x;
    for (double start : {0.0, -1.0}) {
      stm.entropy[0] = start;
      p.UpdateEntropy((int)r.bit, 0);
      Put(f, (double)stm.entropy[0]);
    }
    p.UpdateEntropy((int)r.bit, 1);
    Put(f, (double)stm.entropy[1]);
  }
  return f.good() ? 0 : 5;
}

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "trace")) return Trace(argv[2], strtoull(argv[3], 0, 0), atoi(argv[4]) != 0, argv[5]);
  if (argc == 4 && !strcmp(argv[1], "operands")) return Operands(argv[2], argv[3]);
  fprintf(stderr, "usage: %s trace <input> <n_bytes> <all 0|1> <out> | operands <in> <out>\n", argv[0]);
  return 2;
}
