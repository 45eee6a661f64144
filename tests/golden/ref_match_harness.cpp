// ref_match_harness.cpp -- our own driver around the reference's Match models, for tests/golden/make_match_golden.py
// (build container only; the binary goes to oracle/_ref/).  It includes the reference's headers and links its
// translation units where they lie: a real ShortTermMemory and LongTermMemory, a real BasicContexts, real SkipContext
// objects (stock mode) and real Match objects, run in Predictor's order (predictor.cpp:17-28, :366-368, :383-387).
//
//   ref_match_harness <bytes.bin> <out.bin> stock
//   ref_match_harness <bytes.bin> <out.bin> ctx <contexts.bin> <limit> <table_size>...
//
// stock: the six models of Predictor::AddMatch over last_byte and the five hashes that Predictor::AddSkip's
// SkipContext objects compute.  ctx: K models over variables of ours, set from contexts.bin (u32 [n_bytes][K]) at every
// byte boundary between BasicContexts::Predict and the first Match::Predict.
//
// out.bin (little endian): u32 K, u64 T, then per bit {u32 ctx[K], u32 bit_context, u8 bit, float slot[K], u8
// active[K], u32 longest_match}, then u64 n + the `long` section, u64 n + the 11 K `short` bytes, u64 usage[K], and
// the coverage counters u64 {bytes kept out of the history, end-of-history resets, bits at match_length_ 255, the
// largest count, lookups that hit an entry written on the preceding bit}.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#define private public  // cur_match_ / match_length_ for the coverage counters
#include "models/match.h"
#undef private
#include "contexts/basic-contexts.h"
#include "contexts/skip-context.h"

template <typename T>
static void put(std::vector<uint8_t>& o, const T& v) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
  o.insert(o.end(), p, p + sizeof(T));
}

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::vector<uint8_t> data = slurp(argv[1]);
  const std::string out_path = argv[2], mode = argv[3];
  ShortTermMemory stm;
  LongTermMemory ltm;
  BasicContexts basic;
  std::vector<std::unique_ptr<Model>> skips;
  std::vector<std::unique_ptr<Match>> matches;
  std::vector<unsigned int*> vars;
  std::vector<unsigned int> own(8, 0);
  std::vector<uint32_t> ctx_file;
  if (mode == "stock") {
    skips.emplace_back(new SkipContext({0, 1}, stm.last_two_bytes_hash));
    skips.emplace_back(new SkipContext({0, 1, 2}, stm.last_three_bytes_hash));
    skips.emplace_back(new SkipContext({0, 1, 2, 3}, stm.last_four_bytes_hash));
    skips.emplace_back(new SkipContext({0, 1, 2, 3, 4}, stm.last_five_bytes_hash));
    skips.emplace_back(new SkipContext({0, 1, 2, 3, 4, 5}, stm.last_six_bytes_hash));
    const int limit = 400;
    vars = {&stm.last_byte,           &stm.last_two_bytes_hash,  &stm.last_three_bytes_hash,
            &stm.last_four_bytes_hash, &stm.last_five_bytes_hash, &stm.last_six_bytes_hash};
    const unsigned sizes[6] = {1u << 8, 1u << 16, 1u << 24, 1u << 21, 1u << 21, 1u << 21};
    for (int k = 0; k < 6; ++k) matches.emplace_back(new Match(stm, ltm, sizes[k], *vars[k], limit, "Match", false));
  } else {
    if (argc < 7) return 2;
    const std::vector<uint8_t> raw = slurp(argv[4]);
    ctx_file.resize(raw.size() / 4);
    memcpy(ctx_file.data(), raw.data(), ctx_file.size() * 4);
    const int limit = atoi(argv[5]);
    for (int i = 6; i < argc; ++i) {
      const int k = i - 6;
      vars.push_back(&own[k]);
      matches.emplace_back(new Match(stm, ltm, (unsigned)strtoul(argv[i], nullptr, 10), own[k], limit, "Match", false));
    }
  }
  const int K = (int)matches.size();
  stm.predictions.resize(stm.num_predictions);
  stm.predictions = 0;
  const uint64_t T = 8ull * data.size();
  std::vector<uint8_t> o;
  put(o, (uint32_t)K);
  put(o, T);
  uint64_t not_pushed = 0, eoh = 0, at255 = 0, same_entry = 0;
  std::vector<long long> wrote_bit(K, -2);
  std::vector<uint64_t> wrote_idx(K, 0);
  for (uint64_t t = 0; t < T; ++t) {
    const int bit = (data[t / 8] >> (7 - t % 8)) & 1;
    // ---- Predictor::Predict
    stm.active_models.clear();
    basic.Predict(stm, ltm);
    for (auto& s : skips) s->Predict(stm, ltm);
    if (stm.recent_bits == 1 && !ctx_file.empty())
      for (int k = 0; k < K; ++k) own[k] = ctx_file[(t / 8) * K + k];
    for (int k = 0; k < K; ++k) {
      Match& m = *matches[k];
      if (stm.recent_bits == 1) {  // what Match::Predict is about to decide (match.cpp:29-58), for the counters
        int ml = m.match_length_;
        ml = (stm.new_bit == ((m.cur_byte_ & m.bit_pos_) != 0)) ? std::min(ml + 1, 255) : 0;
        if (m.cur_match_ == ltm.history.size() - 1) {
          ++eoh;
          ml = 0;
        }
        const uint64_t idx = *vars[k] % ltm.match_memory[k].table.size();
        if (ml < 8 && wrote_bit[k] == (long long)t - 1 && wrote_idx[k] == idx) ++same_entry;
      }
      m.Predict(stm, ltm);
    }
    bool any255 = false;
    for (int k = 0; k < K; ++k) {
      put(o, (uint32_t)*vars[k]);
      any255 = any255 || matches[k]->match_length_ == 255;
    }
    at255 += any255;
    put(o, (uint32_t)stm.bit_context);
    put(o, (uint8_t)bit);
    for (int k = 0; k < K; ++k) put(o, (float)stm.predictions[matches[k]->prediction_index_]);
    for (int k = 0; k < K; ++k) {
      const int idx = matches[k]->prediction_index_;
      const bool act = std::find(stm.active_models.begin(), stm.active_models.end(), idx) != stm.active_models.end();
      put(o, (uint8_t)act);
    }
    put(o, (uint32_t)stm.longest_match);
    // ---- Predictor::Perceive, Predictor::Learn
    stm.new_bit = bit;
    const size_t before = ltm.history.size();
    basic.Learn(stm, ltm);
    for (auto& s : skips) s->Learn(stm, ltm);
    for (int k = 0; k < K; ++k) matches[k]->Learn(stm, ltm);
    if (stm.recent_bits >= 128) {
      if (ltm.history.size() == before) {
        ++not_pushed;
      } else {
        for (int k = 0; k < K; ++k) {
          wrote_bit[k] = (long long)t;
          wrote_idx[k] = *vars[k] % ltm.match_memory[k].table.size();
        }
      }
    }
  }
  const std::string tmp = out_path + ".tmp";
  {
    std::ofstream f(tmp, std::ios::binary);
    ltm.WriteToDisk(&f);
  }
  std::vector<uint8_t> sec = slurp(tmp);
  put(o, (uint64_t)sec.size());
  o.insert(o.end(), sec.begin(), sec.end());
  {
    std::ofstream f(tmp, std::ios::binary);
    for (auto& m : matches) m->WriteToDisk(&f);
  }
  sec = slurp(tmp);
  put(o, (uint64_t)sec.size());
  o.insert(o.end(), sec.begin(), sec.end());
  remove(tmp.c_str());
  for (auto& m : matches) put(o, (uint64_t)m->GetMemoryUsage(stm, ltm));
  int max_count = 0;
  for (auto& mm : ltm.match_memory) max_count = std::max(max_count, *std::max_element(mm.counts.begin(), mm.counts.end()));
  put(o, not_pushed);
  put(o, eoh);
  put(o, at255);
  put(o, (uint64_t)max_count);
  put(o, same_entry);
  std::ofstream f(out_path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(o.data()), (std::streamsize)o.size());
  return f.good() ? 0 : 1;
}
