// ref_ctx_harness.cpp -- our own driver around the reference's context objects, for tests/golden/make_ctx_golden.py
// (build container only; the binary goes to oracle/_ref/).  It includes the reference's headers and links its
// translation units where they lie: a real ShortTermMemory and LongTermMemory, a real BasicContexts, and real
// IntervalContext, SkipContext and IndirectHash objects, run in Predictor's order (BasicContexts first,
// predictor.cpp:17-28, :366-368).
//
//   ref_ctx_harness <bytes.bin> <descs.bin> <out.bin> <position>...
//
// descs.bin: V records of gmx_ctx_desc (include/gmxmix.h), 292 bytes each.  RECENT_BYTE variables are
// ShortTermMemory::recent_bytes[i] (0: last_byte), BYTE_PLUS_RECENT 0 / 1 are last_byte_plus_recent /
// second_last_plus_recent, BIT_CONTEXT and ZERO bit_context and always_zero; every other variable is an unsigned int of
// ours that the object writes.  position: bits after which the checkpoint state is recorded (0: never run).
//
// out.bin (little endian): u32 V, u64 T, u32 values[T][V] (at Predict of every bit), u32 P, then per position {u64
// bits, u32 H, per hash variable u64 n + its WriteToDisk bytes, the blackboard as gmx_ctx_blackboard (1316 bytes)},
// and the coverage counters u64 {byte openings where IndirectHash's old and new index are one entry, wraps of
// rotating_history_pos}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#define private public  // outer_hash_ / table_ for the counters, first_prediction_ for the blackboard
#include "contexts/basic-contexts.h"
#include "contexts/indirect-hash.h"
#undef private
#include "contexts/interval-context.h"
#include "contexts/skip-context.h"

struct Desc {
  int32_t kind, index, num_bits, n_bytes, outer_order, inner_order;
  uint32_t table_size;
  uint8_t bytes_to_use[8];
  uint8_t map[256];
};
static_assert(sizeof(Desc) == 292, "gmx_ctx_desc");

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
  const std::vector<uint8_t> data = slurp(argv[1]), raw = slurp(argv[2]);
  const std::string out_path = argv[3];
  std::vector<uint64_t> positions;
  for (int i = 4; i < argc; ++i) positions.push_back(strtoull(argv[i], nullptr, 10));
  const int V = (int)(raw.size() / sizeof(Desc));
  if (V < 1 || V > 64 || raw.size() % sizeof(Desc)) return 2;
  std::vector<Desc> descs(V);
  memcpy(descs.data(), raw.data(), raw.size());

  ShortTermMemory stm;
  LongTermMemory ltm;
  BasicContexts basic;
  std::vector<unsigned int> own(V, 0);
  std::vector<unsigned int*> vars(V, nullptr);
  std::vector<std::unique_ptr<Model>> objs;
  std::vector<IndirectHash*> hashes;
  for (int v = 0; v < V; ++v) {
    const Desc& d = descs[v];
    vars[v] = &own[v];
    switch (d.kind) {
      case 0: vars[v] = &stm.always_zero; break;
      case 1: vars[v] = &stm.bit_context; break;
      case 2: vars[v] = d.index == 0 ? &stm.last_byte : &stm.recent_bytes[d.index]; break;
      case 3:
        if (d.index > 1) return 2;
        vars[v] = d.index == 0 ? &stm.last_byte_plus_recent : &stm.second_last_plus_recent;
        break;
      case 4: {
        std::vector<int> map(d.map, d.map + 256);
        objs.emplace_back(new IntervalContext(map, (unsigned)d.num_bits, own[v]));
        break;
      }
      case 5: {
        std::vector<int> use(d.bytes_to_use, d.bytes_to_use + d.n_bytes);
        objs.emplace_back(new SkipContext(use, own[v]));
        break;
      }
      case 6: {
        IndirectHash* h = new IndirectHash(d.outer_order, d.table_size, d.inner_order, own[v]);
        objs.emplace_back(h);
        hashes.push_back(h);
        break;
      }
      default: return 2;
    }
  }
  const uint64_t T = 8ull * data.size();
  std::vector<uint8_t> o, ck;
  put(o, (uint32_t)V);
  put(o, T);
  uint64_t same_entry = 0, wraps = 0;
  uint32_t n_pos = 0;
  const std::string tmp = out_path + ".tmp";
  auto checkpoint = [&](uint64_t bits) {
    ++n_pos;
    put(ck, bits);
    put(ck, (uint32_t)hashes.size());
    for (IndirectHash* h : hashes) {
      {
        std::ofstream f(tmp, std::ios::binary);
        h->WriteToDisk(&f);
      }
      const std::vector<uint8_t> sec = slurp(tmp);
      put(ck, (uint64_t)sec.size());
      ck.insert(ck.end(), sec.begin(), sec.end());
    }
    put(ck, (int32_t)stm.recent_bits);
    put(ck, (int32_t)stm.new_bit);
    put(ck, (uint32_t)stm.last_byte);
    put(ck, (uint32_t)stm.rotating_history_pos);
    put(ck, (int32_t)basic.first_prediction_);
    for (int i = 0; i < 10; ++i) put(ck, (uint32_t)stm.recent_bytes[i]);
    for (int v = 0; v < 64; ++v) put(ck, (uint32_t)(v < V ? *vars[v] : 0u));
    for (int i = 0; i < 1000; ++i) put(ck, (uint8_t)stm.rotating_history[i]);
  };
  for (uint64_t t = 0; t <= T; ++t) {
    for (uint64_t p : positions)
      if (p == t) checkpoint(t);
    if (t == T) break;
    const int bit = (data[t / 8] >> (7 - t % 8)) & 1;
    // ---- Predictor::Predict
    const unsigned pos_before = stm.rotating_history_pos;
    basic.Predict(stm, ltm);
    if (stm.rotating_history_pos < pos_before) ++wraps;
    std::vector<unsigned> old_idx;
    for (IndirectHash* h : hashes) old_idx.push_back(h->outer_hash_ % h->table_.size());
    for (auto& m : objs) m->Predict(stm, ltm);
    if (stm.recent_bits == 1)
      for (size_t i = 0; i < hashes.size(); ++i)
        same_entry += old_idx[i] == hashes[i]->outer_hash_ % hashes[i]->table_.size();
    for (int v = 0; v < V; ++v) put(o, (uint32_t)*vars[v]);
    // ---- Predictor::Perceive; none of these objects learns
    stm.new_bit = bit;
  }
  remove(tmp.c_str());
  put(o, n_pos);
  o.insert(o.end(), ck.begin(), ck.end());
  put(o, same_entry);
  put(o, wraps);
  std::ofstream f(out_path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(o.data()), (std::streamsize)o.size());
  return f.good() ? 0 : 1;
}
