// The codec of the three sparse `.long` sections (gmix_amd/host/gmx_sections.h) against the expressions the adapters
// carried by hand, written out here as the oracle: the Indirect rule at both sides of size / 3, the Match rule where the
// comparison in double and one in integers part, the mixers' row records; every proper prefix of a section and keys
// outside a table are refused without a byte read or written outside the buffers (run it under
// -fsanitize=address,undefined to see that).  No GPU, no HIP, no reference sources.
//   g++ -std=c++17 -Wall -I gmix_amd/host tests/cpp/test_sections.cpp && ./a.out
#include "gmx_sections.h"

#include <stdio.h>
#include <string.h>

#include <array>
#include <memory>
#include <vector>

namespace sec = gmx::sections;

static char g_case[160] = "";  // the case a failed check belongs to
#define CASE(...) snprintf(g_case, sizeof g_case, __VA_ARGS__)
#define CHECK(c)                                                                        \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      fprintf(stderr, "%s:%d: CHECK(%s) [%s]\n", __FILE__, __LINE__, #c, g_case);       \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

static void put(std::vector<char>& buf, const void* p, size_t n) {
  const char* c = static_cast<const char*>(p);
  buf.insert(buf.end(), c, c + n);
}

// ---- Indirect -------------------------------------------------------------------------------------------------
struct IndirectMem {  // LongTermMemory::indirect[i] as the adapter stages it
  std::vector<unsigned char> nonstationary_table, run_map_table;
  std::array<float, 256> nonstationary_predictions, run_map_predictions;
  explicit IndirectMem(size_t size) : nonstationary_table(size, 255), run_map_table(size, 0) {
    nonstationary_predictions.fill(0);
    run_map_predictions.fill(0);
  }
  sec::IndirectView view() {
    return {nonstationary_table.data(), run_map_table.data(), nonstationary_table.size(), nonstationary_predictions.data(),
            run_map_predictions.data()};
  }
  bool operator==(const IndirectMem& o) const {
    return nonstationary_table == o.nonstationary_table && run_map_table == o.run_map_table &&
           !memcmp(nonstationary_predictions.data(), o.nonstationary_predictions.data(), 1024) &&
           !memcmp(run_map_predictions.data(), o.run_map_predictions.data(), 1024);
  }
};
static IndirectMem make_indirect(unsigned table_size, unsigned live) {
  IndirectMem mem((size_t)table_size * 256 + 1);
  const size_t size = mem.nonstationary_table.size();
  for (unsigned i = 0; i < live; ++i) {
    const size_t k = (size_t)i * 101 % size;  // (101 shares no factor with 257 or 513: `live` distinct keys)
    mem.nonstationary_table[k] = (unsigned char)(i * 7 % 255);
    mem.run_map_table[k] = (unsigned char)(i * 13 + 1);
  }
  for (int i = 0; i < 256; ++i) {
    mem.nonstationary_predictions[i] = 0.25f * (float)i - 3.0f * (float)live;
    mem.run_map_predictions[i] = 1.0f / (float)(i + 1 + live);
  }
  return mem;
}
// the encoder the adapter carried
static std::vector<char> oracle_indirect(const IndirectMem& mem) {
  std::vector<char> buf;
  std::vector<unsigned int> keys;
  for (unsigned int k = 0; k < mem.nonstationary_table.size(); ++k)
    if (mem.nonstationary_table[k] != 255) keys.push_back(k);
  unsigned int size = (unsigned int)keys.size();
  put(buf, &size, 4);
  if (size < mem.nonstationary_table.size() / 3) {
    for (unsigned int key : keys) {
      put(buf, &key, 4);
      put(buf, &mem.nonstationary_table[key], 1);
      put(buf, &mem.run_map_table[key], 1);
    }
  } else {
    put(buf, mem.nonstationary_table.data(), mem.nonstationary_table.size());
    put(buf, mem.run_map_table.data(), mem.run_map_table.size());
  }
  put(buf, mem.nonstationary_predictions.data(), 256 * 4);
  put(buf, mem.run_map_predictions.data(), 256 * 4);
  return buf;
}
static bool decode_indirect(const char* p, size_t len, IndirectMem* out) {
  std::vector<char> exact(p, p + len);  // (a buffer of exactly len bytes: a sanitizer sees the first byte past it)
  sec::Source src(exact.data(), exact.size());
  return sec::IndirectDecode(src, out->view()) && src.left() == 0;
}
static int test_indirect() {
  int cases = 0;
  for (unsigned table_size = 1; table_size <= 2; ++table_size) {
    const unsigned size = table_size * 256 + 1, third = size / 3;
    CHECK(sec::IndirectSize(table_size) == size && third == (table_size == 1 ? 85u : 171u));
    const unsigned counts[] = {0, 1, third - 1, third, third + 1, size};
    for (unsigned live : counts) {
      CASE("indirect table_size %u count %u", table_size, live);
      IndirectMem mem = make_indirect(table_size, live);
      std::vector<char> enc;
      sec::IndirectEncode(sec::Sink{enc}, mem.view());
      CHECK(enc == oracle_indirect(mem));
      const bool sparse = live < third;  // third - 1 is the last sparse count, third the first dense one
      CHECK(enc.size() == 4 + (sparse ? 6 * (size_t)live : 2 * (size_t)size) + 2048);
      CHECK(sec::IndirectPayload(live, size) == enc.size() - 4 - sec::kTrailer);
      IndirectMem back(size);
      CHECK(decode_indirect(enc.data(), enc.size(), &back) && back == mem);
      for (size_t n = 0; n < enc.size(); ++n) {  // every proper prefix
        IndirectMem junk(size);
        CHECK(!decode_indirect(enc.data(), n, &junk));
      }
      ++cases;
    }
    // a sparse key one past the table
    IndirectMem mem = make_indirect(table_size, 1);
    std::vector<char> enc = oracle_indirect(mem);
    memcpy(&enc[4], &size, 4);
    IndirectMem junk(size);
    CHECK(!decode_indirect(enc.data(), enc.size(), &junk));
    const unsigned last = size - 1;
    memcpy(&enc[4], &last, 4);
    CHECK(decode_indirect(enc.data(), enc.size(), &junk) && junk.nonstationary_table[last] == 0);
  }
  // the predicate alone at the stock sizes (gmix_amd/topology.py: table_size 1 << 8, 1 << 15, 1 << 16)
  for (unsigned table_size : {1u << 8, 1u << 15, 1u << 16}) {
    const size_t size = (size_t)table_size * 256 + 1;
    const unsigned int threshold = (unsigned int)(size / 3);
    for (unsigned int count : {threshold - 1, threshold, threshold + 1}) {
      CHECK(sec::IndirectSparse(count, sec::IndirectSize(table_size)) == (count < size / 3));
      CHECK(sec::IndirectPayload(count, size) == (count < size / 3 ? (size_t)count * 6 : size * 2));
    }
  }
  printf("ok: indirect sections, %d cases\n", cases);
  return 0;
}

// ---- Match ----------------------------------------------------------------------------------------------------
struct MatchMem {  // LongTermMemory::match_memory[i]
  std::vector<std::array<unsigned char, 5>> table;
  std::array<float, 256> predictions;
  std::array<int, 256> counts;
  explicit MatchMem(size_t table_size) : table(table_size, std::array<unsigned char, 5>{{0, 0, 0, 0, 0}}) {
    predictions.fill(0);
    counts.fill(0);
  }
  sec::MatchView view() { return {table.data()->data(), table.size(), predictions.data(), counts.data()}; }
  bool operator==(const MatchMem& o) const {
    return table == o.table && !memcmp(predictions.data(), o.predictions.data(), 1024) && counts == o.counts;
  }
};
static MatchMem make_match(unsigned table_size, unsigned live) {
  MatchMem mem(table_size);
  for (unsigned i = 0; i < live; ++i) {
    const size_t k = (size_t)i * 2 % table_size;  // (table_size is odd here: `live` distinct keys)
    mem.table[k] = {{0, 0, (unsigned char)(i & 1), 0, (unsigned char)(i + 1)}};  // (live through its last bytes alone)
  }
  for (int i = 0; i < 256; ++i) {
    mem.predictions[i] = 0.5f + ((float)i + 0.5f) / 512 + (float)live;
    mem.counts[i] = 1 + i * (int)(live + 1);
  }
  return mem;
}
static void oracle_match_history(std::vector<char>& buf, const std::vector<unsigned char>& history) {
  const unsigned long long hs = history.size();
  put(buf, &hs, 8);
  put(buf, history.data(), history.size());
}
static void oracle_match(std::vector<char>& buf, const MatchMem& mem) {
  std::vector<unsigned int> keys;
  for (unsigned int k = 0; k < mem.table.size(); ++k) {
    const auto& e = mem.table[k];
    if (e[0] || e[1] || e[2] || e[3] || e[4]) keys.push_back(k);
  }
  unsigned int size = (unsigned int)keys.size();
  put(buf, &size, 4);
  if (size < (5.0 / 9.0) * mem.table.size()) {
    for (unsigned int key : keys) {
      put(buf, &key, 4);
      put(buf, mem.table[key].data(), 5);
    }
  } else {
    put(buf, mem.table.data(), 5 * mem.table.size());
  }
  put(buf, mem.predictions.data(), 256 * 4);
  put(buf, mem.counts.data(), 256 * 4);
}
static bool decode_match(const char* p, size_t len, std::vector<unsigned char>* history, MatchMem* a, MatchMem* b) {
  std::vector<char> exact(p, p + len);
  sec::Source src(exact.data(), exact.size());
  const unsigned char* h;
  uint64_t hs;
  if (!sec::MatchHistoryDecode(src, &h, &hs)) return false;
  history->assign(h, h + hs);
  return sec::MatchDecode(src, a->view()) && sec::MatchDecode(src, b->view()) && src.left() == 0;
}
static int test_match() {
  static_assert(sizeof(std::array<unsigned char, 5>) == 5, "the table is 5 bytes per entry");
  int cases = 0;
  for (size_t hist : {(size_t)0, (size_t)1, (size_t)1000}) {
    std::vector<unsigned char> history(hist);
    for (size_t i = 0; i < hist; ++i) history[i] = (unsigned char)(i * 31 + 5);
    for (unsigned c7 = 0; c7 <= 7; ++c7)
      for (unsigned c9 = 0; c9 <= 9; ++c9) {  // two models in one section, empty to full
        CASE("match history %zu, table_size 7 count %u, table_size 9 count %u", hist, c7, c9);
        MatchMem m7 = make_match(7, c7), m9 = make_match(9, c9);
        std::vector<char> enc, want;
        sec::MatchHistoryEncode(sec::Sink{enc}, history.data(), history.size());
        sec::MatchEncode(sec::Sink{enc}, m7.view());
        sec::MatchEncode(sec::Sink{enc}, m9.view());
        oracle_match_history(want, history);
        oracle_match(want, m7);
        oracle_match(want, m9);
        CHECK(enc == want);
        // 7: 3 sparse, 4 dense (3 < 35.0 / 9, where 5 * 7 / 9 in integers is 3); 9: 4 sparse, 5 dense (5 < 5.0 is false)
        const size_t b7 = c7 <= 3 ? 9 * (size_t)c7 : 35, b9 = c9 <= 4 ? 9 * (size_t)c9 : 45;
        CHECK(enc.size() == 8 + hist + (4 + b7 + 2048) + (4 + b9 + 2048));
        CHECK(sec::MatchPayload(c7, 7) == b7 && sec::MatchPayload(c9, 9) == b9);
        std::vector<unsigned char> hback;
        MatchMem a(7), b(9);
        CHECK(decode_match(enc.data(), enc.size(), &hback, &a, &b) && hback == history && a == m7 && b == m9);
        const bool edge = (c7 == 3 && c9 == 4) || (c7 == 4 && c9 == 5) || (c7 == 0 && c9 == 9) || (c7 == 7 && c9 == 0);
        if (edge)
          for (size_t n = 0; n < enc.size(); ++n) {  // every proper prefix
            MatchMem ja(7), jb(9);
            CHECK(!decode_match(enc.data(), n, &hback, &ja, &jb));
          }
        ++cases;
      }
  }
  {  // one model alone: payload against the encoded length, and a sparse key one past the table
    for (unsigned table_size : {7u, 9u})
      for (unsigned live = 0; live <= table_size; ++live) {
        MatchMem mem = make_match(table_size, live);
        std::vector<char> enc;
        sec::MatchEncode(sec::Sink{enc}, mem.view());
        CHECK(sec::MatchPayload(live, table_size) == enc.size() - 4 - sec::kTrailer);
      }
    MatchMem mem = make_match(9, 1), junk(9);
    std::vector<char> enc;
    oracle_match(enc, mem);
    const unsigned bad = 9, last = 8;
    memcpy(&enc[4], &bad, 4);
    sec::Source s1(enc.data(), enc.size());
    CHECK(!sec::MatchDecode(s1, junk.view()));
    memcpy(&enc[4], &last, 4);
    sec::Source s2(enc.data(), enc.size());
    CHECK(sec::MatchDecode(s2, junk.view()) && junk.table[8][4] == 1);
  }
  // the predicate alone at the stock table sizes (gmix_amd/topology.py), around the first dense count
  for (unsigned table_size : {1u << 8, 1u << 16, 1u << 24, 1u << 21, 7u, 9u}) {
    unsigned int threshold = 0;
    while (threshold < (5.0 / 9.0) * (size_t)table_size) ++threshold;
    CHECK(threshold >= 1);
    for (unsigned int count : {threshold - 1, threshold, threshold + 1}) {
      const bool sparse = count < (5.0 / 9.0) * (size_t)table_size;
      CHECK(sec::MatchSparse(count, table_size) == sparse && sparse == (count < threshold));
      CHECK(sec::MatchPayload(count, table_size) == (sparse ? (size_t)count * 9 : (size_t)table_size * 5));
    }
  }
  printf("ok: match sections, %d cases\n", cases);
  return 0;
}

// ---- Mixer ----------------------------------------------------------------------------------------------------
struct MixerData {  // the reference's row: a step count and the weights
  unsigned long long steps = 0;
  std::vector<float> weights;
  explicit MixerData(size_t input_size) : weights(input_size, 0.f) {}
};
typedef std::vector<std::unique_ptr<MixerData>> MixerTable;
static MixerTable make_mixer(unsigned table_size, unsigned input_size, int present) {  // 0 none, 1 one row, 2 all
  MixerTable t(table_size);
  for (unsigned c = 0; c < table_size; ++c) {
    if (present == 0 || (present == 1 && c != table_size * 3 / 5)) continue;
    t[c].reset(new MixerData(input_size));
    t[c]->steps = (1ull << 40) + 1000ull * c + input_size;
    for (unsigned i = 0; i < input_size; ++i) t[c]->weights[i] = 0.125f * (float)(c + 1) - (float)i;
  }
  return t;
}
static void oracle_mixer(std::vector<char>& buf, const MixerTable& table) {
  uint32_t n = 0, input_size = 0;
  for (auto& row : table)
    if (row) {
      ++n;
      input_size = (uint32_t)row->weights.size();
    }
  put(buf, &n, 4);
  put(buf, &input_size, 4);
  for (uint32_t c = 0; c < table.size(); ++c) {
    if (!table[c]) continue;
    uint64_t steps = table[c]->steps;
    put(buf, &c, 4);
    put(buf, &steps, 8);
    put(buf, &table[c]->weights[0], 4 * table[c]->weights.size());
  }
}
static void encode_mixer(std::vector<char>& buf, const MixerTable& table) {
  sec::MixerEncode(sec::Sink{buf}, (uint32_t)table.size(), [&](uint32_t c, uint64_t* steps, uint32_t* n) -> const float* {
    if (!table[c]) return nullptr;
    *steps = table[c]->steps;
    *n = (uint32_t)table[c]->weights.size();
    return table[c]->weights.data();
  });
}
static bool decode_mixer(sec::Source& src, MixerTable* table) {
  return sec::MixerDecode(src, (uint32_t)table->size(), [&](uint32_t c, uint64_t steps, const char* w, uint32_t input_size) {
    MixerData* row = new MixerData(input_size);
    row->steps = steps;
    memcpy(row->weights.data(), w, 4 * (size_t)input_size);
    (*table)[c].reset(row);
  });
}
static bool same_rows(const MixerTable& a, const MixerTable& b) {
  if (a.size() != b.size()) return false;
  for (size_t c = 0; c < a.size(); ++c) {
    if (!a[c] != !b[c]) return false;
    if (a[c] && (a[c]->steps != b[c]->steps || a[c]->weights.size() != b[c]->weights.size() ||
                 memcmp(a[c]->weights.data(), b[c]->weights.data(), 4 * a[c]->weights.size())))
      return false;
  }
  return true;
}
static bool decode_mixers(const char* p, size_t len, MixerTable* a, MixerTable* b) {
  std::vector<char> exact(p, p + len);
  sec::Source src(exact.data(), exact.size());
  return decode_mixer(src, a) && decode_mixer(src, b) && src.left() == 0;
}
static int test_mixer() {
  int cases = 0;
  const unsigned shapes[4][4] = {{1, 1, 5, 4}, {1, 4, 5, 1}, {5, 1, 1, 4}, {5, 4, 1, 1}};  // {table, inputs} of two mixers
  for (auto& sh : shapes)
    for (int pa = 0; pa < 3; ++pa)
      for (int pb = 0; pb < 3; ++pb) {
        CASE("mixers {%u, %u} rows %d and {%u, %u} rows %d", sh[0], sh[1], pa, sh[2], sh[3], pb);
        MixerTable a = make_mixer(sh[0], sh[1], pa), b = make_mixer(sh[2], sh[3], pb);
        std::vector<char> enc, want;
        encode_mixer(enc, a);
        const size_t first = enc.size();
        encode_mixer(enc, b);
        oracle_mixer(want, a);
        oracle_mixer(want, b);
        CHECK(enc == want);
        const uint32_t na = pa == 0 ? 0 : pa == 1 ? 1 : sh[0];
        CHECK(first == 8 + (size_t)na * (12 + 4 * sh[1]));
        CHECK(sec::MixerPayload(na, na ? sh[1] : 0) == first - 4);
        MixerTable ra(sh[0]), rb(sh[2]);
        CHECK(decode_mixers(enc.data(), enc.size(), &ra, &rb) && same_rows(ra, a) && same_rows(rb, b));
        for (size_t n = 0; n < enc.size(); ++n) {  // every proper prefix
          MixerTable ja(sh[0]), jb(sh[2]);
          CHECK(!decode_mixers(enc.data(), n, &ja, &jb));
        }
        ++cases;
      }
  // a row one past the table
  MixerTable t = make_mixer(5, 4, 1), junk(5);
  std::vector<char> enc;
  oracle_mixer(enc, t);
  const uint32_t bad = 5, last = 4;
  memcpy(&enc[8], &bad, 4);
  sec::Source s1(enc.data(), enc.size());
  CHECK(!decode_mixer(s1, &junk));
  memcpy(&enc[8], &last, 4);
  sec::Source s2(enc.data(), enc.size());
  CHECK(decode_mixer(s2, &junk) && junk[4] && junk[4]->steps == t[3]->steps);
  printf("ok: mixer sections, %d cases\n", cases);
  return 0;
}

// ---- the source itself ----------------------------------------------------------------------------------------
static int test_source() {
  const char bytes[6] = {1, 2, 3, 4, 5, 6};
  sec::Source s(bytes, 6);
  CHECK(s.Pod<uint32_t>() == 0x04030201u && s.ok() && s.left() == 2);
  CHECK(s.Pod<uint32_t>() == 0 && !s.ok());  // a take that does not fit: zeros, and failed from then on
  CHECK(s.Pod<unsigned char>() == 0 && !s.View(1) && s.left() == 2);
  char dst[3] = {9, 9, 9};
  s.Take(dst, 3);
  CHECK(dst[0] == 0 && dst[1] == 0 && dst[2] == 0);
  sec::Source e(bytes, 0);
  CHECK(e.View(0) && e.ok() && !e.View(1) && !e.ok());
  printf("ok: byte source\n");
  return 0;
}

int main() { return test_source() || test_indirect() || test_match() || test_mixer(); }
