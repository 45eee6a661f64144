// gmx_sections.h -- the byte layout of the three sparse sections of the reference's `.long` file, the ones
// LongTermMemory::WriteToDisk / ReadFromDisk move (long-term-memory.cpp:8-54, :70-106) and gmx_*_export / gmx_*_import
// speak: the Indirect models' tables, the Match models' history and pointer tables, the mixers' gate rows.  The ONE place
// under gmix_amd/host/ that knows when a table is written sparse, how wide an entry is and what follows it: the adapters
// (gmx_model_adapter.h) encode from and decode into LongTermMemory through it, the stand-alone mirrors (gmx_models.h)
// take from it how many bytes to read from a stream.  No HIP, no reference types: tables are plain pointers and sizes,
// the mixers' rows (std::unique_ptr<MixerData> on the adapter's side) small callbacks.
//
// Per section type: *Payload (the bytes between the u32 count and the trailer), *Encode, *Decode.  A decode never reads
// past the buffer and returns false for a truncated section, a sparse key outside the table or a mixer row outside its
// table; what it wrote into the views until then stays.
#ifndef GMX_SECTIONS_H_
#define GMX_SECTIONS_H_

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace gmx {
namespace sections {

struct Sink {  // appends to a byte vector
  std::vector<char>& buf;
  void Put(const void* p, size_t n) {
    const char* c = static_cast<const char*>(p);
    buf.insert(buf.end(), c, c + n);
  }
  template <class T>
  void Pod(T v) {
    Put(&v, sizeof v);
  }
};

class Source {  // a cursor over (ptr, len): a take succeeds, or marks the source failed and gives zeros
 public:
  Source(const void* p, size_t len) : p_(static_cast<const char*>(p)), left_(len) {}
  bool ok() const { return ok_; }
  size_t left() const { return left_; }
  const char* View(size_t n) {  // the next n bytes where they lie, or null
    if (!ok_ || n > left_) {
      ok_ = false;
      return nullptr;
    }
    const char* at = p_;
    p_ += n;
    left_ -= n;
    return at;
  }
  void Take(void* dst, size_t n) {
    if (const char* at = View(n))
      memcpy(dst, at, n);
    else
      memset(dst, 0, n);
  }
  template <class T>
  T Pod() {
    T v;
    Take(&v, sizeof v);
    return v;
  }

 private:
  const char* p_;
  size_t left_;
  bool ok_ = true;
};

constexpr size_t kTrailer = 2 * 256 * 4;  // behind every Indirect and Match model: two arrays of 256 four-byte values

// ---- Indirect (long-term-memory.cpp:8-32): per model u32 count | count x {u32 key, u8 nonstationary, u8 run_map} or
// table A whole, table B whole | 2 x 256 floats.  An entry is live iff nonstationary != 255.
struct IndirectView {
  unsigned char *nonstationary, *run_map;  // [size] each; a decode finds them {255, 0} throughout
  size_t size;                             // IndirectSize(table_size)
  float *nonstationary_predictions, *run_map_predictions;  // [256] each
};
inline uint64_t IndirectSize(uint32_t table_size) { return (uint64_t)table_size * 256u + 1u; }  // indirect.cpp:14-19
inline bool IndirectSparse(uint64_t count, uint64_t size) { return count < size / 3; }
inline size_t IndirectPayload(uint32_t count, uint64_t size) {
  return IndirectSparse(count, size) ? (size_t)count * 6 : (size_t)size * 2;
}
inline void IndirectEncode(Sink s, const IndirectView& v) {
  uint32_t count = 0;
  for (size_t k = 0; k < v.size; ++k) count += v.nonstationary[k] != 255;
  s.Pod(count);
  if (IndirectSparse(count, v.size)) {
    for (size_t k = 0; k < v.size; ++k) {
      if (v.nonstationary[k] == 255) continue;
      s.Pod((uint32_t)k);
      s.Pod(v.nonstationary[k]);
      s.Pod(v.run_map[k]);
    }
  } else {
    s.Put(v.nonstationary, v.size);
    s.Put(v.run_map, v.size);
  }
  s.Put(v.nonstationary_predictions, kTrailer / 2);
  s.Put(v.run_map_predictions, kTrailer / 2);
}
inline bool IndirectDecode(Source& s, const IndirectView& v) {
  const uint32_t count = s.Pod<uint32_t>();
  if (s.left() < IndirectPayload(count, v.size)) return false;
  if (IndirectSparse(count, v.size)) {
    for (uint32_t i = 0; i < count; ++i) {
      const uint32_t key = s.Pod<uint32_t>();
      if (key >= v.size) return false;
      v.nonstationary[key] = s.Pod<unsigned char>();
      v.run_map[key] = s.Pod<unsigned char>();
    }
  } else {
    s.Take(v.nonstationary, v.size);
    s.Take(v.run_map, v.size);
  }
  s.Take(v.nonstationary_predictions, kTrailer / 2);
  s.Take(v.run_map_predictions, kTrailer / 2);
  return s.ok();
}

// ---- Match (long-term-memory.cpp:70-106): u64 history length | history | per model u32 count | count x {u32 key,
// 5 bytes} or the table whole | 2 x 256 x 4 bytes.  An entry is live iff any of its 5 bytes is set.
struct MatchView {
  unsigned char* table;  // [table_size][5]; a decode finds it zero throughout
  size_t table_size;
  void *predictions, *counts;  // 256 x 4 bytes each
};
// (match.cpp's rule, in double: sparse records below 5/9 of the table)
inline bool MatchSparse(uint32_t count, size_t table_size) { return (double)count < (5.0 / 9.0) * (double)table_size; }
inline size_t MatchPayload(uint32_t count, size_t table_size) {
  return MatchSparse(count, table_size) ? (size_t)count * 9 : table_size * 5;
}
inline void MatchHistoryEncode(Sink s, const unsigned char* history, uint64_t n) {
  s.Pod(n);
  s.Put(history, (size_t)n);
}
inline bool MatchHistoryDecode(Source& s, const unsigned char** history, uint64_t* n) {
  *n = s.Pod<uint64_t>();
  static_assert(sizeof(size_t) >= sizeof(uint64_t), "a history length is taken as a size_t");
  *history = reinterpret_cast<const unsigned char*>(s.View((size_t)*n));
  return s.ok();
}
inline bool MatchLive(const unsigned char* e) { return e[0] || e[1] || e[2] || e[3] || e[4]; }
inline void MatchEncode(Sink s, const MatchView& v) {
  uint32_t count = 0;
  for (size_t k = 0; k < v.table_size; ++k) count += MatchLive(v.table + 5 * k);
  s.Pod(count);
  if (MatchSparse(count, v.table_size)) {
    for (size_t k = 0; k < v.table_size; ++k) {
      if (!MatchLive(v.table + 5 * k)) continue;
      s.Pod((uint32_t)k);
      s.Put(v.table + 5 * k, 5);
    }
  } else {
    s.Put(v.table, 5 * v.table_size);
  }
  s.Put(v.predictions, kTrailer / 2);
  s.Put(v.counts, kTrailer / 2);
}
inline bool MatchDecode(Source& s, const MatchView& v) {
  const uint32_t count = s.Pod<uint32_t>();
  if (s.left() < MatchPayload(count, v.table_size)) return false;
  if (MatchSparse(count, v.table_size)) {
    for (uint32_t i = 0; i < count; ++i) {
      const uint32_t key = s.Pod<uint32_t>();
      if (key >= v.table_size) return false;
      s.Take(v.table + 5 * (size_t)key, 5);
    }
  } else {
    s.Take(v.table, 5 * v.table_size);
  }
  s.Take(v.predictions, kTrailer / 2);
  s.Take(v.counts, kTrailer / 2);
  return s.ok();
}

// ---- Mixer (long-term-memory.cpp:35-54): per mixer u32 n | u32 input_size | n x {u32 row, u64 steps, input_size floats}.
// MixerPayload: what follows the count n -- the input_size word and the records.
inline size_t MixerPayload(uint32_t n, uint32_t input_size) { return 4 + (size_t)n * (12 + 4 * (size_t)input_size); }
// row(c, &steps, &n_weights) -> the weights of row c, or null where the table has none
template <class RowAt>
void MixerEncode(Sink s, uint32_t table_size, RowAt row) {
  uint32_t n = 0, input_size = 0, w = 0;
  uint64_t steps = 0;
  for (uint32_t c = 0; c < table_size; ++c)
    if (row(c, &steps, &w)) {
      ++n;
      input_size = w;
    }
  s.Pod(n);
  s.Pod(input_size);
  for (uint32_t c = 0; c < table_size; ++c)
    if (const float* weights = row(c, &steps, &w)) {
      s.Pod(c);
      s.Pod(steps);
      s.Put(weights, 4 * (size_t)w);
    }
}
// put(c, steps, weights, input_size): row c of the table; `weights` are input_size floats wherever the bytes lie
template <class PutRow>
bool MixerDecode(Source& s, uint32_t table_size, PutRow put) {
  const uint32_t n = s.Pod<uint32_t>();
  const uint32_t input_size = s.Pod<uint32_t>();
  if (!s.ok() || s.left() + 4 < MixerPayload(n, input_size)) return false;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = s.Pod<uint32_t>();
    const uint64_t steps = s.Pod<uint64_t>();
    const char* weights = s.View(4 * (size_t)input_size);
    if (!weights || c >= table_size) return false;
    put(c, steps, weights, input_size);
  }
  return true;
}

}  // namespace sections
}  // namespace gmx

#endif  // GMX_SECTIONS_H_
