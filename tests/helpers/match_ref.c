/* match_ref.c -- a plain-C restatement of the reference's Match models, the history rule of BasicContexts::Learn and
 * the match section of the checkpoint.  Test infrastructure only: tests/test_match_ref.py pins it against fixtures the
 * reference itself produced (tests/golden/match_*.npz), tests/test_gpu_match.py then uses it where no fixture reaches
 * (streams replayed from other offsets, sections exchanged with the device).  Build:
 *   gcc -O2 -ffp-contract=off -shared -fPIC match_ref.c -o match_ref.so -lm
 * Table entries are five bytes and cur_match_ is 64 bits wide, as in the reference. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  uint32_t table_size;
  int limit;
  uint8_t* table;          /* [table_size][5], long-term-memory.h:46-47 */
  float predictions[256];  /* long-term-memory.h:50 */
  int counts[256];         /* long-term-memory.h:52 */
  /* match.h:34-42 */
  unsigned long long cur_match;
  uint8_t cur_byte, bit_pos, match_length;
  float learning_rate;
  float slot;              /* ShortTermMemory::predictions[prediction_index_] */
} mref_model;

typedef struct {
  int K;
  mref_model m[8];
  uint8_t* history;        /* long-term-memory.h:82 */
  uint64_t hist_size, hist_cap;
  int new_bit;             /* short-term-memory.h:58 */
} mref;

/* Match::Match (match.cpp:3-23) and MatchMemory (long-term-memory.h:42-45) */
mref* mref_create(int K, const uint32_t* table_size, const int* limit) {
  if (K < 1 || K > 8) return NULL;
  mref* r = (mref*)calloc(1, sizeof(mref));
  r->K = K;
  for (int k = 0; k < K; ++k) {
    mref_model* m = &r->m[k];
    m->table_size = table_size[k];
    m->limit = limit[k];
    m->table = (uint8_t*)calloc((size_t)table_size[k], 5);
    for (int i = 0; i < 256; ++i) {
      m->predictions[i] = 0.5 + (i + 0.5) / 512;
      m->counts[i] = 1;
    }
    m->bit_pos = 128;
    m->learning_rate = 1.0 / limit[k];
  }
  r->hist_cap = 1024;
  r->history = (uint8_t*)malloc(r->hist_cap);
  return r;
}

void mref_destroy(mref* r) {
  if (!r) return;
  for (int k = 0; k < r->K; ++k) free(r->m[k].table);
  free(r->history);
  free(r);
}

/* Sigmoid::Logit (mixer/sigmoid.cpp:7-13) */
static float mref_logit(float p) {
  if (p < 0.0001)
    p = 0.0001;
  else if (p > 0.9999)
    p = 0.9999;
  return logf(p / (1 - p));
}

/* Match::Predict (match.cpp:25-74); ctx = byte_context_, recent_bits = bit_context + 1; returns whether
 * ShortTermMemory::SetPrediction marked the model active (short-term-memory.cpp:187-191). */
static int mref_predict(mref* r, mref_model* m, uint32_t ctx, uint32_t bit_context, unsigned* longest_match) {
  int match = 0, active = 0;
  if (r->new_bit == ((m->cur_byte & m->bit_pos) != 0)) match = 1;
  if (match) {
    if (m->match_length < 255) ++m->match_length;
  } else {
    m->match_length = 0;
  }
  m->bit_pos /= 2;
  if (bit_context == 0) {
    if (m->cur_match == r->hist_size - 1) m->match_length = 0;  /* (uint64: an empty history gives 2^64 - 1) */
    if (m->match_length < 8) {
      const uint8_t* it = m->table + 5ull * (ctx % m->table_size);
      m->cur_match = it[0] + (1 << 8) * it[1] + (1 << 16) * it[2] + (1ull << 24) * it[3] + (1ull << 32) * it[4];
    } else {
      ++m->cur_match;
    }
    if (r->hist_size != 0) m->cur_byte = r->history[m->cur_match];
    m->bit_pos = 128;
  }
  if (m->match_length > 2) {
    float p;
    if (m->cur_byte & m->bit_pos)
      p = m->predictions[m->match_length];
    else
      p = 1 - m->predictions[m->match_length];
    m->slot = mref_logit(p);
    active = p != 0.5;
  }
  unsigned mc = m->match_length / 32;
  if (mc > *longest_match) *longest_match = mc;
  return active;
}

/* Match::Learn (match.cpp:76-109) */
static void mref_learn(mref* r, mref_model* m, uint32_t ctx, uint32_t bit_context, unsigned longest_match) {
  if (m->match_length > 2) {
    int match = 0;
    if (r->new_bit == ((m->cur_byte & m->bit_pos) != 0)) match = 1;
    float learning_rate = m->learning_rate;
    if (m->counts[m->match_length] < m->limit) {
      ++m->counts[m->match_length];
      learning_rate = 1.0 / m->counts[m->match_length];
    }
    m->predictions[m->match_length] += (match - m->predictions[m->match_length]) * learning_rate;
  }
  if (bit_context + 1 >= 128) {
    if (longest_match >= 2) return;
    uint8_t* loc = m->table + 5ull * (ctx % m->table_size);
    unsigned long long pos = r->hist_size - 1;
    loc[0] = pos;
    loc[1] = pos >> 8;
    loc[2] = pos >> 16;
    loc[3] = pos >> 24;
    loc[4] = pos >> 32;
  }
}

/* T bits in Predictor's order (predictor.cpp:366-368, :378-387): BasicContexts::Predict zeroes longest_match
 * (basic-contexts.cpp:39), the K Match::Predict; Perceive; BasicContexts::Learn pushes the byte
 * (basic-contexts.cpp:44-53), the K Match::Learn.  ctx [T][K], pred / act [T][K], longest [T]. */
void mref_run(mref* r, uint64_t T, const uint32_t* ctx, const uint32_t* bc, const uint8_t* bits, float* pred,
              uint8_t* act, uint32_t* longest) {
  const int K = r->K;
  for (uint64_t t = 0; t < T; ++t) {
    unsigned lm = 0;
    for (int k = 0; k < K; ++k) {
      const int a = mref_predict(r, &r->m[k], ctx[t * K + k], bc[t], &lm);
      if (pred) pred[t * K + k] = r->m[k].slot;
      if (act) act[t * K + k] = (uint8_t)a;
    }
    if (longest) longest[t] = lm;
    r->new_bit = bits[t];
    const int current_byte = (int)(bc[t] + 1) * 2 + r->new_bit;
    if (current_byte >= 256 && lm < 2) {
      if (r->hist_size == r->hist_cap) {
        r->hist_cap *= 2;
        r->history = (uint8_t*)realloc(r->history, r->hist_cap);
      }
      r->history[r->hist_size++] = (uint8_t)current_byte;
    }
    for (int k = 0; k < K; ++k) mref_learn(r, &r->m[k], ctx[t * K + k], bc[t], lm);
  }
}

uint64_t mref_history_size(const mref* r) { return r->hist_size; }
void mref_slots_get(const mref* r, float* v, int* new_bit) {
  for (int k = 0; k < r->K; ++k) v[k] = r->m[k].slot;
  *new_bit = r->new_bit;
}
void mref_slots_set(mref* r, const float* v, int new_bit) {
  for (int k = 0; k < r->K; ++k) r->m[k].slot = v[k];
  r->new_bit = new_bit;
}

static int mref_valid(const uint8_t* e) { return e[0] || e[1] || e[2] || e[3] || e[4]; }

/* The history and match section of LongTermMemory::WriteToDisk (long-term-memory.cpp:70-106); buf NULL: size only. */
uint64_t mref_export_long(const mref* r, uint8_t* buf) {
  uint64_t n = 0;
#define PUT(src, len)                      \
  do {                                     \
    if (buf) memcpy(buf + n, (src), (len)); \
    n += (len);                            \
  } while (0)
  unsigned long long size = r->hist_size;
  PUT(&size, 8);
  PUT(r->history, r->hist_size);
  for (int k = 0; k < r->K; ++k) {
    const mref_model* m = &r->m[k];
    unsigned int cnt = 0;
    for (uint32_t i = 0; i < m->table_size; ++i) cnt += mref_valid(m->table + 5ull * i);
    PUT(&cnt, 4);
    if (cnt < (5.0 / 9.0) * m->table_size) {
      for (uint32_t i = 0; i < m->table_size; ++i)
        if (mref_valid(m->table + 5ull * i)) {
          PUT(&i, 4);
          PUT(m->table + 5ull * i, 5);
        }
    } else {
      PUT(m->table, 5ull * m->table_size);
    }
    PUT(m->predictions, 1024);
    PUT(m->counts, 1024);
  }
#undef PUT
  return n;
}

/* Match::WriteToDisk x K (match.cpp:111-116): 11 K bytes */
void mref_export_short(const mref* r, uint8_t* buf) {
  for (int k = 0; k < r->K; ++k, buf += 11) {
    memcpy(buf, &r->m[k].cur_match, 8);
    buf[8] = r->m[k].cur_byte;
    buf[9] = r->m[k].bit_pos;
    buf[10] = r->m[k].match_length;
  }
}

/* LongTermMemory::ReadFromDisk's match part (long-term-memory.cpp:162-190) and Match::ReadFromDisk x K
 * (match.cpp:118-123) into a freshly created object; -1 when the section's length does not fit. */
int mref_import(mref* r, const uint8_t* lb, uint64_t ln, const uint8_t* sb, uint64_t sn) {
  uint64_t p = 0;
  unsigned long long size;
  if (sn != 11ull * r->K || ln < 8) return -1;
  memcpy(&size, lb, 8);
  p = 8;
  if (ln - p < size) return -1;
  if (size > r->hist_cap) {
    r->hist_cap = size;
    r->history = (uint8_t*)realloc(r->history, r->hist_cap);
  }
  memcpy(r->history, lb + p, size);
  r->hist_size = size;
  p += size;
  for (int k = 0; k < r->K; ++k) {
    mref_model* m = &r->m[k];
    unsigned int cnt;
    if (ln - p < 4) return -1;
    memcpy(&cnt, lb + p, 4);
    p += 4;
    if (cnt < (5.0 / 9.0) * m->table_size) {
      if (ln - p < 9ull * cnt) return -1;
      for (unsigned int i = 0; i < cnt; ++i, p += 9) {
        unsigned int key;
        memcpy(&key, lb + p, 4);
        if (key >= m->table_size) return -1;
        memcpy(m->table + 5ull * key, lb + p + 4, 5);
      }
    } else {
      if (ln - p < 5ull * m->table_size) return -1;
      memcpy(m->table, lb + p, 5ull * m->table_size);
      p += 5ull * m->table_size;
    }
    if (ln - p < 2048) return -1;
    memcpy(m->predictions, lb + p, 1024);
    memcpy(m->counts, lb + p + 1024, 1024);
    p += 2048;
  }
  if (p != ln) return -1;
  for (int k = 0; k < r->K; ++k, sb += 11) {
    memcpy(&r->m[k].cur_match, sb, 8);
    r->m[k].cur_byte = sb[8];
    r->m[k].bit_pos = sb[9];
    r->m[k].match_length = sb[10];
  }
  return 0;
}

/* Match::GetMemoryUsage (match.cpp:133-141) */
uint64_t mref_memory_usage(const mref* r, int k) { return 27ull + 256 * 4 + 256 * 4 + 5ull * r->m[k].table_size; }
