/* ctx_ref.c -- a plain-C restatement of the context variables of one stream, bit by bit: the context fields of
 * BasicContexts, IntervalContext, SkipContext and IndirectHash over the byte-level blackboard.  It is pinned to the
 * fixtures the reference produced (tests/golden/ctx_*.npz, tests/test_ctx_ref.py) and supplies per-bit values for the
 * chunkings and positions the fixtures do not record.  The structs are those of include/gmxmix.h. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  int32_t kind, index, num_bits, n_bytes, outer_order, inner_order;
  uint32_t table_size;
  uint8_t bytes_to_use[8];
  uint8_t map[256];
} cref_desc;

typedef struct {
  int32_t recent_bits, new_bit;
  uint32_t last_byte, rotating_history_pos;
  int32_t first_prediction;
  uint32_t recent_bytes[10];
  uint32_t values[64];
  uint8_t rotating_history[1000];
} cref_board;

typedef struct {
  int V;
  cref_desc d[64];
  int shift[64];
  uint32_t* table[64];
  uint64_t outer_context[64];
  uint32_t outer_hash[64];
  cref_board b;
} cref;

static uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
/* MurmurHash3_x86_32 (public domain) of n_words little-endian 32-bit words, seed 0xDEADBEEF */
static uint32_t murmur(const uint32_t* w, int n_words) {
  uint32_t h = 0xDEADBEEFu;
  for (int i = 0; i < n_words; ++i) {
    uint32_t k = w[i] * 0xcc9e2d51u;
    k = rotl(k, 15) * 0x1b873593u;
    h = rotl(h ^ k, 13) * 5u + 0xe6546b64u;
  }
  h ^= (uint32_t)(4 * n_words);
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  return h ^ (h >> 16);
}
static uint32_t murmur64(uint64_t k) {
  uint32_t w[2] = {(uint32_t)k, (uint32_t)(k >> 32)};
  return murmur(w, 2);
}

cref* cref_create(int V, const cref_desc* descs) {
  if (V < 1 || V > 64) return NULL;
  cref* c = (cref*)calloc(1, sizeof(cref));
  c->V = V;
  memcpy(c->d, descs, (size_t)V * sizeof(cref_desc));
  for (int v = 0; v < V; ++v) {
    if (descs[v].kind == 4) {
      int mx = 0, sh = 1;
      for (int i = 0; i < 256; ++i)
        if (descs[v].map[i] > mx) mx = descs[v].map[i];
      while ((1 << sh) <= mx) ++sh;
      c->shift[v] = sh;
    }
    if (descs[v].kind == 6) c->table[v] = (uint32_t*)calloc(descs[v].table_size, 4);
  }
  c->b.recent_bits = 1;
  c->b.first_prediction = 1;
  return c;
}

void cref_destroy(cref* c) {
  if (!c) return;
  for (int v = 0; v < c->V; ++v) free(c->table[v]);
  free(c);
}

static uint32_t recent_byte(const cref_board* b, int ago) {
  int pos = (int)b->rotating_history_pos - ago;
  if (pos < 0) pos += 1000;
  return b->rotating_history[pos];
}

/* Predict of one bit (the variables as the models see them), then the bit is perceived. */
static void step(cref* c, int bit) {
  cref_board* b = &c->b;
  int opening;
  if (b->first_prediction) {
    b->first_prediction = 0;  /* BasicContexts returns early: nothing of the blackboard moves */
  } else {
    b->recent_bits += b->recent_bits + b->new_bit;
    if (b->recent_bits >= 256) {
      b->last_byte = (uint32_t)b->recent_bits - 256;
      if (++b->rotating_history_pos == 1000) b->rotating_history_pos = 0;
      b->rotating_history[b->rotating_history_pos] = (uint8_t)b->last_byte;
      for (int i = 0; i < 10; ++i) b->recent_bytes[i] = recent_byte(b, i);
      b->recent_bits = 1;
    }
  }
  opening = b->recent_bits == 1;
  const uint32_t bc = (uint32_t)b->recent_bits - 1;
  for (int v = 0; v < c->V; ++v) {
    const cref_desc* d = &c->d[v];
    uint32_t* val = &b->values[v];
    switch (d->kind) {
      case 0: *val = 0; break;
      case 1: *val = bc; break;
      case 2: *val = b->recent_bytes[d->index]; break;
      case 3: *val = (b->recent_bytes[d->index] << 8) + bc; break;
      case 4:
        if (opening) {
          const uint32_t mask = (uint32_t)((1ull << d->num_bits) - 1);
          *val = mask & ((*val << c->shift[v]) + d->map[b->last_byte]);
        }
        break;
      case 5:
        if (opening) {
          uint64_t key = 0;
          for (int i = 0; i < d->n_bytes; ++i) key = (key << 8) + recent_byte(b, d->bytes_to_use[i]);
          *val = murmur64(key);
        }
        break;
      case 6:
        if (opening) {
          const uint64_t omod = 1ull << (8 * (d->outer_order - 1)), imod = 1ull << (8 * (d->inner_order - 1));
          uint32_t* e = &c->table[v][c->outer_hash[v] % d->table_size];
          *e = (uint32_t)(((*e % imod) << 8) + b->last_byte);
          c->outer_context[v] = ((c->outer_context[v] % omod) << 8) + b->last_byte;
          c->outer_hash[v] = murmur64(c->outer_context[v]);
          *val = murmur(&c->table[v][c->outer_hash[v] % d->table_size], 1);
        }
        break;
    }
  }
  b->new_bit = bit;
}

/* values: [T][V] or NULL */
void cref_run(cref* c, uint64_t T, const uint8_t* bits, uint32_t* values) {
  for (uint64_t t = 0; t < T; ++t) {
    step(c, bits[t]);
    if (values) memcpy(values + t * (uint64_t)c->V, c->b.values, (size_t)c->V * 4);
  }
}

void cref_board_get(const cref* c, cref_board* out) { *out = c->b; }
void cref_board_set(cref* c, const cref_board* in) { c->b = *in; }

/* IndirectHash::WriteToDisk of the hash variables in order; buf NULL: the size.  offsets [H + 1] nullable. */
uint64_t cref_export(const cref* c, uint8_t* buf, uint64_t* offsets) {
  uint64_t n = 0;
  int h = 0;
  for (int v = 0; v < c->V; ++v) {
    if (c->d[v].kind != 6) continue;
    const uint32_t size = c->d[v].table_size;
    uint32_t cnt = 0;
    for (uint32_t i = 0; i < size; ++i) cnt += c->table[v][i] != 0;
    if (offsets) offsets[h] = n;
    ++h;
    if (buf) memcpy(buf + n, &cnt, 4);
    n += 4;
    if (cnt < size / 2) {
      for (uint32_t i = 0; i < size; ++i)
        if (c->table[v][i]) {
          if (buf) {
            memcpy(buf + n, &i, 4);
            memcpy(buf + n + 4, &c->table[v][i], 4);
          }
          n += 8;
        }
    } else {
      if (buf) memcpy(buf + n, c->table[v], 4ull * size);
      n += 4ull * size;
    }
    if (buf) {
      memcpy(buf + n, &c->outer_context[v], 8);
      memcpy(buf + n + 8, &c->outer_hash[v], 4);
    }
    n += 12;
  }
  if (offsets) offsets[h] = n;
  return n;
}

/* IndirectHash::ReadFromDisk; 0, or -1 when the bytes do not fit the tables */
int cref_import(cref* c, const uint8_t* buf, uint64_t bytes) {
  uint64_t n = 0;
  for (int v = 0; v < c->V; ++v) {
    if (c->d[v].kind != 6) continue;
    const uint32_t size = c->d[v].table_size;
    uint32_t cnt;
    if (bytes - n < 4) return -1;
    memcpy(&cnt, buf + n, 4);
    n += 4;
    memset(c->table[v], 0, 4ull * size);
    if (cnt < size / 2) {
      if (bytes - n < 8ull * cnt) return -1;
      for (uint32_t i = 0; i < cnt; ++i, n += 8) {
        uint32_t key;
        memcpy(&key, buf + n, 4);
        if (key >= size) return -1;
        memcpy(&c->table[v][key], buf + n + 4, 4);
      }
    } else {
      if (bytes - n < 4ull * size) return -1;
      memcpy(c->table[v], buf + n, 4ull * size);
      n += 4ull * size;
    }
    if (bytes - n < 12) return -1;
    memcpy(&c->outer_context[v], buf + n, 8);
    memcpy(&c->outer_hash[v], buf + n + 8, 4);
    n += 12;
  }
  return n == bytes ? 0 : -1;
}
