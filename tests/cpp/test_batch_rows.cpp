// What the record batches of the five bank types share off the GPU (gmix_amd/csrc/gmx_batch_rows.h): the geometry of
// a transfer of the first records of every stream, replayed here with memcpy on two byte arrays, and the five column
// tables, whose per-direction byte sums (they decide when a transfer takes a stream of its own) and allocation sizes
// are compared with the expressions the five hand-written copies of the batch code used.  No GPU, no HIP.
//   g++ -std=c++17 -Wall -I gmix_amd/csrc tests/cpp/test_batch_rows.cpp && ./a.out
#include "gmx_batch_rows.h"

#include <stdio.h>
#include <string.h>

#include <vector>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#include "gmx_internal.h"  // GMX_L_NI

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      return 1;                                                   \
    }                                                             \
  } while (0)

// ---- the geometry ---------------------------------------------------------------------------------------------
static int test_geometry() {
  const size_t widths[] = {1, 4, 29, 132};
  const uint8_t kUntouched = 0xff;  // (the source holds 0 .. 250)
  int cases = 0;
  for (int S = 1; S <= 4; ++S)
    for (uint64_t max_rows = 1; max_rows <= 9; ++max_rows)
      for (uint64_t n_rows = 0; n_rows <= max_rows; ++n_rows)
        for (size_t rb : widths) {
          const size_t total = (size_t)S * max_rows * rb;
          std::vector<uint8_t> src(total), dst(total, kUntouched), want(total, kUntouched);
          for (size_t i = 0; i < total; ++i) src[i] = (uint8_t)((i * 7 + i / 251) % 251);
          for (int s = 0; s < S; ++s)
            for (uint64_t r = 0; r < n_rows; ++r) {
              const size_t at = ((size_t)s * max_rows + r) * rb;
              memcpy(&want[at], &src[at], rb);
            }
          const GmxRowCopy c = gmx_row_copy(S, max_rows, n_rows, rb);
          const bool one_block = n_rows == max_rows || S == 1;
          CHECK((c.height == 0) == one_block);
          if (c.height == 0) {
            CHECK(c.bytes == (S == 1 ? n_rows * rb : total));
            CHECK(c.bytes <= total);
            memcpy(dst.data(), src.data(), c.bytes);
          } else {
            CHECK(c.height == (size_t)S && c.pitch == max_rows * rb && c.width == n_rows * rb);
            CHECK((c.height - 1) * c.pitch + c.width <= total);
            for (size_t h = 0; h < c.height; ++h) memcpy(&dst[h * c.pitch], &src[h * c.pitch], c.width);
          }
          // exactly the first n_rows records of every stream, and no other byte (one block over S > 1 streams is the
          // whole array: n_rows == max_rows there, so `want` is the whole source too)
          CHECK(dst == want);
          ++cases;
        }
  printf("ok: row copies, %d shapes\n", cases);
  return 0;
}

// ---- the tables: stand-ins with the members of the five batch structs -------------------------------------------
struct MixerBatch {
  float *d_pred, *d_p, *d_out, *d_last, *d_pstate, *h_pred, *h_p, *h_out, *h_last;
  uint32_t *d_mask, *d_ctx, *d_cstate, *h_mask, *h_ctx;
  uint8_t *d_bits, *h_bits;
  uint64_t *d_rng, *d_tcount;
};
struct IndBatch {
  uint32_t *d_ctx, *d_bc, *d_recent, *d_cstate, *h_ctx, *h_bc;
  uint8_t *d_bits, *d_act, *h_bits, *h_act;
  float *d_pred, *h_pred;
  uint64_t* d_rng;
};
struct LstmBatch {
  float *d_ppm, *d_pred, *h_ppm, *h_pred;
  uint8_t *d_bytes, *d_act, *h_bytes, *h_act;
  uint32_t *d_ctx, *h_ctx;
};
struct MatchBatch {
  uint32_t *d_ctx, *d_bc, *d_long, *h_ctx, *h_bc, *h_long;
  uint8_t *d_bits, *d_act, *h_bits, *h_act;
  float *d_pred, *h_pred;
};
struct CtxBatch {
  uint8_t *d_bits, *h_bits;
  uint32_t *d_values, *d_scratch, *h_values;
};

static const int kS = 3;
static const uint64_t kMax = 5;
static const size_t R = (size_t)kS * kMax;

static const GmxBatchCol* find(const GmxBatchCols& t, const void* dev_slot) {
  for (const GmxBatchCol& c : t)
    if ((const void*)c.dev == dev_slot) return &c;
  return nullptr;
}
// the column of `dev_slot`: its device bytes, its pinned bytes (0 bytes for a device-only array), its direction
static bool col_is(const GmxBatchCols& t, const void* dev_slot, const void* host_slot, size_t dev_bytes,
                   size_t host_bytes, GmxColDir dir) {
  const GmxBatchCol* c = find(t, dev_slot);
  if (!c || (const void*)c->host != host_slot || c->dir != dir) return false;
  return gmx_col_dev_bytes(*c, kS, kMax) == dev_bytes && (!c->host || gmx_col_host_bytes(*c, kS, kMax) == host_bytes);
}
static bool order_is(const GmxBatchCols& t, std::vector<const void*> dev_slots) {
  if ((size_t)t.n != dev_slots.size()) return false;
  for (int i = 0; i < t.n; ++i)
    if ((const void*)t.col[i].dev != dev_slots[(size_t)i]) return false;
  return true;
}

static int test_mixers() {
  const size_t n_pad = 8, m = 3, mw = 1;
  for (unsigned mask = 0; mask < 2; ++mask)
    for (unsigned outs = 0; outs < 2; ++outs)
      for (unsigned last = 0; last < 2; ++last) {
        const unsigned flags =
            (mask ? GMX_BATCH_MASK : 0u) | (outs ? GMX_BATCH_OUTPUTS : 0u) | (last ? GMX_BATCH_LAST_OUTPUTS : 0u);
        MixerBatch b = {};
        GmxBatchCols t;
        gmx_mixer_batch_cols(t, &b, (int)n_pad, (int)m, (int)mw, flags);
        CHECK(gmx_cols_row_bytes(t, GMX_COL_UP) == n_pad * 4 + m * 4 + 1 + (mask ? mw * 4 : 0));
        CHECK(gmx_cols_row_bytes(t, GMX_COL_DOWN) == 4 + (outs ? m * 4 : 0));  // (the last outputs do not count)
        CHECK(col_is(t, &b.d_pred, &b.h_pred, R * n_pad * 4, R * n_pad * 4, GMX_COL_UP));
        CHECK(mask ? col_is(t, &b.d_mask, &b.h_mask, R * mw * 4, R * mw * 4, GMX_COL_UP) : !find(t, &b.d_mask));
        CHECK(col_is(t, &b.d_ctx, &b.h_ctx, (R + 1) * m * 4, R * m * 4, GMX_COL_UP));  // the extra context record
        CHECK(col_is(t, &b.d_bits, &b.h_bits, R, R, GMX_COL_UP));
        CHECK(col_is(t, &b.d_p, &b.h_p, R * 4, R * 4, GMX_COL_DOWN));
        CHECK(outs ? col_is(t, &b.d_out, &b.h_out, R * m * 4, R * m * 4, GMX_COL_DOWN) : !find(t, &b.d_out));
        CHECK(last ? col_is(t, &b.d_last, &b.h_last, kS * m * 4, kS * m * 4, GMX_COL_DOWN) : !find(t, &b.d_last));
        CHECK(!last || find(t, &b.d_last)->per_stream);
        std::vector<const void*> order = {&b.d_pred};
        if (mask) order.push_back(&b.d_mask);
        order.insert(order.end(), {&b.d_ctx, &b.d_bits, &b.d_p});
        if (outs) order.push_back(&b.d_out);
        if (last) order.push_back(&b.d_last);
        order.insert(order.end(), {&b.d_rng, &b.d_tcount, &b.d_pstate, &b.d_cstate});
        CHECK(order_is(t, order));
        for (const void* s : {(const void*)&b.d_rng, (const void*)&b.d_tcount, (const void*)&b.d_pstate,
                              (const void*)&b.d_cstate})
          CHECK(col_is(t, s, nullptr, 0, 0, GMX_COL_NONE));  // made by the generator's first call, freed by the table
      }
  printf("ok: mixer table, 8 flag combinations\n");
  return 0;
}

static int test_indirect() {
  const size_t k = 3;
  IndBatch b = {};
  GmxBatchCols t;
  gmx_ind_batch_cols(t, &b, (int)k);
  CHECK(gmx_cols_row_bytes(t, GMX_COL_UP) == 4 * k + 5);
  CHECK(gmx_cols_row_bytes(t, GMX_COL_DOWN) == 10 * k);
  CHECK(col_is(t, &b.d_ctx, &b.h_ctx, R * k * 4, R * k * 4, GMX_COL_UP));
  CHECK(col_is(t, &b.d_bc, &b.h_bc, R * 4, R * 4, GMX_COL_UP));
  CHECK(col_is(t, &b.d_bits, &b.h_bits, R, R, GMX_COL_UP));
  CHECK(col_is(t, &b.d_pred, &b.h_pred, R * 2 * k * 4, R * 2 * k * 4, GMX_COL_DOWN));
  CHECK(col_is(t, &b.d_act, &b.h_act, R * 2 * k, R * 2 * k, GMX_COL_DOWN));
  CHECK(order_is(t, {&b.d_ctx, &b.d_bc, &b.d_bits, &b.d_pred, &b.d_act, &b.d_rng, &b.d_recent, &b.d_cstate}));
  for (const void* s : {(const void*)&b.d_rng, (const void*)&b.d_recent, (const void*)&b.d_cstate})
    CHECK(col_is(t, s, nullptr, 0, 0, GMX_COL_NONE));
  printf("ok: Indirect table, k = 3\n");
  return 0;
}

static int test_lstm() {
  LstmBatch b = {};
  GmxBatchCols t;
  gmx_lstm_batch_cols(t, &b, GMX_L_NI);
  CHECK(gmx_cols_row_bytes(t, GMX_COL_UP) == GMX_L_NI * 4 + 1);
  CHECK(gmx_cols_row_bytes(t, GMX_COL_DOWN) == 44);
  CHECK(col_is(t, &b.d_ppm, &b.h_ppm, R * GMX_L_NI * 4, R * GMX_L_NI * 4, GMX_COL_UP));
  CHECK(col_is(t, &b.d_bytes, &b.h_bytes, R, R, GMX_COL_UP));
  CHECK(col_is(t, &b.d_pred, &b.h_pred, R * 8 * 4, R * 8 * 4, GMX_COL_DOWN));
  CHECK(col_is(t, &b.d_act, &b.h_act, R * 8, R * 8, GMX_COL_DOWN));
  CHECK(col_is(t, &b.d_ctx, &b.h_ctx, R * 4, R * 4, GMX_COL_DOWN));
  CHECK(order_is(t, {&b.d_ppm, &b.d_bytes, &b.d_pred, &b.d_act, &b.d_ctx}));
  printf("ok: LSTM table\n");
  return 0;
}

static int test_match() {
  const size_t k = 2;
  MatchBatch b = {};
  GmxBatchCols t;
  gmx_match_batch_cols(t, &b, (int)k);
  CHECK(gmx_cols_row_bytes(t, GMX_COL_UP) == 4 * k + 5);
  CHECK(gmx_cols_row_bytes(t, GMX_COL_DOWN) == 5 * k + 4);
  CHECK(col_is(t, &b.d_ctx, &b.h_ctx, R * k * 4, R * k * 4, GMX_COL_UP));
  CHECK(col_is(t, &b.d_bc, &b.h_bc, R * 4, R * 4, GMX_COL_UP));
  CHECK(col_is(t, &b.d_bits, &b.h_bits, R, R, GMX_COL_UP));
  CHECK(col_is(t, &b.d_pred, &b.h_pred, R * k * 4, R * k * 4, GMX_COL_DOWN));
  CHECK(col_is(t, &b.d_act, &b.h_act, R * k, R * k, GMX_COL_DOWN));
  CHECK(col_is(t, &b.d_long, &b.h_long, R * 4, R * 4, GMX_COL_DOWN));
  CHECK(order_is(t, {&b.d_ctx, &b.d_bc, &b.d_bits, &b.d_pred, &b.d_act, &b.d_long}));
  printf("ok: Match table, k = 2\n");
  return 0;
}

static int test_ctx() {
  const size_t v = 5;
  for (unsigned values = 0; values < 2; ++values) {
    CtxBatch b = {};
    GmxBatchCols t;
    gmx_ctx_batch_cols(t, &b, (int)v, values ? GMX_CTX_BATCH_VALUES : 0u);
    CHECK(gmx_cols_row_bytes(t, GMX_COL_UP) == 1);
    CHECK(gmx_cols_row_bytes(t, GMX_COL_DOWN) == (values ? v * 4 : 0));
    CHECK(col_is(t, &b.d_bits, &b.h_bits, R, R, GMX_COL_UP));
    CHECK(values ? col_is(t, &b.d_values, &b.h_values, R * v * 4, R * v * 4, GMX_COL_DOWN) : !find(t, &b.d_values));
    CHECK(col_is(t, &b.d_scratch, nullptr, 0, 0, GMX_COL_NONE));  // sized by max_fires, by the batch's create
    CHECK(t.n == (values ? 3 : 2) && (const void*)t.col[0].dev == &b.d_bits &&
          (const void*)t.col[t.n - 1].dev == &b.d_scratch);
  }
  printf("ok: context table, v = 5, with and without values\n");
  return 0;
}

int main() {
  if (test_geometry() || test_mixers() || test_indirect() || test_lstm() || test_match() || test_ctx()) return 1;
  return 0;
}
