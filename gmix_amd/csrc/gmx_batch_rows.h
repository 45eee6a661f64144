// gmx_batch_rows.h -- what the record batches of the six bank types (mixers, Indirect models, LSTM, Match models,
// context variables, PPMd) have in common, as far as it needs no HIP: the geometry of a transfer of the first records of
// every stream, and the table of a batch's columns with the declarations of the five tables.  The transfers
// themselves, their streams and their ordering are GmxBatchCore's in gmx_capi.cpp; a plain host program can drive
// what is here (tests/cpp/test_batch_rows.cpp).
#ifndef GMX_BATCH_ROWS_H_
#define GMX_BATCH_ROWS_H_

#include <stddef.h>
#include <stdint.h>

#include "../../include/gmxmix.h"

// The copy of the first n_rows records of every stream of an [S][max_rows][row_bytes] array: one block of `bytes`
// (height == 0) where the records wanted lie back to back, `height` rows of `width` bytes at `pitch` otherwise.
struct GmxRowCopy {
  size_t bytes, pitch, width, height;
};
static inline GmxRowCopy gmx_row_copy(int S, uint64_t max_rows, uint64_t n_rows, size_t row_bytes) {
  const size_t pitch = (size_t)max_rows * row_bytes, width = (size_t)n_rows * row_bytes;
  if (n_rows == max_rows || S == 1) return GmxRowCopy{S == 1 ? width : pitch * (size_t)S, pitch, width, 0};
  return GmxRowCopy{0, pitch, width, (size_t)S};
}

enum GmxColDir : uint8_t { GMX_COL_NONE, GMX_COL_UP, GMX_COL_DOWN };

// One array of a batch.  `dev` and `host` are the addresses of the owning struct's typed pointers (b->d_pred,
// b->h_pred): the launch code keeps reading those, the table is how the shared code finds them.
struct GmxBatchCol {
  void** dev;
  void** host;         // pinned staging; null: the array lives on the device only
  size_t row_bytes;    // 0: made by its own code when first needed; the table only frees it
  GmxColDir dir;       // which transfer carries it
  bool per_stream;     // one row per stream, copied whole behind the record columns ([S][row_bytes]: d_last)
  uint32_t extra_rows; // records allocated on the device behind the S * max_rows
};

struct GmxBatchCols {
  static const int kMax = 12;
  GmxBatchCol col[kMax];
  int n = 0;
  template <class D, class H>
  void add(D** dev, H** host, size_t row_bytes, GmxColDir dir, bool per_stream = false, uint32_t extra_rows = 0) {
    col[n++] = GmxBatchCol{(void**)dev, (void**)host, row_bytes, dir, per_stream, extra_rows};
  }
  template <class D>
  void add_device_only(D** dev) { col[n++] = GmxBatchCol{(void**)dev, nullptr, 0, GMX_COL_NONE, false, 0}; }
  const GmxBatchCol* begin() const { return col; }
  const GmxBatchCol* end() const { return col + n; }
};

// Bytes per record that an upload / a download moves: times S * n_rows, this is what decides whether the transfer
// takes a stream of its own.  (A per-stream column does not count: it is a few bytes whatever n_rows is.)
static inline size_t gmx_cols_row_bytes(const GmxBatchCols& t, GmxColDir dir) {
  size_t sum = 0;
  for (const GmxBatchCol& c : t)
    if (c.dir == dir && !c.per_stream) sum += c.row_bytes;
  return sum;
}
static inline size_t gmx_col_host_bytes(const GmxBatchCol& c, int S, uint64_t max_rows) {
  return (size_t)S * (c.per_stream ? 1 : (size_t)max_rows) * c.row_bytes;
}
static inline size_t gmx_col_dev_bytes(const GmxBatchCol& c, int S, uint64_t max_rows) {
  return gmx_col_host_bytes(c, S, max_rows) + (size_t)c.extra_rows * c.row_bytes;
}

// ---- the five tables, in the order their copies are issued.  B is the batch struct (a test passes a stand-in with
// the same members); a column that a flag switches off is not in the table, and its accessor returns null. -----------

template <class B>
static inline void gmx_mixer_batch_cols(GmxBatchCols& t, B* b, int n_pad, int m, int mask_words, unsigned flags) {
  t.add(&b->d_pred, &b->h_pred, (size_t)n_pad * 4, GMX_COL_UP);
  if (flags & GMX_BATCH_MASK) t.add(&b->d_mask, &b->h_mask, (size_t)mask_words * 4, GMX_COL_UP);
  // (+ one record: gmx_stock_kernel's plain build reads, and ignores, the context word behind its last bit)
  t.add(&b->d_ctx, &b->h_ctx, (size_t)m * 4, GMX_COL_UP, false, 1);
  t.add(&b->d_bits, &b->h_bits, 1, GMX_COL_UP);
  t.add(&b->d_p, &b->h_p, 4, GMX_COL_DOWN);
  if (flags & GMX_BATCH_OUTPUTS) t.add(&b->d_out, &b->h_out, (size_t)m * 4, GMX_COL_DOWN);
  if (flags & GMX_BATCH_LAST_OUTPUTS) t.add(&b->d_last, &b->h_last, (size_t)m * 4, GMX_COL_DOWN, true);
  // synthetic generator state (gmx_batch_fill_synthetic)
  t.add_device_only(&b->d_rng);
  t.add_device_only(&b->d_tcount);
  t.add_device_only(&b->d_pstate);
  t.add_device_only(&b->d_cstate);
}

template <class B>
static inline void gmx_ind_batch_cols(GmxBatchCols& t, B* b, int k) {
  t.add(&b->d_ctx, &b->h_ctx, (size_t)k * 4, GMX_COL_UP);
  t.add(&b->d_bc, &b->h_bc, 4, GMX_COL_UP);
  t.add(&b->d_bits, &b->h_bits, 1, GMX_COL_UP);
  t.add(&b->d_pred, &b->h_pred, (size_t)k * 8, GMX_COL_DOWN);
  t.add(&b->d_act, &b->h_act, (size_t)k * 2, GMX_COL_DOWN);
  // synthetic generator state: xorshift64, recent_bits, contexts (gmx_ind_batch_fill_synthetic)
  t.add_device_only(&b->d_rng);
  t.add_device_only(&b->d_recent);
  t.add_device_only(&b->d_cstate);
}

template <class B>
static inline void gmx_lstm_batch_cols(GmxBatchCols& t, B* b, int n_inputs) {
  t.add(&b->d_ppm, &b->h_ppm, (size_t)n_inputs * 4, GMX_COL_UP);
  t.add(&b->d_bytes, &b->h_bytes, 1, GMX_COL_UP);
  t.add(&b->d_pred, &b->h_pred, 8 * 4, GMX_COL_DOWN);
  t.add(&b->d_act, &b->h_act, 8, GMX_COL_DOWN);
  t.add(&b->d_ctx, &b->h_ctx, 4, GMX_COL_DOWN);
}

template <class B>
static inline void gmx_match_batch_cols(GmxBatchCols& t, B* b, int k) {
  t.add(&b->d_ctx, &b->h_ctx, (size_t)k * 4, GMX_COL_UP);
  t.add(&b->d_bc, &b->h_bc, 4, GMX_COL_UP);
  t.add(&b->d_bits, &b->h_bits, 1, GMX_COL_UP);
  t.add(&b->d_pred, &b->h_pred, (size_t)k * 4, GMX_COL_DOWN);
  t.add(&b->d_act, &b->h_act, (size_t)k, GMX_COL_DOWN);
  t.add(&b->d_long, &b->h_long, 4, GMX_COL_DOWN);
}

template <class B>
static inline void gmx_ctx_batch_cols(GmxBatchCols& t, B* b, int v, unsigned flags) {
  t.add(&b->d_bits, &b->h_bits, 1, GMX_COL_UP);
  if (flags & GMX_CTX_BATCH_VALUES) t.add(&b->d_values, &b->h_values, (size_t)v * 4, GMX_COL_DOWN);
  t.add_device_only(&b->d_scratch);  // [S][max_fires][H], made by gmx_ctx_batch_create
}

// The PPMd bank's records are bytes: the byte in; its distribution, the eight bit predictions with their flags and the
// model's memory usage out.
template <class B>
static inline void gmx_ppmd_batch_cols(GmxBatchCols& t, B* b) {
  t.add(&b->d_bytes, &b->h_bytes, 1, GMX_COL_UP);
  t.add(&b->d_ppm, &b->h_ppm, 256 * 4, GMX_COL_DOWN);
  t.add(&b->d_pred, &b->h_pred, 8 * 4, GMX_COL_DOWN);
  t.add(&b->d_act, &b->h_act, 8, GMX_COL_DOWN);
  t.add(&b->d_used, &b->h_used, 8, GMX_COL_DOWN);
}

#endif  // GMX_BATCH_ROWS_H_
