/* gmxmix_lstm_shape.h -- a device LSTM bank for an Lstm(...) line other than the stock one: an extension of
 * include/gmxmix.h, which it includes.  libgmxmix.so exports these functions; they are declared here, not in gmxmix.h,
 * whose list of entry points is pinned by the project's ABI tests.  DESIGN.md section 4.21.
 *
 * The reference builds Lstm(256, 256, 50, 1, 100, 0.03, 10, ...) (models/lstm-model.cpp:7) and gmx_lstm_create gives
 * exactly that.  gmx_lstm_create_shaped takes num_cells, horizon, learning_rate and gradient_clip from the caller and
 * is bit-exact with the reference's Lstm at that shape: one layer, 256 inputs, 256 outputs, update_limit 3000.
 *
 * num_layers > 1 is NOT supported: the reference's LstmLayer constructor writes its random draw into
 * neuron_layer_weights[0..2] for every layer (lstm-layer.cpp:182-195), so the gates of a second layer start at zero,
 * and nobody runs that configuration. */
#ifndef GMXMIX_LSTM_SHAPE_H_
#define GMXMIX_LSTM_SHAPE_H_

#include "gmxmix.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gmx_lstm_shape {
  int32_t num_cells, horizon;          /* 1 .. 256, 2 .. 256 */
  float learning_rate, gradient_clip;  /* finite, > 0 */
} gmx_lstm_shape;

/* 1 if gmx_lstm_create_shaped accepts the shape, else 0.  Host code: no device is touched. */
int gmx_lstm_shape_supported(const gmx_lstm_shape* shape);

/* gmx_lstm_create for a shape.  GMX_ERR_INVALID for an unsupported shape, before anything is allocated.
 * {50, 100, 0.03f, 10.0f} gives the very object gmx_lstm_create makes: same layout, same kernels, every surface.
 * Any other shape runs the general kernel, and the extents of the arrays follow the shape:
 *   gmx_lstm_set_weights / _get_weights   weights [3][num_cells][512 + num_cells + 1],
 *                                         output_layer [horizon][256][num_cells + 1];
 *   gmx_lstm_export / _import             the reference's own `.long` / `.short` bytes at that shape;
 *   gmx_lstm_bank_bytes, gmx_lstm_memory_usage   the shape's figures (LstmModel::GetMemoryUsage evaluated at it).
 * On such a bank gmx_lstm_reset, _sync, _set_cu_mask, _set_weights, _get_weights, gmx_lstm_batch_*, gmx_lstm_run,
 * gmx_lstm_run_ragged, gmx_lstm_feed, gmx_lstm_forward / _perceive (one launch per call, never a per-byte session),
 * gmx_lstm_export / _import / _copy (between banks of the same shape; else GMX_ERR_INVALID) and
 * gmx_lstm_memory_usage work.  gmx_chainstep_create and gmx_lstm_group_export / _import return GMX_ERR_INVALID for
 * it and leave it untouched. */
int gmx_lstm_create_shaped(gmx_lstm** out, const gmx_lstm_shape* shape, int n_streams, int device);

/* The shape of a bank; {50, 100, 0.03f, 10.0f} for one made by gmx_lstm_create. */
int gmx_lstm_get_shape(const gmx_lstm* l, gmx_lstm_shape* out);

/* How many times the general kernel has been launched for this bank (tests): stays 0 on a stock bank unless the
 * environment held GMX_LSTM_BUILD=any when it was created, which gives a stock-shape bank the general layout and
 * kernel (and the refusals above). */
int64_t gmx_debug_lstm_any_launches(const gmx_lstm* l);

#ifdef __cplusplus
}
#endif
#endif /* GMXMIX_LSTM_SHAPE_H_ */
