// gmx_lstm_any.h -- the LSTM byte model at a shape given at run time (gmx_lstm_create_shaped):
// what gmx_lstm_any.hip and the host side (gmx_lstm_any.inc) share.  The stock shape's structs and macros
// (gmx_internal.h, GMX_L_*) are untouched: its kernels read them at compile time.
#ifndef GMX_LSTM_ANY_H_
#define GMX_LSTM_ANY_H_

#include <stdint.h>

#include "gmx_internal.h"

#define GMX_LA_MAX_CELLS 256
#define GMX_LA_MAX_HORIZON 256
#define GMX_LA_UPDATE_LIMIT 3000

// One stream's bank: the float offsets of GmxLstmDev (lin_t and errs are not part of this layout and stay 0) with the
// extents the kernel loops over.  Every [cell] vector is padded to cp floats, cp = num_cells rounded up to 64.  The gate
// matrices (weights, update_, m_, v_) are plain input-major [w][cp]: row j = input j (the 256 one-hot symbol columns
// first, then the lin layer inputs), so that the chains of neighbouring cells read one coalesced row per step.
// out_layer is [h][hid][256], hidden [hidp], layer_input [h][linp], transpose [hid][cp].
struct GmxLstmAnyDev {
  GmxLstmDev o;
  int32_t nc, h;        // num_cells, horizon
  int32_t cp;           // cell pitch
  int32_t lin, linp;    // 256 + nc + 1 layer inputs, and their pitch
  int32_t hid, hidp;    // nc + 1, and its pitch
  int32_t w;            // 256 + lin columns of a gate matrix
  float lr, clip;       // learning_rate, gradient_clip
};

#endif  // GMX_LSTM_ANY_H_
