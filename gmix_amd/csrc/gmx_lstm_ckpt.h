// gmx_lstm_ckpt.h -- the checkpoint of a whole LSTM group on the device: the ONE description of how a bank
// (GmxLstmDev, gmx_internal.h) maps onto the reference's two files, and the arguments of the kernels that move the
// bytes (gmx_lstm_ckpt.hip), shared with their host side (gmx_lstm_ckpt.inc) and with tests/cpp/test_lstm_ckpt_layout.cpp.
//
// Two halves, each a run of 4-byte words:
//   long   the LSTM section of LongTermMemory::WriteToDisk (long-term-memory.cpp:57-67): lstm_output_layer
//          [epoch][symbol][hidden], then the three gates' weights [cell][563].  5 560 200 bytes.
//   short  LstmModel::WriteToDisk (lstm-model.cpp:62-68) and everything behind it, in the field order of
//          lstm_short_io (gmx_lstm.inc).  1 458 256 bytes.
// A half is a table of segments that tile it in file order.  A segment says where its words are in the bank:
//   plain        n consecutive floats
//   rows         `rows` rows of n floats, `pitch` floats apart in the bank (the [cell] vectors sit at pitch 64, the
//                layer inputs at 320)
//   cell_major   a reference [cell][563] matrix, in the bank input-major as gmx_l_mat(input, cell) has it
//   out_layer    [epoch][symbol][hidden] in the file, [epoch][hidden][symbol] in the bank
//   range        the 12 bytes top_ / mid_ / bot_: not in the bank; the host's per-stream record decides (below)
//   scal         u32 words of the bank's `scal` array (n of them), zero-extended to the file's width (update_steps is
//                a u64 in the file, one word in the bank)
// The kernels walk a half in tiles -- (segment, first) -- one block each, the same list for every stream.
//
// The segment table needs no GPU: it compiles with a plain C++ compiler (the test does that).
#ifndef GMX_LSTM_CKPT_H_
#define GMX_LSTM_CKPT_H_

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#include "gmx_internal.h"

#define GMX_LSTM_CKPT_LONG_BYTES \
  (((uint32_t)GMX_L_H * GMX_L_NO * GMX_L_HID + 3u * GMX_L_NC * GMX_L_W) * 4u)
#define GMX_LSTM_CKPT_GATE_FLOATS \
  ((uint32_t)GMX_L_NC + GMX_L_H + 8u * GMX_L_NC + GMX_L_H * GMX_L_NC + 3u * GMX_L_NC * GMX_L_W + \
   GMX_L_HID * GMX_L_NC + GMX_L_H * GMX_L_NC)
#define GMX_LSTM_CKPT_SHORT_BYTES                                                                              \
  (12u + 4u * ((uint32_t)GMX_L_NO + GMX_L_H + GMX_L_HID + GMX_L_NC + GMX_L_H * GMX_L_LIN + GMX_L_H * GMX_L_NO) + 4u + \
   4u * (3u * GMX_L_NC + 3u * GMX_L_H * GMX_L_NC) + 4u + 8u + 3u * 4u * GMX_LSTM_CKPT_GATE_FLOATS)
static_assert(GMX_LSTM_CKPT_LONG_BYTES == 5560200u && GMX_LSTM_CKPT_SHORT_BYTES == 1458256u, "the reference's sizes");

enum GmxLstmCkptKind : uint32_t {
  GMX_LCK_PLAIN = 0,
  GMX_LCK_ROWS = 1,
  GMX_LCK_CELL_MAJOR = 2,
  GMX_LCK_OUT_LAYER = 3,
  GMX_LCK_RANGE = 4,
  GMX_LCK_SCAL = 5,
};

#define GMX_LCK_NONE 0xffffffffu
struct GmxLstmCkptSeg {
  uint32_t file_off;   // bytes from the start of the stream's section
  uint32_t floats;     // 4-byte words of the file that the segment covers
  uint32_t kind;       // GmxLstmCkptKind
  uint32_t rows, n, pitch;  // rows: rows of n floats, pitch apart (plain: 1, floats, 0; scal: n words are the bank's)
  uint32_t one_at;     // import: the word of the segment that becomes 1.0f whatever the file says (GMX_LCK_NONE: none)
  uint32_t pad_;
  uint64_t bank_off;   // floats from the start of the bank (range: unused)
  uint64_t twin;       // import, rows: the bank's input-major copy [n][GMX_L_HP] of the same values (0: none)
};

// Tile lengths.  Element-parallel segments: GMX_LCK_TILE words of the file, `first` = the tile's first word inside the
// segment.  cell_major: GMX_LCK_JTILE inputs x every cell, `first` = the tile's first input (the symbol rows and the
// layer-input rows of gmx_l_mat never share a tile: 256 is a multiple of the tile).  out_layer: GMX_LCK_JTILE symbols
// x every hidden unit of one epoch, `first` = epoch * 256 + the tile's first symbol.
#define GMX_LCK_TILE 4096u
#define GMX_LCK_JTILE 64u
static_assert(GMX_L_NO % GMX_LCK_JTILE == 0 && GMX_LCK_JTILE % 4 == 0, "tiles respect gmx_l_mat's two parts");
struct GmxLstmCkptTile {
  uint32_t seg;
  uint32_t first;
};

#define GMX_LCK_MAX_SEGS 64
#define GMX_LCK_MAX_TILES 512
struct GmxLstmCkptHalf {
  uint32_t bytes;      // one stream's section
  uint32_t n_segs, n_tiles;
  uint32_t pad_;
  uint64_t scal;       // GmxLstmDev::scal
  GmxLstmCkptSeg seg[GMX_LCK_MAX_SEGS];
  GmxLstmCkptTile tile[GMX_LCK_MAX_TILES];
};

struct GmxLstmCkptLayout {
  GmxLstmCkptHalf half[2];  // 0: long, 1: short
  // byte offsets inside a short section of what the host reads itself at an import
  uint32_t off_probs, off_history, off_epoch, off_layer_epoch, off_update_steps;
};
#define GMX_LCK_LONG 0
#define GMX_LCK_SHORT 1

// Bank float offset of word k of a segment, ~0 where the bank has none (the range header, the upper half of
// update_steps).
__host__ __device__ inline uint64_t gmx_lstm_ckpt_bank(const GmxLstmCkptSeg& s, uint32_t k) {
  switch (s.kind) {
    case GMX_LCK_PLAIN:
      return s.bank_off + k;
    case GMX_LCK_ROWS:
      return s.bank_off + (uint64_t)(k / s.n) * s.pitch + k % s.n;
    case GMX_LCK_CELL_MAJOR:
      return s.bank_off + gmx_l_mat((int)(k % GMX_L_W), (int)(k / GMX_L_W));
    case GMX_LCK_OUT_LAYER: {
      const uint32_t j = k % GMX_L_HID, i = k / GMX_L_HID % GMX_L_NO, e = k / (GMX_L_HID * GMX_L_NO);
      return s.bank_off + ((uint64_t)e * GMX_L_HID + j) * GMX_L_NO + i;
    }
    case GMX_LCK_SCAL:
      return k < s.n ? s.bank_off + k : ~0ull;
    default:
      return ~0ull;
  }
}

// Builds both halves' segments and tiles.  false: a table is too small, or a half's size is not the reference's.
inline bool gmx_lstm_ckpt_layout(const GmxLstmDev& d, GmxLstmCkptLayout* out) {
  bool ok = true;
  for (int h = 0; h < 2; ++h) {
    GmxLstmCkptHalf& hf = out->half[h];
    hf.bytes = hf.n_segs = hf.n_tiles = hf.pad_ = 0;
    hf.scal = d.scal;
  }
  // appends a segment to a half and returns its byte offset
  auto add = [&ok](GmxLstmCkptHalf& hf, uint32_t kind, uint64_t bank_off, uint32_t floats, uint32_t rows, uint32_t n,
                   uint32_t pitch) -> uint32_t {
    const uint32_t at = hf.bytes;
    if (hf.n_segs >= GMX_LCK_MAX_SEGS) {
      ok = false;
      return at;
    }
    GmxLstmCkptSeg& s = hf.seg[hf.n_segs];
    s.file_off = at;
    s.floats = floats;
    s.kind = kind;
    s.rows = rows;
    s.n = n;
    s.pitch = pitch;
    s.one_at = GMX_LCK_NONE;
    s.pad_ = 0;
    s.bank_off = bank_off;
    s.twin = 0;
    // its tiles
    uint32_t step = GMX_LCK_TILE, end = floats;
    if (kind == GMX_LCK_CELL_MAJOR) {
      step = GMX_LCK_JTILE;
      end = GMX_L_W;
    } else if (kind == GMX_LCK_OUT_LAYER) {
      step = GMX_LCK_JTILE;
      end = GMX_L_H * GMX_L_NO;
    }
    for (uint32_t f = 0; f < end; f += step) {
      if (hf.n_tiles >= GMX_LCK_MAX_TILES) {
        ok = false;
        break;
      }
      hf.tile[hf.n_tiles].seg = hf.n_segs;
      hf.tile[hf.n_tiles].first = f;
      ++hf.n_tiles;
    }
    ++hf.n_segs;
    hf.bytes += floats * 4u;
    return at;
  };
  const uint32_t H = GMX_L_H, NC = GMX_L_NC, CP = GMX_L_CP, NO = GMX_L_NO, HID = GMX_L_HID;
  auto plain = [&](GmxLstmCkptHalf& hf, uint64_t at, uint32_t n) { return add(hf, GMX_LCK_PLAIN, at, n, 1, n, 0); };
  auto rows = [&](GmxLstmCkptHalf& hf, uint64_t at, uint32_t r, uint32_t n, uint32_t pitch) {
    return add(hf, GMX_LCK_ROWS, at, r * n, r, n, pitch);
  };
  auto cell_major = [&](GmxLstmCkptHalf& hf, uint64_t at) {
    return add(hf, GMX_LCK_CELL_MAJOR, at, NC * GMX_L_W, NC, GMX_L_W, 0);
  };

  GmxLstmCkptHalf& lg = out->half[GMX_LCK_LONG];
  add(lg, GMX_LCK_OUT_LAYER, d.out_layer, H * NO * HID, H * NO, HID, 0);
  for (int g = 0; g < 3; ++g) cell_major(lg, d.gate[g].weights);

  GmxLstmCkptHalf& sh = out->half[GMX_LCK_SHORT];
  add(sh, GMX_LCK_RANGE, 0, 3, 1, 0, 0);
  out->off_probs = plain(sh, d.probs, NO);
  out->off_history = plain(sh, d.input_history, H);
  plain(sh, d.hidden, HID);
  if (ok) sh.seg[sh.n_segs - 1].one_at = HID - 1;  // hidden_[50] (lstm.cpp:31), the bias input
  plain(sh, d.hidden_error, NC);
  rows(sh, d.layer_input, H, GMX_L_LIN, GMX_L_LINP);
  if (ok) sh.seg[sh.n_segs - 1].twin = d.lin_t;
  rows(sh, d.output, H, NO, NO);
  out->off_epoch = add(sh, GMX_LCK_SCAL, d.scal + 0, 1, 1, 1, 0);
  plain(sh, d.state, NC);
  plain(sh, d.state_error, NC);
  plain(sh, d.stored_error, NC);
  rows(sh, d.tanh_state, H, NC, CP);
  rows(sh, d.input_gate_state, H, NC, CP);
  rows(sh, d.last_state, H, NC, CP);
  out->off_layer_epoch = add(sh, GMX_LCK_SCAL, d.scal + 1, 1, 1, 1, 0);
  out->off_update_steps = add(sh, GMX_LCK_SCAL, d.scal + 2, 2, 1, 1, 0);
  for (int g = 0; g < 3; ++g) {
    const GmxLstmGateOff& o = d.gate[g];
    plain(sh, d.errs + (uint64_t)g * H * CP, NC);  // error_: epoch 0 of the last backward pass (lstm-layer.cpp:311-316)
    plain(sh, o.ivar, H);
    const uint64_t vecs[] = {o.gamma, o.gamma_u, o.gamma_m, o.gamma_v, o.beta, o.beta_u, o.beta_m, o.beta_v};
    for (uint64_t v : vecs) plain(sh, v, NC);
    rows(sh, o.state, H, NC, CP);
    cell_major(sh, o.update);
    cell_major(sh, o.m);
    cell_major(sh, o.v);
    rows(sh, o.transpose, HID, NC, CP);
    rows(sh, o.norm, H, NC, CP);
  }
  return ok && lg.bytes == GMX_LSTM_CKPT_LONG_BYTES && sh.bytes == GMX_LSTM_CKPT_SHORT_BYTES;
}

// ---- the kernels' arguments ------------------------------------------------------------------------------------

// Export, short half: how the stream's 12-byte range header comes about (gmx_lstm_export's rules).  fixed != 0: tmb
// as given -- what a file said while nothing has moved since, or 255 / 127 / 0 between a forward and its perceive;
// fixed == 0: the kernel derives it from the bank -- [b & ~1, b | 1] with mid_ = bot_ once a byte has been coded
// (scal[6], b = scal[3]), else 255 / 127 / 0.
struct GmxLstmCkptOut {
  uint32_t fixed;
  int32_t tmb[3];
};
// Import, short half: scal[0 .. 6] as the host has computed them (both epochs, steps, last byte, arg-max context,
// the bit prediction -- the host's logf --, "a byte has been coded").
struct GmxLstmCkptIn {
  uint32_t scal[8];
};

struct GmxLstmCkptArgs {
  uint32_t* banks;               // bank of the launch's stream 0, as words: values travel as bit patterns
  uint64_t bank_floats;
  const GmxLstmCkptHalf* half;   // device copy of the half the launch moves
  uint32_t n_tiles;              // the host's copy of half->n_tiles
  int32_t n_streams;             // streams of the launch
  uint8_t* buf;                  // packed sections: the launch's stream i at buf + i * stride, 4-byte aligned
  uint64_t stride;
  const GmxLstmCkptOut* out;     // pack, short half: [n_streams]
  const GmxLstmCkptIn* in;       // scatter, short half: [n_streams]
};

#endif  // GMX_LSTM_CKPT_H_
