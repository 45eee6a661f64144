// The LSTM group checkpoint's layout description (gmix_amd/csrc/gmx_lstm_ckpt.h) without a GPU: the segment tables
// that the kernels of gmx_lstm_ckpt.hip walk, built over a fabricated GmxLstmDev whose arrays lie in an order of their
// own with gaps between them, against the file layouts restated here independently.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "gmx_lstm_ckpt.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      exit(1);                                                    \
    }                                                             \
  } while (0)

// what an array occupies in a bank, padding included
struct Room {
  uint64_t at, size;
  int kind;  // 0: dense; 1: rows at pitch CP, cells >= 50 padding; 2: rows at pitch LINP, inputs >= 307 padding;
             // 3: gmx_l_mat
};
static std::vector<Room> rooms;

static GmxLstmDev fabricate() {
  GmxLstmDev d;
  uint64_t off = 192;  // (nothing at 0: an offset that was never set shows)
  auto take = [&off](uint64_t n, int kind) {
    const uint64_t o = off;
    rooms.push_back(Room{o, n, kind});
    off += (n + 63) / 64 * 64 + 64 * (1 + rooms.size() % 3);  // distinct, non-overlapping, gaps of varying length
    return o;
  };
  const uint64_t H = GMX_L_H, CP = GMX_L_CP;
  // (not the product's order)
  d.scal = take(16, 0);
  d.probs = take(GMX_L_NO, 0);
  d.input_history = take(H, 0);
  d.output = take(H * GMX_L_NO, 0);
  d.errs = take(3 * H * CP, 1);
  d.lin_t = take((uint64_t)GMX_L_LIN * GMX_L_HP, 0);
  d.layer_input = take(H * GMX_L_LINP, 2);
  d.hidden_error = take(CP, 1);
  d.hidden = take(CP, 0);
  d.last_state = take(H * CP, 1);
  d.input_gate_state = take(H * CP, 1);
  d.tanh_state = take(H * CP, 1);
  d.stored_error = take(CP, 1);
  d.state_error = take(CP, 1);
  d.state = take(CP, 1);
  for (int g = 2; g >= 0; --g) {
    GmxLstmGateOff& o = d.gate[g];
    o.transpose = take((uint64_t)GMX_L_HID * CP, 1);
    o.ivar = take(H, 0);
    o.norm = take(H * CP, 1);
    o.state = take(H * CP, 1);
    uint64_t* vecs[] = {&o.error, &o.beta_v, &o.beta_m, &o.beta_u, &o.beta, &o.gamma_v, &o.gamma_m, &o.gamma_u, &o.gamma};
    for (uint64_t* p : vecs) *p = take(CP, 1);
    o.v = take(GMX_L_MAT_FLOATS, 3);
    o.m = take(GMX_L_MAT_FLOATS, 3);
    o.update = take(GMX_L_MAT_FLOATS, 3);
    o.weights = take(GMX_L_MAT_FLOATS, 3);
  }
  d.out_layer = take(H * GMX_L_HID * GMX_L_NO, 0);
  d.bank_floats = off;
  return d;
}

// the restated gmx_l_mat: 256 symbol rows of 64 cells, then blocks of four layer inputs, [block][cell][4]
static uint64_t l_mat(int j, int c) {
  if (j < 256) return (uint64_t)j * 64 + c;
  const int r = j - 256;
  return 256ull * 64 + ((uint64_t)(r / 4) * 64 + c) * 4 + r % 4;
}

static bool is_padding(uint64_t bank) {
  for (const Room& r : rooms) {
    if (bank < r.at || bank >= r.at + r.size) continue;
    const uint64_t k = bank - r.at;
    if (r.kind == 1) return k % GMX_L_CP >= GMX_L_NC;
    if (r.kind == 2) return k % GMX_L_LINP >= GMX_L_LIN;
    if (r.kind == 3) {
      if (k < 256ull * 64) return k % 64 >= GMX_L_NC;
      const uint64_t q = k - 256ull * 64, c = q / 4 % 64, j = q / 256 * 4 + q % 4;
      return c >= GMX_L_NC || j >= (uint64_t)GMX_L_LIN;
    }
    return false;
  }
  return true;  // between the arrays
}

// file word -> bank float of a half through the table, ~0 where the bank has none
static std::vector<uint64_t> file_map(const GmxLstmCkptHalf& hf) {
  std::vector<uint64_t> m(hf.bytes / 4, ~0ull - 1);
  for (uint32_t i = 0; i < hf.n_segs; ++i) {
    const GmxLstmCkptSeg& s = hf.seg[i];
    for (uint32_t k = 0; k < s.floats; ++k) m[s.file_off / 4 + k] = gmx_lstm_ckpt_bank(s, k);
  }
  return m;
}

int main() {
  const GmxLstmDev d = fabricate();
  static GmxLstmCkptLayout lay;
  CHECK(gmx_lstm_ckpt_layout(d, &lay));

  // ---- the segments tile both sections exactly, in order; the tiles cover every segment, in order
  const uint32_t sizes[2] = {5560200u, 1458256u};
  for (int h = 0; h < 2; ++h) {
    const GmxLstmCkptHalf& hf = lay.half[h];
    CHECK(hf.bytes == sizes[h] && hf.scal == d.scal);
    CHECK(hf.n_segs > 0 && hf.n_segs <= GMX_LCK_MAX_SEGS && hf.n_tiles > 0 && hf.n_tiles <= GMX_LCK_MAX_TILES);
    uint32_t at = 0, t = 0;
    for (uint32_t i = 0; i < hf.n_segs; ++i) {
      const GmxLstmCkptSeg& s = hf.seg[i];
      CHECK(s.file_off == at && s.floats > 0 && s.file_off % 4 == 0);
      at += 4 * s.floats;
      if (s.kind == GMX_LCK_ROWS || s.kind == GMX_LCK_PLAIN) CHECK(s.rows * s.n == s.floats && (s.rows == 1 || s.pitch >= s.n));
      // its tiles: consecutive, from 0, a fixed step, to the segment's end
      const uint32_t step = s.kind == GMX_LCK_CELL_MAJOR || s.kind == GMX_LCK_OUT_LAYER ? GMX_LCK_JTILE : GMX_LCK_TILE;
      const uint32_t end = s.kind == GMX_LCK_CELL_MAJOR ? 563u : s.kind == GMX_LCK_OUT_LAYER ? 100u * 256u : s.floats;
      for (uint32_t f = 0; f < end; f += step, ++t) CHECK(t < hf.n_tiles && hf.tile[t].seg == i && hf.tile[t].first == f);
    }
    CHECK(at == sizes[h] && t == hf.n_tiles);
  }
  printf("ok: segments and tiles tile [0, 5 560 200) and [0, 1 458 256) in order\n");

  // ---- injective, inside the bank, never on padding
  const std::vector<uint64_t> lm = file_map(lay.half[GMX_LCK_LONG]), sm = file_map(lay.half[GMX_LCK_SHORT]);
  {
    std::vector<uint8_t> hit(d.bank_floats, 0);
    size_t none = 0;
    for (const std::vector<uint64_t>* m : {&lm, &sm})
      for (uint64_t b : *m) {
        CHECK(b != ~0ull - 1);  // every file word belongs to a segment
        if (b == ~0ull) {
          ++none;
          continue;
        }
        CHECK(b < d.bank_floats);
        CHECK(!hit[b]);
        hit[b] = 1;
        CHECK(!is_padding(b));
      }
    CHECK(none == 4);  // top_, mid_, bot_ and the upper half of update_steps
    // and nothing of lin_t, which the file leaves implicit, is mapped
    for (uint64_t k = 0; k < (uint64_t)GMX_L_LIN * GMX_L_HP; ++k) CHECK(!hit[d.lin_t + k]);
  }
  printf("ok: file word -> bank float is injective, below bank_floats and never on padding\n");

  // ---- spot formulas, restated
  for (uint32_t e = 0; e < 100; e += 9)
    for (uint32_t i = 0; i < 256; i += 5)
      for (uint32_t j = 0; j < 51; ++j) CHECK(lm[(e * 256 + i) * 51 + j] == d.out_layer + (e * 51ull + j) * 256 + i);
  CHECK(lm[(99u * 256 + 255) * 51 + 50] == d.out_layer + (99 * 51ull + 50) * 256 + 255);
  for (int g = 0; g < 3; ++g)
    for (int c = 0; c < 50; ++c)
      for (int j = 0; j < 563; ++j)
        CHECK(lm[100u * 256 * 51 + ((uint32_t)g * 50 + c) * 563 + j] == d.gate[g].weights + l_mat(j, c));
  CHECK(sm[0] == ~0ull && sm[1] == ~0ull && sm[2] == ~0ull);
  CHECK(sm[3] == d.probs && sm[3 + 256] == d.input_history && sm[3 + 356] == d.hidden && sm[3 + 356 + 50] == d.hidden + 50);
  CHECK(sm[3 + 407] == d.hidden_error);
  CHECK(sm[3 + 457 + 3 * 307 + 306] == d.layer_input + 3 * 320 + 306);
  CHECK(lay.off_epoch == 227040 && sm[227040 / 4] == d.scal + 0);
  CHECK(lay.off_layer_epoch == 287644 && sm[287644 / 4] == d.scal + 1);
  CHECK(lay.off_update_steps == 287648 && sm[287648 / 4] == d.scal + 2 && sm[287648 / 4 + 1] == ~0ull);
  CHECK(lay.off_probs == 12 && lay.off_history == 12 + 1024);
  CHECK(sm[227044 / 4] == d.state && sm[227044 / 4 + 150 + 7 * 50 + 49] == d.tanh_state + 7 * 64 + 49);
  {
    // a gate's stretch: error_, ivar, eight vectors, state, update, m, v, transpose, norm
    const uint32_t gate_floats = 50 + 100 + 8 * 50 + 5000 + 3 * 28150 + 51 * 50 + 5000;
    for (int g = 0; g < 3; ++g) {
      const uint32_t g0 = 287656 / 4 + (uint32_t)g * gate_floats;
      const GmxLstmGateOff& o = d.gate[g];
      CHECK(sm[g0] == d.errs + (uint64_t)g * 100 * 64 && sm[g0 + 50] == o.ivar && sm[g0 + 150] == o.gamma);
      CHECK(sm[g0 + 150 + 7 * 50] == o.beta_v && sm[g0 + 550 + 99 * 50 + 49] == o.state + 99 * 64 + 49);
      const uint64_t mats[3] = {o.update, o.m, o.v};
      for (int q = 0; q < 3; ++q)
        for (int c = 0; c < 50; c += 7)
          for (int j = 0; j < 563; ++j) CHECK(sm[g0 + 5550 + (uint32_t)q * 28150 + c * 563 + j] == mats[q] + l_mat(j, c));
      CHECK(sm[g0 + 5550 + 3 * 28150 + 50 * 50 + 49] == o.transpose + 50 * 64 + 49);
      CHECK(sm[g0 + 5550 + 3 * 28150 + 51 * 50] == o.norm);
    }
  }
  printf("ok: out_layer, gate weights, epoch / layer epoch / update_steps and the gates' fields lie where the files have them\n");

  // ---- what an import adds: lin_t beside layer_input, hidden[50]
  {
    const GmxLstmCkptHalf& sh = lay.half[GMX_LCK_SHORT];
    int twins = 0, ones = 0;
    for (uint32_t i = 0; i < sh.n_segs; ++i) {
      const GmxLstmCkptSeg& s = sh.seg[i];
      if (s.twin) {
        ++twins;
        CHECK(s.twin == d.lin_t && s.bank_off == d.layer_input && s.kind == GMX_LCK_ROWS && s.n == 307 && s.rows == 100);
      }
      if (s.one_at != GMX_LCK_NONE) {
        ++ones;
        CHECK(s.bank_off == d.hidden && s.one_at == 50 && s.kind == GMX_LCK_PLAIN);
      }
    }
    CHECK(twins == 1 && ones == 1);
    CHECK(sh.seg[0].kind == GMX_LCK_RANGE && sh.seg[0].floats == 3);
    for (uint32_t i = 0; i < lay.half[GMX_LCK_LONG].n_segs; ++i)
      CHECK(!lay.half[GMX_LCK_LONG].seg[i].twin && lay.half[GMX_LCK_LONG].seg[i].one_at == GMX_LCK_NONE);
  }
  printf("ok: the import's implicit fields hang on layer_input and hidden alone\n");
  return 0;
}
