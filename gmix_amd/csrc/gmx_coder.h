// gmx_coder.h -- the two pieces of the reference that kept the host in the lock step's loop for every bit, as pure
// functions for host and device alike (GMX_HD, as gmx_math.h): the arithmetic decoder's bit (coder/decoder.cpp:17-39,
// without the Predictor calls) and ModPPMD's walk down the byte distribution (mod_ppmd.cpp:1662-1681).  No HIP in here:
// tests/cpp/test_coder.cpp builds it for the host; gmx_coder.hip hosts it in the lock step's byte graphs.
//
// Nothing here may be contracted: Discretize is one rounded multiply and one rounded add (the device spells them out,
// the host is built with -ffp-contract=off), the sums are std::accumulate's, strictly left to right.
#ifndef GMX_CODER_H_
#define GMX_CODER_H_

#include "gmx_math.h"

// Decoder's x1_, x2_, x_ (what WriteCheckpoint stores) and the read position in the stream's compressed input: bytes
// consumed so far, never beyond the input's length (every read past the end is 0, as ReadByte after !good()).
struct GmxCoderState {
  uint32_t x1, x2, x, pos;
};

// Decoder::Discretize: `1 + 65534 * p` in float, truncated to unsigned.
GMX_HD uint32_t gmx_coder_discretize(float p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__fadd_rn(1.0f, __fmul_rn(65534.0f, p));
#else
  const float m = 65534.0f * p;
  return (uint32_t)(1.0f + m);
#endif
}

GMX_HD uint32_t gmx_coder_read_byte(GmxCoderState* st, const uint8_t* input, uint32_t n) {
  if (st->pos >= n) return 0u;
  return (uint32_t)input[st->pos++];
}

// Decoder's constructor without `resume`: the four start bytes.
GMX_HD void gmx_coder_init(GmxCoderState* st, const uint8_t* input, uint32_t n) {
  st->x1 = 0u;
  st->x2 = 0xffffffffu;
  st->x = 0u;
  st->pos = 0u;
  for (int i = 0; i < 4; ++i) st->x = (st->x << 8) + gmx_coder_read_byte(st, input, n);
}

// Decoder::Decode for the probability `p` Predict() returned.  The renormalisation shifts at most four bytes: after
// four x1 is 0 and x2 is 0xffffffff.
GMX_HD uint32_t gmx_coder_decode(GmxCoderState* st, float p, const uint8_t* input, uint32_t n) {
  const uint32_t pr = gmx_coder_discretize(p);
  const uint32_t range = st->x2 - st->x1;
  const uint32_t xmid = st->x1 + (range >> 16) * pr + (((range & 0xffffu) * pr) >> 16);
  uint32_t bit = 0u;
  if (st->x <= xmid) {
    bit = 1u;
    st->x2 = xmid;
  } else {
    st->x1 = xmid + 1u;
  }
  for (int i = 0; i < 4 && ((st->x1 ^ st->x2) & 0xff000000u) == 0u; ++i) {
    st->x1 <<= 8;
    st->x2 = (st->x2 << 8) + 255u;
    st->x = (st->x << 8) + gmx_coder_read_byte(st, input, n);
  }
  return bit;
}

// ModPPMD's range [bot, top] over the 256 byte values: a byte opens with the whole range, a coded bit halves it.
struct GmxCoderWalk {
  int32_t top, bot;
};
GMX_HD void gmx_coder_walk_open(GmxCoderWalk* w) {
  w->top = 255;
  w->bot = 0;
}
GMX_HD void gmx_coder_walk_bit(GmxCoderWalk* w, uint32_t bit) {
  const int32_t mid = w->bot + ((w->top - w->bot) / 2);
  if (bit)
    w->bot = mid + 1;
  else
    w->top = mid;
}
// The bit prediction of the range: num over (mid, top], denom on from num over [bot, mid], both in std::accumulate's
// order.  Returns false when denom == 0 (ModPPMD writes nothing: the slot keeps its value and stays inactive);
// otherwise *slot = SetPrediction's Logit of the clamped quotient and *active = the quotient is not 0.5.
GMX_HD bool gmx_coder_walk_predict(const GmxCoderWalk* w, const float* ppm, float* slot, bool* active) {
  const int32_t mid = w->bot + ((w->top - w->bot) / 2);
  float num = 0.0f;
  for (int32_t i = mid + 1; i <= w->top; ++i) num += ppm[i];
  float denom = num;
  for (int32_t i = w->bot; i <= mid; ++i) denom += ppm[i];
  if (denom == 0.0f) return false;
  const float p = num / denom;
  *slot = gmx_logit(p);
  *active = p != 0.5f;
  return true;
}

#endif  // GMX_CODER_H_
