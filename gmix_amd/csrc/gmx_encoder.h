// gmx_encoder.h -- the reference's arithmetic encoder (coder/encoder.cpp: Encode, Flush) as pure functions for host and
// device alike (GMX_HD, as gmx_coder.h, whose Discretize it shares).  No HIP in here: tests/cpp/test_encoder.cpp builds
// it for the host, gmx_encoder.hip runs it a lane per stream, scripts/encoder_host_leg.c times it on host threads.
//
// All arithmetic is modulo 2^32 as in the reference, and any two state words are accepted.  Nothing here may be
// contracted (gmx_coder_discretize: one rounded multiply, one rounded add).
#ifndef GMX_ENCODER_H_
#define GMX_ENCODER_H_

#include "gmx_coder.h"

// Encoder's x1_, x2_: what WriteCheckpoint stores.
struct GmxEncoderState {
  uint32_t x1, x2;
};

// The domain of p: 0 <= p <= 1 (-0.0 is 0).  NaN and everything else is a bad p, which the callers do not code.
GMX_HD bool gmx_encoder_p_ok(float p) { return p >= 0.0f && p <= 1.0f; }

// The renormalisation loop of Encode and Flush, closed: it shifts a byte out while the top bytes of x1 and x2 agree,
// at most four times (after four shifts x1 is 0 and x2 is 0xffffffff, which differ).  Returns the count k = 0..4 and
// leaves the k bytes in *word in the order they were written, the first in the low byte.
GMX_HD uint32_t gmx_encoder_shift(GmxEncoderState* st, uint32_t* word) {
  const uint32_t x1 = st->x1, x2 = st->x2, d = x1 ^ x2;
  const uint32_t k = (d & 0xff000000u) ? 0u : (d & 0x00ff0000u) ? 1u : (d & 0x0000ff00u) ? 2u : (d & 0x000000ffu) ? 3u : 4u;
  const uint32_t sh = 8u * k;
  const uint32_t rev = (x2 >> 24) | ((x2 >> 8) & 0xff00u) | ((x2 << 8) & 0xff0000u) | (x2 << 24);
  const uint32_t ones = (uint32_t)((1ull << sh) - 1ull);
  *word = rev & ones;
  st->x1 = (uint32_t)((uint64_t)x1 << sh);
  st->x2 = (uint32_t)((uint64_t)x2 << sh) | ones;
  return k;
}

// Encoder::Encode behind Discretize: pr is the 16-bit probability (1..65535 for a p of the domain).
GMX_HD uint32_t gmx_encoder_bit_pr(GmxEncoderState* st, uint32_t bit, uint32_t pr, uint32_t* word) {
  const uint32_t range = st->x2 - st->x1;
  const uint32_t xmid = st->x1 + (range >> 16) * pr + (((range & 0xffffu) * pr) >> 16);
  if (bit)
    st->x2 = xmid;
  else
    st->x1 = xmid + 1u;
  return gmx_encoder_shift(st, word);
}

// Encoder::Encode(bit, p): writes 0..4 bytes to `out` and returns how many.
GMX_HD uint32_t gmx_encoder_bit(GmxEncoderState* st, uint32_t bit, float p, uint8_t* out) {
  uint32_t word;
  const uint32_t k = gmx_encoder_bit_pr(st, bit, gmx_coder_discretize(p), &word);
  for (uint32_t i = 0; i < k; ++i) out[i] = (uint8_t)(word >> (8u * i));
  return k;
}

// Encoder::Flush: the same loop, then x2 >> 24.  Writes 1..5 bytes and returns how many; the state is what the loop left.
GMX_HD uint32_t gmx_encoder_flush(GmxEncoderState* st, uint8_t* out) {
  uint32_t word;
  const uint32_t k = gmx_encoder_shift(st, &word);
  for (uint32_t i = 0; i < k; ++i) out[i] = (uint8_t)(word >> (8u * i));
  out[k] = (uint8_t)(st->x2 >> 24);
  return k + 1u;
}

#endif  // GMX_ENCODER_H_
