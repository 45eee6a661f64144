// chainstep_byte_host.cpp -- the host's turn of a per-bit lock step, in C, for scripts/bench_chainstep_byte.py (leg A):
// for every stream Decoder::Decode of the bit from the last p, ModPPMD's range walk, its slot and mask bit of the
// stream's record, and the step's bits / what.  gmx_coder.h built for the host; the script compiles this file into
// build_tmp/ with g++ -O2 -ffp-contract=off and calls it through ctypes.
#include <cstdint>

#include "gmx_coder.h"

extern "C" void gmxb_init(int S, GmxCoderState* st, const uint8_t* buf, uint32_t len) {
  for (int s = 0; s < S; ++s) gmx_coder_init(&st[s], buf + (uint64_t)s * len, len);
}

// j: the bit's place in its byte, 0..7.  decode: the streams have a Predict outstanding (every step but the very first).
extern "C" void gmxb_host_bit(int S, int j, int decode, GmxCoderState* st, GmxCoderWalk* walk, const uint8_t* buf,
                              uint32_t len, const float* p, const float* ppm, float* pred, int n_pad, uint32_t* mask,
                              int mask_words, int slot, uint8_t* bits, uint8_t* what) {
  for (int s = 0; s < S; ++s) {
    uint32_t bit = 0;
    if (decode) bit = gmx_coder_decode(&st[s], p[s], buf + (uint64_t)s * len, len);
    bits[s] = (uint8_t)bit;
    what[s] = (uint8_t)(decode ? 3 : 2);
    if (j == 0)
      gmx_coder_walk_open(&walk[s]);
    else
      gmx_coder_walk_bit(&walk[s], bit);
    float v = pred[(uint64_t)s * n_pad + slot];
    bool active = false;
    if (gmx_coder_walk_predict(&walk[s], ppm + (uint64_t)s * 256, &v, &active)) pred[(uint64_t)s * n_pad + slot] = v;
    uint32_t* w = mask + (uint64_t)s * mask_words + (slot >> 5);
    const uint32_t m = 1u << (slot & 31);
    *w = active ? (*w | m) : (*w & ~m);
  }
}
