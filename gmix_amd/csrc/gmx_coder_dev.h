// gmx_coder_dev.h -- what the host (gmx_coder.inc) and gmx_coder.hip share: a stream's resident decoder, the per-byte
// block the host fills, and the arguments of the two kernels of a byte graph.
#ifndef GMX_CODER_DEV_H_
#define GMX_CODER_DEV_H_

#include "gmx_coder.h"
#include "gmx_ctx.h"

// What the host says per byte and stream (gmx_chainstep_byte): read by the byte's first step, which keeps a copy.
struct GmxCoderByteIn {
  uint8_t take;       // the stream decodes this byte (else it sits all eight steps out)
  uint8_t w_first;    // what_dev of the byte's first step: PREDICT | 4, LEARN when a Learn is outstanding, 8 on the
                      // stream's first Predict with a Match bank
  uint8_t b_first;    // the bit that Learn takes
  uint8_t pad;
  uint32_t seq0;      // the step number in front of the byte: step j stamps seq0 + j
  float dec[8];       // decay factor of step j's Learn (decay_base of the stream's learn count)
};

// A stream's decoder, resident in device memory between the steps and the bytes.
struct GmxCoderStream {
  GmxCoderState st;        // after the last decoded bit
  const uint8_t* input;    // the stream's compressed payload (device memory), in_len bytes
  uint32_t in_len;
  GmxCoderWalk walk;       // ModPPMD's top_ / bot_
  float slot;              // ModPPMD's slot of the record: a silent bit (denom == 0) keeps the value
  uint32_t acc;            // the byte's bits decoded so far
  GmxCoderByteIn cur;      // the running byte's copy
  float p[8];              // the byte's eight probabilities
};

struct GmxCoderStepArgs {
  GmxCoderStream* streams;        // [S]
  const GmxCoderByteIn* byte_in;  // [S] (j == 1 reads it)
  const float* p_prev;            // [S] what the mixers' kernel of the step before stored
  const float* ppm;               // [S][256] the byte distributions (the LSTM's array)
  // this step's device copy of the control words and of the mixers' records
  uint8_t *bits, *what;
  float* dec;
  uint32_t* seq;
  uint64_t *tl_learn, *tl_pred;
  float* pred;                    // [S][n_pad]
  uint32_t* mask;                 // [S][mask_words]
  int32_t n_pad, mask_words, slot, j;  // j: 1..8 the step of the byte; 9: the tail
  // the tail's answers, in pinned host memory
  uint8_t* out_byte;              // [S]
  float* out_p;                   // [S][8]
  uint32_t* out_state;            // [S][4]
  uint32_t* stamp;                // [S]
  // the context bank's bit of the step (gmx_ctx_step.h)
  GmxCtxStepArgs ctx;
};

#endif  // GMX_CODER_DEV_H_
