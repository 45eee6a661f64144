/* gmxmix_encoder.h -- the arithmetic encoder (coder/encoder.cpp) on the device: compressed bytes out of a batch.  An
 * extension of include/gmxmix.h, which it includes; libgmxmix.so exports these functions, they are declared here because
 * gmxmix.h's list of entry points is pinned by the project's ABI tests.  DESIGN.md section 4.22.
 *
 * A gmx_encoder holds Encoder's state {x1, x2} for n_streams streams.  It codes the bits of a gmx_batch from the batch's
 * DEVICE `bits` and `p`, as the last run left them, or arrays the caller hands in, and returns each stream's bytes, bit
 * for bit what Encoder::Encode / Flush write.  A round is what lies between two takes: within it a stream may be given
 * at most max_bits bits, and a call that would exceed that is refused before anything is queued.
 *
 * Domain of p: 0 <= p <= 1.  At the first bit t of a stream whose p is outside (NaN included) the stream stops: state
 * and output stay as after bit t - 1, the rest of its bits in this call and later ones are skipped until a reset,
 * gmx_encoder_bad_bit(s) is t counted since the reset, and every take until then returns GMX_ERR_INVALID while the
 * other streams' bytes are valid and delivered.
 *
 * NULL handles: GMX_ERR_INVALID, NULL or 0. */
#ifndef GMXMIX_ENCODER_H_
#define GMXMIX_ENCODER_H_

#include "gmxmix.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gmx_encoder gmx_encoder;

/* max_bits: 1 .. 2^28. */
int gmx_encoder_create(gmx_encoder** out, int n_streams, uint64_t max_bits, int device);
void gmx_encoder_destroy(gmx_encoder* e);
/* s = -1: every stream.  state NULL: the constructor's {0, 0xffffffff}; otherwise ReadCheckpoint's two words.  Clears
 * the stream's totals and its bad-p mark and discards its bytes not yet taken. */
int gmx_encoder_reset(gmx_encoder* e, int s, const uint32_t* state);
/* {x1, x2} as WriteCheckpoint stores them.  Synchronous: waits for the queued work. */
int gmx_encoder_state(gmx_encoder* e, int s, uint32_t out[2]);
/* Codes bits [0, n_bits[s]) of every stream (0: the stream sits the call out).  Asynchronous, on the batch's group's
 * stream behind the runs queued so far; it counts as a use of the batch as a run does: an upload, synthetic fill or run
 * of the batch queued afterwards does not overtake it.  kernel_ms non-NULL makes the call synchronous, as in
 * gmx_group_run.  GMX_ERR_INVALID, before anything is queued: another stream count, another device, a count beyond
 * either object's max_bits or the round's, a batch whose group is gone. */
int gmx_encoder_encode_batch(gmx_encoder* e, gmx_batch* b, const uint64_t* n_bits, float* kernel_ms);
/* The same for host arrays p [S][pitch], bits [S][pitch]; they are copied before the call returns. */
int gmx_encoder_encode(gmx_encoder* e, const float* p, const uint8_t* bits, uint64_t pitch, const uint64_t* n_bits);
/* Encoder::Flush for the streams with which[s] != 0 (NULL: all).  The state is what the loop left, as in the reference:
 * a new file starts with a reset.  The area of a round holds one flush behind max_bits bits. */
int gmx_encoder_flush(gmx_encoder* e, const uint8_t* which);
/* Brings home everything coded since the last take; take = take_launch, then take_wait.  What crosses the link is a
 * 32-byte line per stream and the bytes produced, in whole dwords. */
int gmx_encoder_take(gmx_encoder* e);
int gmx_encoder_take_launch(gmx_encoder* e);
int gmx_encoder_take_wait(gmx_encoder* e);
/* The bytes of the last take: valid until the next encode, flush, take or reset (NULL / 0 after one). */
const uint8_t* gmx_encoder_bytes(gmx_encoder* e, int s);
uint64_t gmx_encoder_n_bytes(gmx_encoder* e, int s);
/* tellp() since the reset, bytes not yet taken included, as of the last take or state call. */
uint64_t gmx_encoder_total_bytes(gmx_encoder* e, int s);
/* -1: healthy, as of the last take or state call. */
int64_t gmx_encoder_bad_bit(gmx_encoder* e, int s);
/* Bytes the last take's kernels wrote into pinned host memory, header lines included. */
int64_t gmx_debug_encoder_d2h_bytes(gmx_encoder* e);

#ifdef __cplusplus
}
#endif
#endif /* GMXMIX_ENCODER_H_ */
