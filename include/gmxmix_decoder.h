/* gmxmix_decoder.h -- a whole byte per call in the lock-step chain: the arithmetic decoder (coder/decoder.cpp) and
 * ModPPMD's range walk on the device.  An extension of include/gmxmix.h, which it includes; libgmxmix.so exports these
 * functions, they are declared here because gmxmix.h's list of entry points is pinned by the project's ABI tests.
 * DESIGN.md section 4.20.
 *
 * With every bank attached a gmx_chainstep needs, per bit, the bit the host decoded from the last p and ModPPMD's bit
 * prediction, and per byte ppm[s][256].  After gmx_chainstep_attach_decoder the first two are the device's: the
 * stream's compressed input is resident there (gmx_chainstep_decoder_set_input), and gmx_chainstep_byte runs eight
 * steps and answers with the byte.  Per byte the host writes decoder_ppm[s] and take[s], and learns the byte.
 * Per-bit gmx_chainstep_step calls and byte calls may alternate at byte boundaries; a file's last byte is followed by a
 * GMX_STEP_LEARN-only step with bits[s] = byte & 1. */
#ifndef GMXMIX_DECODER_H_
#define GMXMIX_DECODER_H_

#include "gmxmix.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Once, before the object's first step and after gmx_chainstep_attach_match / _attach_ctx.  ppmd_slot: ModPPMD's slot
 * of the mixers' record; every other slot no device model writes is inactive (0, mask clear) in a byte call.
 * GMX_ERR_INVALID: no context bank is attached; a gate-context column of the mixers, an Indirect column or a Match
 * context word is owned by nobody on the device (the context bank's routes, the Match bank's ctx_columns,
 * mixer_ctx_col / ind_ctx_col); ppmd_slot is outside [0, n) or a slot a device model writes.  GMX_ERR_STATE: after
 * the first step, or twice.  Works with or without an LSTM. */
int gmx_chainstep_attach_decoder(gmx_chainstep* cs, int ppmd_slot);
/* [S][256] floats: PPMd's byte distribution of every stream that takes the coming byte (the array of gmx_chainstep_ppm
 * where there is an LSTM, which reads the same values). */
float* gmx_chainstep_decoder_ppm(gmx_chainstep* cs);
/* Stream s's compressed payload becomes resident on the device (copied: `data` may go).  state NULL: the four start
 * bytes are read as in Decoder's constructor.  state {x1, x2, x, pos}: Decoder::ReadCheckpoint plus the read position,
 * as gmx_chainstep_decoder_state returned it.  GMX_ERR_STATE between launch and wait, or inside a byte call's byte. */
int gmx_chainstep_decoder_set_input(gmx_chainstep* cs, int s, const void* data, size_t n, const uint32_t* state);
/* {x1, x2, x, pos} of stream s after the last answered byte. */
int gmx_chainstep_decoder_state(gmx_chainstep* cs, int s, uint32_t out[4]);
/* [S] flags, 0 / 1: the stream decodes the coming byte. */
uint8_t* gmx_chainstep_take(gmx_chainstep* cs);
/* Eight steps in one call for every stream with take[s] = 1: Learn of the outstanding bit (if any), then Predict,
 * decode, Learn + Predict seven times, and the decode of the eighth bit, whose Learn is left outstanding.  A taking
 * stream must stand at a byte boundary and have an input; the bit of its outstanding Learn is the last decoded byte's
 * low bit, or bits[s] when its last Predict went through gmx_chainstep_step.  A stream with a Learn outstanding may
 * not sit the byte out.  Otherwise GMX_ERR_STATE / GMX_ERR_INVALID, before anything is queued or counted.
 * _launch returns when the byte is queued, _wait (or gmx_chainstep_wait) when decoded / byte_p hold the answers. */
int gmx_chainstep_byte(gmx_chainstep* cs);
int gmx_chainstep_byte_launch(gmx_chainstep* cs);
int gmx_chainstep_byte_wait(gmx_chainstep* cs);
/* gmx_chainstep_byte with HIP events around the byte's graph: device milliseconds (0 when nothing was queued). */
int gmx_chainstep_timed_byte(gmx_chainstep* cs, float* device_ms);
/* [S] the decoded bytes, [S][8] the probabilities their bits were decoded from (what gmx_chainstep_p held per bit). */
const uint8_t* gmx_chainstep_decoded(gmx_chainstep* cs);
const float* gmx_chainstep_byte_p(gmx_chainstep* cs);
/* Per-bit graphs launched by this object so far (tests: it stands still across byte calls). */
int64_t gmx_debug_chainstep_bit_launches(const gmx_chainstep* cs);

#ifdef __cplusplus
}
#endif
#endif /* GMXMIX_DECODER_H_ */
