/* gmxmix_ppmd.h -- the PPMd byte model on the device (extension of gmxmix.h).
 *
 * A gmx_ppmd bank holds the reference's PPMD::ModPPMD (models/mod_ppmd.cpp: PPMd with SEE, inheritance, rescale and
 * the cutOff model flush) for S independent streams, each with an arena of arena_mb MiB, bit-exact with the reference
 * for as long as a stream's arena has not run full; from a stream's first model flush on, its answers are those of a
 * reference model with the same arena size (ModPPMD's `memory` argument).  gmx_ppmd_restores counts the flushes.
 *
 * Two surfaces, one model per stream:
 *
 *   records (gmx_ppmd_run, for compressing): bytes[s][n] is the byte being CODED, as in the LSTM bank's records.
 *   Record n runs ppmd_UpdateByte of the byte before it -- which the stream still owes: 0 for a new model, as a new
 *   Predictor's first Predict hands in -- and ppmd_PrepareByte, and gives
 *     ppm[256]        ModPPMD::Predict's normalised byte distribution (ShortTermMemory::ppm_predictions)
 *     predictions[8]  the model's slot at each of the eight bits of bytes[s][n] (SetPrediction's logit)
 *     active[8]       whether the slot counts as active (p != 0.5)
 *     used            ModPPMD::GetMemoryUsage (16 + the allocator's used bytes) behind the record
 *   The record's own byte is the update the stream owes next.
 *
 *   steps (gmx_ppmd_step, for decoding in lock step): the caller hands in the byte coded LAST, as the reference's
 *   last_byte (0 before the first byte); the step runs ppmd_UpdateByte(last_byte) and ppmd_PrepareByte and gives
 *   ppm[256].  The stream then owes nothing: a record right behind a step prepares the same distribution again,
 *   without an update, and takes its byte as the one owed next.  A step behind records is handed the last record's
 *   byte like any other.
 *
 * Every call returns 0 or a gmx_status.  GMX_ERR_INVALID comes before anything is queued or changed.  Run and feed are
 * asynchronous on the bank's stream; a batch's download and wait follow the rules of the other banks' batches.
 */
#ifndef GMXMIX_PPMD_H_
#define GMXMIX_PPMD_H_

#include "gmxmix.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gmx_ppmd gmx_ppmd;
typedef struct gmx_ppmd_batch gmx_ppmd_batch;

/* what gmx_ppmd_batch_download fetches */
enum { GMX_PPMD_PPM = 1, GMX_PPMD_PREDICTIONS = 2, GMX_PPMD_USED = 4, GMX_PPMD_ALL = 7 };

/* order 2 .. 64 (below 2 is the reference's solid mode: refused), arena_mb 1 .. 4095.  GMX_ERR_NOMEM when
 * n_streams x arena_mb does not fit on the device, GMX_ERR_NO_DEVICE without one. */
int gmx_ppmd_create(gmx_ppmd** out, int n_streams, int order, int arena_mb, int device);
void gmx_ppmd_destroy(gmx_ppmd* p);
int gmx_ppmd_n_streams(const gmx_ppmd* p);
uint64_t gmx_ppmd_bank_bytes(const gmx_ppmd* p);   /* device bytes per stream */
int gmx_ppmd_reset(gmx_ppmd* p, int stream);       /* a new model; -1: every stream */
int gmx_ppmd_sync(gmx_ppmd* p);

/* records of up to max_bytes bytes per stream: bytes [S][max_bytes] in; ppm [S][max_bytes][256],
 * predictions [S][max_bytes][8], active [S][max_bytes][8] and used [S][max_bytes] out (pinned host arrays) */
int gmx_ppmd_batch_create(gmx_ppmd_batch** out, gmx_ppmd* p, uint64_t max_bytes);
void gmx_ppmd_batch_destroy(gmx_ppmd_batch* b);
uint64_t gmx_ppmd_batch_max_bytes(const gmx_ppmd_batch* b);
uint8_t* gmx_ppmd_batch_bytes(gmx_ppmd_batch* b);
const float* gmx_ppmd_batch_ppm(gmx_ppmd_batch* b);
const float* gmx_ppmd_batch_predictions(gmx_ppmd_batch* b);
const uint8_t* gmx_ppmd_batch_active(gmx_ppmd_batch* b);
const uint64_t* gmx_ppmd_batch_used(gmx_ppmd_batch* b);
int gmx_ppmd_batch_upload(gmx_ppmd_batch* b, uint64_t n_bytes);
int gmx_ppmd_batch_download(gmx_ppmd_batch* b, uint64_t n_bytes, unsigned what);
int gmx_ppmd_batch_wait(gmx_ppmd_batch* b);

/* the first n_bytes records of every stream / n_bytes[s] of stream s (0: the stream sits the call out) */
int gmx_ppmd_run(gmx_ppmd* p, gmx_ppmd_batch* b, uint64_t n_bytes, float* kernel_ms);
int gmx_ppmd_run_ragged(gmx_ppmd* p, gmx_ppmd_batch* b, const uint64_t* n_bytes);

/* device to device, behind a run: ppm of the first n_bytes records into the LSTM batch's ppm column, the eight
 * predictions of byte n into slot `slot` of records 8n .. 8n+7 of the mixer batch and the active flags into its mask.
 * Either target may be NULL, not both.  Counts as a use of the target batches. */
int gmx_ppmd_feed(gmx_ppmd* p, gmx_ppmd_batch* b, uint64_t n_bytes, gmx_lstm_batch* lstm_batch, gmx_batch* mixer_batch,
                  int slot);

/* the per-byte surface: UpdateByte(last_byte[s]) and PrepareByte for every stream with take[s] != 0; its ppm[256]
 * lands in row s of the bank's pinned array (a stream that sits the step out keeps its row).  One step in flight at
 * a time (GMX_ERR_STATE otherwise). */
int gmx_ppmd_step_launch(gmx_ppmd* p, const uint8_t* last_byte, const uint8_t* take);
int gmx_ppmd_step_wait(gmx_ppmd* p);
int gmx_ppmd_step(gmx_ppmd* p, const uint8_t* last_byte, const uint8_t* take);
const float* gmx_ppmd_step_ppm(gmx_ppmd* p);       /* [S][256] */

/* ModPPMD::GetMemoryUsage of a stream, and its model flushes (RestoreModelRare calls) since create / reset; both wait
 * for the bank's queued work.  0 / -1 for a bad handle or stream. */
uint64_t gmx_ppmd_memory_usage(gmx_ppmd* p, int stream);
int64_t gmx_ppmd_restores(gmx_ppmd* p, int stream);

/* model kernels launched so far (run, run_ragged, step); GMX_ERR_INVALID for NULL */
int64_t gmx_debug_ppmd_launches(gmx_ppmd* p);

#ifdef __cplusplus
}
#endif

#endif /* GMXMIX_PPMD_H_ */
