/* gmxmix_analysis.h -- the analysis averages (predictor.cpp: RunAnalysis, UpdateEntropy) on the device: per-model entropy
 * averages out of a batch.  An extension of include/gmxmix.h, which it includes; libgmxmix.so exports these functions,
 * they are declared here because gmxmix.h's list of entry points is pinned by the project's ABI tests.  DESIGN.md
 * section 4.23.
 *
 * A gmx_analysis holds ShortTermMemory::entropy[] -- double exponential averages of the log2 loss -- for n_streams
 * streams x n_columns columns, and ShortTermMemory::bits_seen and the sample frequency of every stream.  It updates them
 * from a mixer gmx_batch's DEVICE arrays as the last run left them (predictions, active mask, outputs, p, bits), or from
 * arrays the caller hands in, bit for bit as the reference does, and captures the rows of analysis/entropy.tsv on the
 * way: per stream and bit, every column is updated; then, with F > 0, bits_seen > 0 and bits_seen % F == 0, the C
 * averages are captured under the label bits_seen; then ++bits_seen.  bits_seen is the count of bits before this one
 * (BasicContexts::Predict skips the increment on the first prediction).  A take brings home the averages and the rows
 * captured since the last take; no per-bit array crosses the link.
 *
 * A NaN value gives a NaN average from there on.
 *
 * NULL handles: GMX_ERR_INVALID, NULL or 0. */
#ifndef GMXMIX_ANALYSIS_H_
#define GMXMIX_ANALYSIS_H_

#include "gmxmix.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gmx_analysis gmx_analysis;

/* What a column averages, per bit:
 *   GMX_AN_INPUT    slot `index` of the batch's prediction record, taken as 0 when the slot's mask bit is off (with
 *                   analysis on Predictor::Predict zeroes the blackboard first, and a silent model leaves that zero); a
 *                   batch without GMX_BATCH_MASK has every slot active
 *   GMX_AN_MIXER    output `index` of the batch's outputs (the batch needs GMX_BATCH_OUTPUTS)
 *   GMX_AN_FINAL_P  the batch's clamped p: the final mixer without its output (index is ignored) */
enum { GMX_AN_INPUT = 0, GMX_AN_MIXER = 1, GMX_AN_FINAL_P = 2 };
typedef struct gmx_analysis_column {
  uint32_t kind;
  uint32_t index;
} gmx_analysis_column;

/* n_columns: 1 .. 512.  max_samples: rows a stream can capture between two takes, 0 .. 2^20.  Averages and bits_seen
 * start at 0, the frequencies at 0 (no rows). */
int gmx_analysis_create(gmx_analysis** out, int n_streams, const gmx_analysis_column* cols, int n_columns,
                        uint64_t max_samples, int device);
void gmx_analysis_destroy(gmx_analysis* a);
/* s = -1: every stream.  ema: n_columns averages (ShortTermMemory::ReadFromDisk's; a new Predictor's are all -1,
 * predictor.cpp:39), NULL: zeros.  Discards the stream's rows not yet taken; its frequency stays. */
int gmx_analysis_reset(gmx_analysis* a, int s, const double* ema, uint64_t bits_seen);
/* Predictor::EnableAnalysis's sample_frequency for stream s (-1: every stream); 0: no rows. */
int gmx_analysis_set_frequency(gmx_analysis* a, int s, uint64_t frequency);
/* Updates every stream with bits [0, n_bits[s]) of the batch (0: the stream sits the call out).  Asynchronous, on the
 * batch's group's stream behind the runs queued so far; it counts as a use of the batch as a run does: an upload,
 * synthetic fill or run of the batch queued afterwards does not overtake it.  kernel_ms non-NULL makes the call
 * synchronous, as in gmx_group_run.  GMX_ERR_INVALID, before anything is queued or changed: another stream count or
 * device, a count beyond the batch's max_bits, an INPUT index >= the group's input count, a MIXER index >= its mixer
 * count or a MIXER column on a batch without GMX_BATCH_OUTPUTS, a batch whose group is gone, a call that would capture
 * more than max_samples rows for a stream since the last take. */
int gmx_analysis_update_batch(gmx_analysis* a, gmx_batch* b, const uint64_t* n_bits, float* kernel_ms);
/* The same for host arrays: values [S][pitch][n_columns], a logit per column (a probability for a GMX_AN_FINAL_P
 * column), bits [S][pitch]; they are copied before the call returns. */
int gmx_analysis_update(gmx_analysis* a, const float* values, const uint8_t* bits, uint64_t pitch,
                        const uint64_t* n_bits);
/* Brings home the averages and the rows captured since the last take; take = take_launch, then take_wait.  What
 * crosses the link is a 16-byte line per stream, 8 * n_columns bytes of averages and 8 * (n_columns + 1) bytes per
 * captured row. */
int gmx_analysis_take(gmx_analysis* a);
int gmx_analysis_take_launch(gmx_analysis* a);
int gmx_analysis_take_wait(gmx_analysis* a);
/* The last take: valid until the next take (NULL / 0 before the first).  ema: n_columns averages; samples: [n][n_columns]
 * rows in capture order; sample_bits: their labels. */
const double* gmx_analysis_ema(gmx_analysis* a, int s);
uint64_t gmx_analysis_bits_seen(gmx_analysis* a, int s);
uint64_t gmx_analysis_n_samples(gmx_analysis* a, int s);
const double* gmx_analysis_samples(gmx_analysis* a, int s);
const uint64_t* gmx_analysis_sample_bits(gmx_analysis* a, int s);
/* Bytes the last take's kernel wrote into pinned host memory, header lines included. */
int64_t gmx_debug_analysis_d2h_bytes(gmx_analysis* a);

#ifdef __cplusplus
}
#endif
#endif /* GMXMIX_ANALYSIS_H_ */
