// gmx_ind_ckpt.h -- arguments of the Indirect group checkpoint kernels (gmx_ind_ckpt.hip), shared with their host
// side (gmx_ind_ckpt.inc).
#ifndef GMX_IND_CKPT_H_
#define GMX_IND_CKPT_H_

#include "gmx_internal.h"

// A model's u16 table is walked in chunks of GMX_IND_CKPT_CHUNK entries, one block per (chunk, stream); the chunks of
// all models of a bank description form one list, the same for every stream.  16 Ki entries = 32 KiB of table per
// block: the 41 stock models give 24 161 chunks, so a stream's counts are 94 KiB on their way to the host.
#define GMX_IND_CKPT_CHUNK 16384
// entries a block takes per iteration: 256 lanes x one 16-byte load of 8 entries
#define GMX_IND_CKPT_STEP 2048
struct GmxIndCkptChunk {
  uint32_t model;
  uint32_t first_entry;
};

struct GmxIndCkptArgs {
  uint8_t* banks;                  // bank of the launch's stream 0
  const GmxIndDev* dev;            // device copy
  const GmxIndCkptChunk* chunks;   // [n_chunks]
  uint32_t n_chunks;
  int32_t n_streams;               // streams of the launch
  // count writes, pack reads: live entries (low byte != 255) per (stream, chunk)
  uint32_t* chunk_cnt;             // [n_streams][n_chunks]
  // pack: live entries of the chunk's model in front of the chunk = index of the chunk's first record
  const uint32_t* chunk_base;      // [n_streams][n_chunks]
  // pack, scatter: the `cnt` of every model's header; cnt < size / 3 = sparse, as on disk
  const uint32_t* model_cnt;       // [n_streams][k]
  // pack, scatter: byte offset of a model's header in `buf` (any alignment)
  const uint64_t* model_off;       // [n_streams][k]
  uint8_t* buf;                    // the packed sections of the launch's streams
};

#endif  // GMX_IND_CKPT_H_
