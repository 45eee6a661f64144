// gmx_ckpt.h -- arguments of the group checkpoint kernels (gmx_ckpt.hip), shared with their host side (gmx_ckpt.inc).
#ifndef GMX_CKPT_H_
#define GMX_CKPT_H_

#include "gmx_internal.h"

// A mixer's table is walked in chunks of GMX_CKPT_CHUNK rows, one block per (chunk, stream); the chunks of all
// mixers of a topology form one list, the same for every stream.
#define GMX_CKPT_CHUNK 256
struct GmxCkptChunk {
  uint32_t mixer;
  uint32_t first_row;
};

struct GmxCkptArgs {
  uint8_t* banks;               // bank of the launch's stream 0
  const GmxTopoDev* topo;       // device copy
  const GmxCkptChunk* chunks;   // [n_chunks]
  uint32_t n_chunks;
  int32_t n_streams;            // streams of the launch
  // count writes, pack reads: rows with steps != 0 per (stream, chunk)
  uint32_t* chunk_cnt;          // [n_streams][n_chunks]
  // pack: byte offset of a chunk's first record in `long_buf`
  const uint64_t* chunk_off;    // [n_streams][n_chunks]
  // pack, scatter: learned rows of every mixer (the `cnt` of its header)
  const uint32_t* mixer_cnt;    // [n_streams][m]
  // scatter: byte offset of a mixer's first record in `long_buf`
  const uint64_t* mixer_off;    // [n_streams][m]
  uint32_t* long_buf;           // the packed long sections of the launch's streams
  uint32_t* short_buf;          // [n_streams][6 * m] dwords: {steps_, max_steps_, contexts_seen_} x m
};

#endif  // GMX_CKPT_H_
