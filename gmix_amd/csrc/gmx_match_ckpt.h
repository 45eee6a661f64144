// gmx_match_ckpt.h -- arguments of the Match group checkpoint kernels (gmx_match_ckpt.hip), shared with their host
// side (gmx_match_ckpt.inc).  The chunk list and GMX_MATCH_CKPT_CHUNK are the bank's own (gmx_match.h).
#ifndef GMX_MATCH_CKPT_H_
#define GMX_MATCH_CKPT_H_

#include "gmx_match.h"

// What a bank keeps behind its tables, probabilities and counts, as it lies there: 144 contiguous bytes.
struct GmxMatchGckStates {
  GmxMatchModelState m[GMX_MATCH_MAX_MODELS];
  GmxMatchStreamState s;
};

// One stream of the call.
struct GmxMatchGckStream {
  uint64_t sec_off;    // byte offset of the stream's long section in the image
  uint32_t hist_size;  // its u64 header (history_capacity is below 2^32)
  uint32_t pad;
};

// One (stream, model) of the call.
struct GmxMatchGckModel {
  uint64_t off;        // byte offset in the image of the model's u32 count; the body follows, then the 2 KiB tail
  uint32_t cnt;        // valid entries
  uint32_t cur_match;  // import: the model's short section ...
  uint8_t dense;       // the branch, decided on the host in double as the reference does
  uint8_t cur_byte, bit_pos, match_length;  // ... import
};

struct GmxMatchGckArgs {
  uint8_t* banks;                    // bank of the call's first stream
  uint8_t* hist;                     // history of the call's first stream
  const GmxMatchDev* dev;
  const GmxMatchCkptChunk* chunks;   // [n_chunks]
  uint32_t n_chunks;
  uint32_t n_streams;                // streams of the call
  uint32_t blocks;                   // history, zero: blocks per stream; scatter: blocks per (stream, model)
  uint32_t* chunk_cnt;               // [n_streams][n_chunks] count writes, pack reads: valid entries per chunk
  const uint32_t* chunk_base;        // [n_streams][n_chunks] pack: valid entries of the chunk's model in front of it
  GmxMatchGckStates* states;         // [n_streams] count writes: the banks' states, for the host
  const GmxMatchGckStream* st;       // [n_streams]
  const GmxMatchGckModel* md;        // [n_streams][k]
  uint8_t* image;                    // every stream's long section, laid out as the caller's buffer
};

#endif  // GMX_MATCH_CKPT_H_
