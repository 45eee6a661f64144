// gmx_ctx_ckpt.h -- arguments of the context group checkpoint kernels (gmx_ctx_ckpt.hip), shared with their host side
// (gmx_ctx_ckpt.inc).  The chunk list and GMX_CTX_CKPT_CHUNK are the bank's own (gmx_ctx.h).
#ifndef GMX_CTX_CKPT_H_
#define GMX_CTX_CKPT_H_

#include "gmx_ctx.h"

// One (stream, table) of the call.
struct GmxCtxGckTable {
  uint64_t off;    // byte offset in the image of the table's u32 count (a multiple of 4); body and trailer follow
  uint32_t cnt;    // non-zero entries
  uint32_t dense;  // the branch, decided on the host (ctx_is_dense)
};

// gmx_ctx_blackboard (include/gmxmix.h) as the board kernels see it: the records of one contiguous device array.
struct GmxCtxGckBoard {
  int32_t recent_bits;
  int32_t new_bit;
  uint32_t last_byte;
  uint32_t rotating_history_pos;
  int32_t first_prediction;
  uint32_t recent_bytes[10];
  uint32_t values[GMX_CTX_MAX_VARS];
  uint8_t rotating_history[GMX_CTX_RING];
};

struct GmxCtxGckArgs {
  uint8_t* banks;                   // bank of the launch's first stream
  const GmxCtxDev* dev;
  const GmxCtxCkptChunk* chunks;    // [n_chunks]
  uint32_t n_chunks;
  uint32_t n_streams;               // streams of the launch
  uint32_t blocks;                  // zero, scatter: blocks per (stream, table)
  uint32_t pad;
  uint32_t* chunk_cnt;              // [n_streams][n_chunks] count writes, pack reads: non-zero entries per chunk
  const uint32_t* chunk_base;       // [n_streams][n_chunks] pack: non-zero entries of the chunk's table in front of it
  GmxCtxHashState* states;          // [n_streams][GMX_CTX_MAX_HASH] count writes: the banks' hash states, for the host
  const GmxCtxGckTable* tb;         // [n_streams][h]
  uint8_t* image;                   // the launch's sections, laid out as the caller's buffer
  GmxCtxGckBoard* boards;           // [n_streams] board gather writes, board scatter reads
};

#endif  // GMX_CTX_CKPT_H_
