// gmx_ctx.h -- device structs of the context banks (gmx_ctx.hip), shared with their host side (gmx_ctx.inc).
#ifndef GMX_CTX_H_
#define GMX_CTX_H_

#include <stdint.h>

#define GMX_CTX_MAX_VARS 64
#define GMX_CTX_MAX_HASH 16      // lane = (stream, hash variable): 16 lanes per stream, four streams per wave
#define GMX_CTX_MAX_ROUTE 128    // columns of one target's records
#define GMX_CTX_RING 1000        // ShortTermMemory::rotating_history (short-term-memory.h:23)
#define GMX_CTX_TILE 32          // byte slots one block of the expand kernel covers (256 bit records)

// kinds: the values of gmx_ctx_kind (include/gmxmix.h)
#define GMX_CTXK_ZERO 0
#define GMX_CTXK_BIT_CONTEXT 1
#define GMX_CTXK_RECENT_BYTE 2
#define GMX_CTXK_BYTE_PLUS_RECENT 3
#define GMX_CTXK_INTERVAL 4
#define GMX_CTXK_SKIP 5
#define GMX_CTXK_INDIRECT_HASH 6

struct GmxCtxVarDev {
  int32_t kind;
  int32_t index;        // RECENT_BYTE / BYTE_PLUS_RECENT: bytes ago.  INTERVAL: row of GmxCtxDev::maps.  INDIRECT_HASH: h
  int32_t num_bits;     // INTERVAL
  int32_t shift;        // INTERVAL: shift_ (interval-context.cpp:12-13)
  int32_t n_bytes;      // SKIP
  uint8_t bytes_to_use[8];
  uint32_t pad;
};

struct GmxCtxHashDev {
  uint64_t tab_off;     // byte offset of the u32 table in a bank
  uint32_t table_size;
  uint32_t outer_mask;  // outer_mod_ - 1 = (1 << (8 * (order - 1))) - 1, indirect-hash.cpp:10-11: x % mod is x & mask
  uint32_t inner_mask;
  int32_t var;          // the variable it writes
};

// What IndirectHash keeps besides its table (indirect-hash.h:29-33).
struct GmxCtxHashState {
  uint64_t outer_context;
  uint32_t outer_hash;
  uint32_t pad;
};

// The byte-level blackboard of one stream as of its newest Predict, and new_bit, the bit coded since.
struct GmxCtxBoard {
  uint32_t recent_bits;       // ShortTermMemory::recent_bits
  uint32_t new_bit;           // ShortTermMemory::new_bit
  uint32_t first_prediction;  // BasicContexts::first_prediction_
  uint32_t pos;               // rotating_history_pos; last_byte is ring[pos], recent_bytes[i] is ring[pos - i]
  uint32_t values[GMX_CTX_MAX_VARS];
  uint32_t next_values[GMX_CTX_MAX_VARS];  // expand -> commit: the values at the run's last record
  uint8_t ring[GMX_CTX_RING];
};

struct GmxCtxDev {
  int32_t v, h;
  uint64_t bank_bytes;  // per stream: tables, hash states, board
  uint64_t tab_bytes;   // leading part: the tables
  uint64_t hstate_off;  // GmxCtxHashState [16]
  uint64_t board_off;   // GmxCtxBoard
  GmxCtxVarDev var[GMX_CTX_MAX_VARS];
  GmxCtxHashDev hash[GMX_CTX_MAX_HASH];
  uint8_t maps[GMX_CTX_MAX_VARS][256];  // row i: the map of the i-th INTERVAL variable
};

struct GmxCtxTarget {
  uint32_t* ctx;        // [S][stride][n_cols]; null: no such target
  uint32_t* bc;         // [S][stride] nullable
  uint8_t* bits;        // [S][stride] nullable
  uint64_t stride;
  int32_t n_cols;
  int32_t pad;
  int32_t route[GMX_CTX_MAX_ROUTE];
};

struct GmxCtxRunArgs {
  uint8_t* banks;
  const uint8_t* bits;      // [S][rec_stride]
  uint32_t* values;         // [S][rec_stride][v] nullable
  uint32_t* scratch;        // [S][max_fires][h]: the hash variables at every byte opening of the run
  uint64_t rec_stride;
  uint64_t max_fires;
  uint64_t T;               // bits of every stream, or the largest of T_list
  const uint64_t* T_list;   // nullable [n_streams]
  int32_t n_streams;
  int32_t pad;
  GmxCtxTarget tg[3];       // mixers, Indirect, Match
};

// One lock-step bit (gmx_ctx_step.h): the step's device copy of the control words and of the records.
struct GmxCtxStepArgs {
  uint8_t* banks;
  const uint8_t* bits;      // [S] the bit a stream learns
  const uint8_t* what;      // [S] GMX_STEP_*; 0: the stream sits the step out
  uint32_t* bc;             // [S] bit_contexts of the step's records; nullable
  int32_t n_streams;
  int32_t pad;
  GmxCtxTarget tg[3];       // mixers, Indirect, Match: ctx [S][n_cols] (stride, bc, bits unused)
};

// One bit of ONE stream on the launch path (gmx_ctx_forward / gmx_ctx_learn, gmx_ctx_bit_kernel): what the stream asks
// and the bit a Learn takes are kernel arguments; the answer goes into a small pinned block.
struct GmxCtxBitReply {
  uint32_t bit_context;
  uint32_t pad[15];
  uint32_t values[GMX_CTX_MAX_VARS];
};
struct GmxCtxBitArgs {
  uint8_t* banks;
  GmxCtxBitReply* reply;    // pinned host memory
  int32_t stream;
  uint32_t what;            // GMX_CTX_STEP_LEARN | GMX_CTX_STEP_PREDICT
  uint32_t bit;
  uint32_t pad;
};

// The stream's context variables riding in the per-bit session wave of the Indirect models (gmx_indirect_attach_ctx,
// gmx_ctx_step_wave in gmx_ctx_step.h).  What they do in a chained forward is the command's ctx_what word:
// GMX_CTX_STEP_LEARN | GMX_CTX_STEP_PREDICT, and
#define GMX_CTX_WAVE_VALUES 4u     // the V values go into the reply as well
#define GMX_CTX_WAVE_RELOAD 8u     // something else has moved the stream's board since the wave's last step: its register
                                   // copy is read again
#define GMX_CTX_WAVE_BIT_SHIFT 8   // the coded bit of the Learn
struct GmxCtxWaveArgs {
  const GmxCtxDev* dev;     // null: no context bank rides
  uint8_t* bank;            // the STREAM's bank
  const int32_t* routes;    // device memory: [64] Indirect columns | [8] Match columns | [64] mixer columns; -1: not routed
  int32_t n_mixer_cols;
  int32_t pad;
};
#define GMX_CTX_WAVE_ROUTE_IND 0
#define GMX_CTX_WAVE_ROUTE_MATCH 64
#define GMX_CTX_WAVE_ROUTE_MIXER 72
#define GMX_CTX_WAVE_ROUTE_WORDS 136

// ---- checkpoint (indirect-hash.cpp:33-54): tables walked in chunks, one block per chunk
#define GMX_CTX_CKPT_CHUNK 16384
struct GmxCtxCkptChunk {
  uint32_t hash;
  uint32_t first_entry;
};
struct GmxCtxCkptArgs {
  uint8_t* bank;
  const GmxCtxDev* dev;
  const GmxCtxCkptChunk* chunks;
  uint32_t n_chunks;
  uint32_t* chunk_cnt;          // count writes: non-zero entries per chunk
  const uint32_t* chunk_base;   // pack: non-zero entries of the chunk's table in front of the chunk
  const uint8_t* hash_dense;    // pack, scatter: the branch
  const uint32_t* hash_cnt;     // scatter: pairs per table
  const uint64_t* hash_off;     // pack, scatter: u32 offset of a table's pairs in buf
  uint32_t* buf;                // {key, value} pairs
};

#endif  // GMX_CTX_H_
