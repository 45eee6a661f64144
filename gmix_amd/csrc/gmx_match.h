// gmx_match.h -- device structs of the Match-model banks (gmx_match.hip), shared with their host side
// (gmx_match.inc).  Kept out of gmx_internal.h: that header belongs to the mixer kernels' sources.
#ifndef GMX_MATCH_H_
#define GMX_MATCH_H_

#include <stdint.h>

#define GMX_MATCH_MAX_MODELS 8   // one lane group of a wave: lane = (stream, model)
#define GMX_MATCH_MAX_CTX_COLS 8 // mixer context columns that receive longest_match
#define GMX_MATCH_MAX_MASK_WORDS 64

// One Match object (models/match.h:13-45).  Its table holds history pointers as u32 (the reference packs five
// bytes, match.cpp:54-56, :101-107): history_capacity stays below 2^32.
struct GmxMatchModelDev {
  uint64_t tab_off;     // byte offset of the u32 table in a bank
  uint32_t table_size;
  int32_t limit;
  int32_t slot;         // prediction index (ShortTermMemory::AddPrediction, match.cpp:14-15)
  float rate_at_limit;  // learning_rate_ = float(1.0 / limit), match.cpp:13
};

// What a Match object keeps besides its tables (match.h:34-41) and, of ShortTermMemory, what only it writes.
struct GmxMatchModelState {
  uint32_t cur_match;
  uint32_t ctx;         // the aliased context variable as of this byte's first Predict
  float slot_value;     // ShortTermMemory::predictions[slot]
  uint8_t cur_byte, bit_pos, match_length, pad;
};

struct GmxMatchStreamState {
  uint32_t hist_size;   // LongTermMemory::history.size()
  uint32_t new_bit;     // ShortTermMemory::new_bit
  uint32_t bit_context; // of the newest Predict (the per-bit surface learns in a later launch)
  uint32_t pad;
};

struct GmxMatchDev {
  int32_t k;
  int32_t n_slots;      // 1 + the largest slot
  uint64_t bank_bytes;  // per stream: tables, probabilities, counts, model states, stream state
  uint64_t tab_bytes;   // leading part: the tables
  uint64_t pred_off;    // float [k][256]
  uint64_t cnt_off;     // int32 [k][256]
  uint64_t mstate_off;  // GmxMatchModelState [8]
  uint64_t sstate_off;  // GmxMatchStreamState
  uint64_t hist_cap;    // bytes of a stream's history buffer
  GmxMatchModelDev m[GMX_MATCH_MAX_MODELS];
};

#define GMX_MATCH_PREDICT 1u
#define GMX_MATCH_LEARN 2u

struct GmxMatchRunArgs {
  uint8_t* banks;
  uint8_t* hist;              // [S][hist_cap]
  const uint32_t* ctx;        // [S][rec_stride][k]
  const uint32_t* bc;         // [S][rec_stride]
  const uint8_t* bits;        // [S][rec_stride]
  float* pred_out;            // [S][rec_stride][k]
  uint8_t* act_out;           // [S][rec_stride][k]
  uint32_t* longest_out;      // [S][rec_stride]
  uint64_t rec_stride;
  uint64_t T;                 // bits of every stream, or the largest of T_list
  const uint64_t* T_list;     // nullable: [n_streams] bits of each stream of the launch
  uint32_t what;              // GMX_MATCH_PREDICT | GMX_MATCH_LEARN (a batch: both)
  int32_t stream_base;        // first stream (bank) of the launch
  int32_t rec_base;           // its row in the record arrays
  int32_t n_streams;          // streams of the launch
  // the attached mixer batch (nullable)
  float* mx_pred;             // [S][mx_rec_stride][mx_n_pad]
  uint32_t* mx_mask;          // [S][mx_rec_stride][mx_mask_words]
  uint32_t* mx_ctx;           // [S][mx_rec_stride][mx_m]
  uint64_t mx_rec_stride;
  int32_t mx_n_pad, mx_mask_words, mx_m;
  int32_t n_ctx_cols;
  int32_t ctx_cols[GMX_MATCH_MAX_CTX_COLS];
};

// One bit of every stream in lock step, the coded bit of a forward known a launch later (gmx_match_step.h; hosted by
// gmx_match_step_kernel and by gmx_indirect_step_kernel, gmx_chainstep.inc)
struct GmxMatchStepArgs {
  uint8_t* banks;
  uint8_t* hist;              // [S][hist_cap]
  const uint32_t* ctx;        // [S][k]  read when the step's Predict opens a byte, or what[s] & 8
  const uint32_t* bc;         // [S]     bit_context of this step's Predict
  const uint8_t* bits;        // [S]     the coded bit of each stream's previous forward
  const uint8_t* what;        // [S]     bit 0: learn, bit 1: predict, bit 3: read ctx whatever bc; 0: sits out
  float* mx_pred;             // [S][mx_n_pad] the mixers' records of the same step
  uint32_t* mx_mask;          // [S][mx_mask_words]
  uint32_t* mx_ctx;           // [S][mx_m]
  int32_t mx_n_pad, mx_mask_words, mx_m;
  int32_t n_ctx_cols;
  int32_t ctx_cols[GMX_MATCH_MAX_CTX_COLS];
  int32_t n_streams;
};

// ---- checkpoint (long-term-memory.cpp:70-106) -------------------------------------------------------------
// A table is walked in chunks of GMX_MATCH_CKPT_CHUNK entries, one block per chunk: the six stock tables are
// 1 412 chunks.  An entry is valid when it is not 0 (its fifth byte is always 0 here).
#define GMX_MATCH_CKPT_CHUNK 16384
struct GmxMatchCkptChunk {
  uint32_t model;
  uint32_t first_entry;
};
struct GmxMatchCkptArgs {
  uint8_t* bank;                    // the stream's bank
  const GmxMatchDev* dev;
  const GmxMatchCkptChunk* chunks;  // [n_chunks]
  uint32_t n_chunks;
  uint32_t* chunk_cnt;              // count writes: valid entries per chunk
  const uint32_t* chunk_base;       // pack: valid entries of the chunk's model in front of the chunk
  const uint32_t* model_cnt;        // pack, scatter: valid entries per model; < 5/9 of the table = sparse
  const uint8_t* model_dense;       // pack, scatter: the branch, decided on the host in double as the reference does
  const uint64_t* model_off;        // pack, scatter: byte offset of a model's body (behind its count) in buf
  uint8_t* buf;
};

#endif  // GMX_MATCH_H_
