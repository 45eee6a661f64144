// gmx_ppmd_dev.h -- what gmx_ppmd.hip and its host side (gmx_ppmd.inc) share: the launch arguments of the PPMd bank's
// kernels and their launchers.  The model itself is gmx_ppmd.h.
#ifndef GMX_PPMD_DEV_H_
#define GMX_PPMD_DEV_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmx_ppmd.h"

// Bytes of slack behind every stream's arena: the model's glue step looks at the unit behind a free block, which for
// the reference is whatever lies behind its heap.  (No free block ends at the arena's end -- the root context, never
// freed, is the last unit -- so nothing reads the slack; it is there so that a broken model cannot reach another
// stream's arena or leave the allocation by one unit.)
#define GMX_PPMD_ARENA_SLACK 256u

// n bytes of stream stream_base + blockIdx.x.  A record (gmx_ppmd_record): the update the model owes, PrepareByte, the
// normalised distribution, the walk down it along the record's byte.  With `explicit_last` the bytes are the bytes
// coded last (gmx_ppmd_byte, the per-byte surface): UpdateByte(byte), PrepareByte, the distribution.
struct GmxPpmdRunArgs {
  GmxPpmdState* states;    // [S]
  uint8_t* arena;          // [S][arena_stride]
  uint64_t arena_stride;
  const uint8_t* bytes;    // [S][byte_pitch]
  uint64_t byte_pitch;
  const uint64_t* n_list;  // [S] bytes of each stream (0 sits the launch out); null: n for all
  uint64_t n;
  float* ppm_out;          // [S][rec_pitch][256]
  float* pred_out;         // [S][rec_pitch][8] or null: the byte's own eight bit predictions ...
  uint8_t* act_out;        // [S][rec_pitch][8]   ... and their active flags
  uint64_t* used_out;      // [S][rec_pitch] or null: 16 + used memory behind every byte
  uint64_t rec_pitch;
  int32_t stream_base;
  int32_t explicit_last;
};

struct GmxPpmdFeedArgs {
  const float* ppm;        // the bank's batch
  const float* pred;
  const uint8_t* act;
  uint64_t rec_pitch, n_bytes;
  float* lstm_ppm;         // [S][lstm_pitch][256] or null
  uint64_t lstm_pitch;
  float* mx_pred;          // [S][mx_pitch][mx_n_pad] or null
  uint32_t* mx_mask;       // [S][mx_pitch][mx_mask_words]
  uint64_t mx_pitch;
  int32_t mx_n_pad, mx_mask_words, slot;
};

extern "C" {
hipError_t gmx_launch_ppmd_init(GmxPpmdState* states, uint8_t* arena, uint64_t arena_stride, uint64_t arena_bytes,
                                int order, int stream_base, int n_streams, hipStream_t stream);
hipError_t gmx_launch_ppmd_run(const GmxPpmdRunArgs* args, int n_streams, hipStream_t stream);
hipError_t gmx_launch_ppmd_feed(const GmxPpmdFeedArgs* args, int n_streams, hipStream_t stream);
}

#endif  // GMX_PPMD_DEV_H_
