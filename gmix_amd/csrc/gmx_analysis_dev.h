// gmx_analysis_dev.h -- what gmx_analysis.hip and gmx_analysis.inc share: the column kinds, the kernels' arguments, the
// capture arithmetic the host mirrors, and the launchers.
#ifndef GMX_ANALYSIS_DEV_H_
#define GMX_ANALYSIS_DEV_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define GMX_AN_COLS 64    // columns of a block: a lane per column walks
#define GMX_AN_TILE 64    // bits of a tile
#define GMX_AN_LINE 64    // a section of the packed buffer starts on a line
#define GMX_AN_HEAD 16    // bytes of a stream's header line: bits_seen, rows captured

// (include/gmxmix_analysis.h: GMX_AN_INPUT, GMX_AN_MIXER, GMX_AN_FINAL_P)
#define GMX_AN_K_INPUT 0u
#define GMX_AN_K_MIXER 1u
#define GMX_AN_K_FINAL_P 2u

// Bits of a call until its first capture, counted from the call's first bit: the smallest t with bits_seen + t > 0 and
// (bits_seen + t) % F == 0.  ~0 for F = 0.
__host__ __device__ inline uint64_t gmx_an_first(uint64_t bits_seen, uint64_t F) {
  if (F == 0) return ~0ull;
  const uint64_t rem = bits_seen % F;
  return rem ? F - rem : (bits_seen ? 0ull : F);
}
// Rows a call of n bits captures.
__host__ __device__ inline uint64_t gmx_an_captures(uint64_t bits_seen, uint64_t F, uint64_t n) {
  const uint64_t first = gmx_an_first(bits_seen, F);
  return n > first ? (n - 1 - first) / F + 1 : 0ull;
}

// The per-stream list of a launch, staged by the host from its mirror: [4][S].
enum { GMX_AN_L_NBITS = 0, GMX_AN_L_SEEN = 1, GMX_AN_L_ROWS = 2, GMX_AN_L_FREQ = 3, GMX_AN_L_COUNT = 4 };

struct GmxAnArgs {
  double* ema;             // [S][C]
  double* rows;            // [S][max_samples][C]
  uint64_t* labels;        // [S][max_samples]
  const uint32_t* cols;    // [C][2]: kind, index
  // a batch's arrays ...
  const float* pred;       // [S][pitch][n_pad]
  const uint32_t* mask;    // [S][pitch][mask_words], or NULL: every slot active
  const float* out;        // [S][pitch][m]
  const float* p;          // [S][pitch]
  // ... or the caller's values, a logit (FINAL_P: a probability) per column
  const float* values;     // [S][pitch][C]
  const uint8_t* bits;     // [S][pitch]
  const uint64_t* list;    // [GMX_AN_L_COUNT][S]
  uint64_t pitch;
  uint32_t n_pad, mask_words, m, n_columns, max_samples;
  int32_t n_streams;
};
// The take's list: [3][S] bits_seen, rows captured, byte offset of the stream's section in the packed body.
struct GmxAnPackArgs {
  const double* ema;
  const double* rows;
  const uint64_t* labels;
  const uint64_t* list;
  uint8_t* packed;         // pinned host, as the device sees it: [S] header lines, then the body
  uint64_t body_off;       // bytes of the header part, a multiple of GMX_AN_LINE
  uint32_t n_columns, max_samples;
  int32_t n_streams;
};

extern "C" {
hipError_t gmx_launch_analysis(const GmxAnArgs* a, hipStream_t stream);
// ema[s0 .. s0 + n)[C] = src[C] (NULL: zeros)
hipError_t gmx_launch_analysis_reset(double* ema, const double* src, int s0, int n, uint32_t n_columns, hipStream_t stream);
hipError_t gmx_launch_analysis_pack(const GmxAnPackArgs* a, hipStream_t stream);
}

#endif  // GMX_ANALYSIS_DEV_H_
