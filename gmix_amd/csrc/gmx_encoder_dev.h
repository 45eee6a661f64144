// gmx_encoder_dev.h -- what gmx_encoder.hip and gmx_encoder.inc share: a stream's record on the device, the header line
// a take brings home, the kernels' arguments and their launchers.
#ifndef GMX_ENCODER_DEV_H_
#define GMX_ENCODER_DEV_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define GMX_ENC_WAVE 64   // streams of a wave: a lane per stream
#define GMX_ENC_TILE 64   // bits of a tile
#define GMX_ENC_LINE 64   // a section of the packed buffer starts on a line

// One stream of a gmx_encoder.  32 bytes; the take's header line is a copy of it as it was before the round closed.
struct GmxEncStream {
  uint32_t x1, x2;     // Encoder's x1_, x2_
  uint32_t n_round;    // bytes in the stream's output area: coded since the last take
  uint32_t n_pack;     // bytes of the round the running take packs
  uint64_t total;      // bytes since the reset (tellp)
  int64_t bad_bit;     // first bit since the reset whose p was outside [0, 1], or -1
};
// (bits coded since the reset: bad_bit counts from there)
struct GmxEncArgs {
  GmxEncStream* streams;
  uint64_t* n_coded;        // [S]
  uint32_t* out;            // [S][area_words]
  const float* p;           // [S][pitch]
  const uint8_t* bits;      // [S][pitch]
  const uint64_t* n_bits;   // [S]
  uint64_t pitch;
  uint32_t area_words;
  int32_t n_streams;
};
struct GmxEncPackArgs {
  GmxEncStream* streams;
  const uint32_t* out;      // [S][area_words]
  uint64_t* offsets;        // [S] device: byte offset of the stream's section in the packed body
  uint8_t* packed;          // pinned host, as the device sees it: [S] header lines of 32 bytes, then the body
  uint64_t body_off;        // bytes of the header part, a multiple of GMX_ENC_LINE
  uint32_t area_words;
  int32_t n_streams;
};

extern "C" {
hipError_t gmx_launch_encoder(const GmxEncArgs* a, hipStream_t stream);
hipError_t gmx_launch_encoder_flush(const GmxEncArgs* a, const uint8_t* which, hipStream_t stream);
hipError_t gmx_launch_encoder_reset(GmxEncStream* streams, uint64_t* n_coded, int s0, int n, uint32_t x1, uint32_t x2,
                                    hipStream_t stream);
hipError_t gmx_launch_encoder_pack(const GmxEncPackArgs* a, hipStream_t stream);
}

#endif  // GMX_ENCODER_DEV_H_
