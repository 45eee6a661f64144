// gmx_encoder.hip -- the arithmetic encoder on the device (gmx_encoder.h; host side gmx_encoder.inc, DESIGN.md section
// 4.22).  The chain over a stream's bits is serial, the streams are parallel:
//
//   gmx_encoder_kernel        a wave per 64 neighbouring streams, tiles of 64 bits.  Per tile the wave loads the 64
//                             streams' p and bits rows, the lanes running ALONG a row (256 and 64 bytes per request),
//                             discretizes all of them in parallel and lays the 16-bit pr and the bit into LDS, a row per
//                             stream (stride 65 words: the transposed read is conflict free).  Lane s then walks its own
//                             stream's row: Encoder::Encode per bit.  The bytes gather in a 64-bit register and leave in
//                             whole dwords for the stream's output area.
//   gmx_encoder_flush_kernel  Encoder::Flush, a lane per stream.
//   gmx_encoder_reset_kernel  the constructor's or ReadCheckpoint's two words, a lane per stream.
//   gmx_encoder_count_kernel  closes the round: the header line of every stream and the offset of its section in the
//                             packed buffer (sections start on 64-byte lines), one wave
//   gmx_encoder_pack_kernel   ... and the sections themselves, a wave per stream, in whole dwords into pinned host
//                             memory: what crosses the link is what was produced, not the areas' capacity.
#include <hip/hip_runtime.h>

#include "gmx_encoder.h"
#include "gmx_encoder_dev.h"

#define GMX_ENC_BAD 0x20000u
#define GMX_ENC_STRIDE (GMX_ENC_TILE + 1)

// A stream's output area as the walk sees it: the dword under construction and its place.
struct GmxEncOut {
  uint32_t* area;
  uint64_t acc;
  uint32_t n_acc, w, words;
};
__device__ __forceinline__ void gmx_enc_open(GmxEncOut& o, uint32_t* area, uint32_t words, uint32_t n_round) {
  o.area = area;
  o.words = words;
  o.w = n_round >> 2;
  o.n_acc = n_round & 3u;
  o.acc = (o.n_acc && o.w < words) ? (uint64_t)(area[o.w] & ((1u << (8u * o.n_acc)) - 1u)) : 0ull;
}
// k <= 4 bytes, the first in word's low byte (the host keeps a round within the area; the guard is for a caller's bug)
__device__ __forceinline__ void gmx_enc_put(GmxEncOut& o, uint32_t word, uint32_t k) {
  o.acc |= (uint64_t)word << (8u * o.n_acc);
  o.n_acc += k;
  if (o.n_acc >= 4u) {
    if (o.w < o.words) o.area[o.w] = (uint32_t)o.acc;
    ++o.w;
    o.acc >>= 32;
    o.n_acc -= 4u;
  }
}
__device__ __forceinline__ void gmx_enc_close(GmxEncOut& o) {
  if (o.n_acc && o.w < o.words) o.area[o.w] = (uint32_t)o.acc;
}

__global__ __launch_bounds__(GMX_ENC_WAVE) void gmx_encoder_kernel(const GmxEncArgs a) {
  __shared__ uint32_t tile[GMX_ENC_WAVE * GMX_ENC_STRIDE];
  const uint32_t lane = threadIdx.x;
  const int s0 = (int)blockIdx.x * GMX_ENC_WAVE, s = s0 + (int)lane;
  const bool live = s < a.n_streams;
  GmxEncStream rec = {0u, 0u, 0u, 0u, 0ull, -1};
  uint32_t n = 0u;
  if (live) {
    rec = a.streams[s];
    n = rec.bad_bit >= 0 ? 0u : (uint32_t)a.n_bits[s];
  }
  uint32_t nmax = n;
  for (int off = 32; off > 0; off >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, off));
  if (nmax == 0u) return;  // (wave-uniform)
  GmxEncoderState st = {rec.x1, rec.x2};
  GmxEncOut o;
  gmx_enc_open(o, a.out + (size_t)(live ? s : 0) * a.area_words, live ? a.area_words : 0u, rec.n_round);
  uint32_t coded = 0u, emitted = 0u;
  for (uint32_t t0 = 0u; t0 < nmax; t0 += GMX_ENC_TILE) {
    const uint32_t t = t0 + lane;
#pragma unroll 8
    for (int r = 0; r < GMX_ENC_WAVE; ++r) {
      const uint32_t nr = (uint32_t)__shfl((int)n, r);
      if (t < nr) {
        const size_t at = (size_t)(s0 + r) * a.pitch + t;
        const float p = a.p[at];
        const uint32_t b = a.bits[at] ? 1u : 0u;
        tile[r * GMX_ENC_STRIDE + lane] = gmx_encoder_p_ok(p) ? (gmx_coder_discretize(p) | (b << 16)) : GMX_ENC_BAD;
      }
    }
    __syncthreads();
    const uint32_t cnt = n > t0 ? min(n - t0, (uint32_t)GMX_ENC_TILE) : 0u;
    for (uint32_t i = 0u; i < cnt; ++i) {
      const uint32_t v = tile[lane * GMX_ENC_STRIDE + i];
      if (v & GMX_ENC_BAD) {  // the stream stops: state and output stay as after the bit before
        rec.bad_bit = (int64_t)(a.n_coded[s] + coded);
        n = 0u;
        break;
      }
      uint32_t word;
      const uint32_t k = gmx_encoder_bit_pr(&st, v >> 16, v & 0xffffu, &word);
      gmx_enc_put(o, word, k);
      emitted += k;
      ++coded;
    }
    __syncthreads();
  }
  if (!live || (coded == 0u && rec.bad_bit < 0)) return;
  gmx_enc_close(o);
  rec.x1 = st.x1;
  rec.x2 = st.x2;
  rec.n_round += emitted;
  rec.total += emitted;
  a.streams[s] = rec;
  a.n_coded[s] += coded;
}

__global__ __launch_bounds__(64) void gmx_encoder_flush_kernel(const GmxEncArgs a, const uint8_t* __restrict__ which) {
  const int s = (int)(blockIdx.x * 64u + threadIdx.x);
  if (s >= a.n_streams || (which && !which[s])) return;
  GmxEncStream rec = a.streams[s];
  if (rec.bad_bit >= 0) return;
  GmxEncoderState st = {rec.x1, rec.x2};
  GmxEncOut o;
  gmx_enc_open(o, a.out + (size_t)s * a.area_words, a.area_words, rec.n_round);
  uint32_t word;
  const uint32_t k = gmx_encoder_shift(&st, &word);
  gmx_enc_put(o, word, k);
  gmx_enc_put(o, st.x2 >> 24, 1u);
  gmx_enc_close(o);
  rec.x1 = st.x1;
  rec.x2 = st.x2;
  rec.n_round += k + 1u;
  rec.total += k + 1u;
  a.streams[s] = rec;
}

__global__ __launch_bounds__(64) void gmx_encoder_reset_kernel(GmxEncStream* streams, uint64_t* n_coded, int s0, int n,
                                                               uint32_t x1, uint32_t x2) {
  const int i = (int)(blockIdx.x * 64u + threadIdx.x);
  if (i >= n) return;
  GmxEncStream rec = {x1, x2, 0u, 0u, 0ull, -1};
  rec.n_pack = streams[s0 + i].n_pack;
  streams[s0 + i] = rec;
  n_coded[s0 + i] = 0ull;
}

// One wave: lane l owns the streams [l * per, (l + 1) * per).
__global__ __launch_bounds__(64) void gmx_encoder_count_kernel(const GmxEncPackArgs a) {
  const int lane = (int)threadIdx.x, S = a.n_streams;
  const int per = (S + 63) / 64, lo = min(S, lane * per), hi = min(S, lo + per);
  uint64_t sum = 0ull;
  for (int s = lo; s < hi; ++s)
    sum += ((uint64_t)a.streams[s].n_round + (GMX_ENC_LINE - 1)) & ~(uint64_t)(GMX_ENC_LINE - 1);
  uint64_t incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t lo32 = (uint32_t)__shfl_up((int)(uint32_t)incl, off), hi32 = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), off);
    if (lane >= off) incl += ((uint64_t)hi32 << 32) | lo32;
  }
  uint64_t at = incl - sum;
  for (int s = lo; s < hi; ++s) {
    GmxEncStream rec = a.streams[s];
    uint4* line = (uint4*)(a.packed + (size_t)s * sizeof(GmxEncStream));
    line[0] = make_uint4(rec.x1, rec.x2, rec.n_round, rec.n_pack);
    line[1] = make_uint4((uint32_t)rec.total, (uint32_t)(rec.total >> 32), (uint32_t)(uint64_t)rec.bad_bit,
                         (uint32_t)((uint64_t)rec.bad_bit >> 32));
    a.offsets[s] = at;
    at += ((uint64_t)rec.n_round + (GMX_ENC_LINE - 1)) & ~(uint64_t)(GMX_ENC_LINE - 1);
    a.streams[s].n_pack = rec.n_round;
    a.streams[s].n_round = 0u;
  }
}

__global__ __launch_bounds__(256) void gmx_encoder_pack_kernel(const GmxEncPackArgs a) {
  const int s = (int)(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
  if (s >= a.n_streams) return;
  const uint32_t words = min((a.streams[s].n_pack + 3u) >> 2, a.area_words);
  const uint32_t* src = a.out + (size_t)s * a.area_words;
  uint32_t* dst = (uint32_t*)(a.packed + a.body_off + a.offsets[s]);
  for (uint32_t i = (uint32_t)lane; i < words; i += 64u) dst[i] = src[i];
}

extern "C" hipError_t gmx_launch_encoder(const GmxEncArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  if (a->n_streams < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_encoder_kernel, dim3((unsigned)((a->n_streams + GMX_ENC_WAVE - 1) / GMX_ENC_WAVE)),
                     dim3(GMX_ENC_WAVE), 0, stream, *a);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_encoder_flush(const GmxEncArgs* a, const uint8_t* which, hipStream_t stream) {
  (void)hipGetLastError();
  if (a->n_streams < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_encoder_flush_kernel, dim3((unsigned)((a->n_streams + 63) / 64)), dim3(64), 0, stream, *a, which);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_encoder_reset(GmxEncStream* streams, uint64_t* n_coded, int s0, int n, uint32_t x1,
                                               uint32_t x2, hipStream_t stream) {
  (void)hipGetLastError();
  if (n < 1 || s0 < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_encoder_reset_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, streams, n_coded, s0,
                     n, x1, x2);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_encoder_pack(const GmxEncPackArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  if (a->n_streams < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_encoder_count_kernel, dim3(1), dim3(64), 0, stream, *a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gmx_encoder_pack_kernel, dim3((unsigned)((a->n_streams + 3) / 4)), dim3(256), 0, stream, *a);
  return hipGetLastError();
}
