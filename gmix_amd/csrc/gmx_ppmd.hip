// gmx_ppmd.hip -- the PPMd byte model on the device: one wave per stream.
//
// The model is gmx_ppmd.h, the same text the host builds.  A launch keeps the stream's state block (the free lists'
// heads, the model's scalars, both SEE tables, the symbol mask, sqp, the explicit stacks, the constant tables: 11 KB)
// in LDS from its first byte to its last; the arena stays in HBM.  Per byte:
//   UpdateByte         (of the byte before, which a record owes: gmx_ppmd_record) lane 0: pointer chasing through the arena, the allocator, rescale, the model flush
//   PrepareByte        the wave: per context of the suffix chain a lane per symbol -- one 16-bit load of {Symbol, Freq}
//                      each, the mask test in LDS, the masked frequency sum by a wave reduction, sqp by lanes (a 64-bit
//                      division each, all at once)
//   the distribution   float(max(sqp, 1)) by lanes, the reference's left-to-right float sum on one lane, 256 divisions
//                      by lanes, stored as 1 KiB coalesced
//   the bit walk       lanes 0..7, one bit of the known byte each (gmx_coder_walk_*)
// Every store to device memory is a plain vector store.
#include <hip/hip_runtime.h>

#include "gmx_coder.h"
#include "gmx_ppmd_dev.h"

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}

// One context of PrepareByte's chain by the wave: sqp of its unmasked symbols from `cum`, the mask, and the cum its
// escape leaves.  see_freq < 0: the unmasked context the chain begins with (its total is SummFreq, its escape what the
// symbols leave of it).  A symbol is in a table once, so lanes never meet in sqp or in the mask.
__device__ __forceinline__ uint32_t ppmd_context_wave(GmxPpmdState* st, const uint8_t* arena, uint32_t ctx, uint32_t cum,
                                                      int see_freq, int lane) {
  const uint32_t cnum = GMX_PP_NS(arena, ctx), tab = GMX_PP_STATS(arena, ctx);
  const uint32_t esc = st->esc_count;
  uint32_t sf[4];  // {Symbol, Freq} of states lane, lane + 64, ...; 0x10000: masked or beyond the table
  uint32_t part = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t i = (uint32_t)(64 * k + lane);
    sf[k] = 0x10000u;
    if (64u * k <= cnum && i <= cnum) {
      const uint32_t v = gmx_pp_ld16(arena, tab + 6u * i);
      if (see_freq < 0 || st->char_mask[v & 0xffu] != esc) {
        sf[k] = v;
        part += v >> 8;
      }
    }
  }
  const uint32_t low = wave_sum(part);
  const uint32_t total = see_freq < 0 ? GMX_PP_SUMM(arena, ctx) : (uint32_t)see_freq + low;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (sf[k] != 0x10000u) {
      const uint32_t sym = sf[k] & 0xffu;
      st->sqp[sym] = gmx_pp_scale(cum, sf[k] >> 8, total) + 1;
      st->char_mask[sym] = esc;
    }
  }
  return gmx_pp_scale(cum, see_freq < 0 ? total - low : (uint32_t)see_freq, total);
}

// gmx_ppmd_prepare_byte by the wave.  The chain's scalars (cum, NumMasked, the context) are wave-uniform registers;
// lane 0 stores what the model keeps (BSumm, EscCount, NumMasked).
__device__ __forceinline__ void ppmd_prepare_wave(GmxPpmdState* st, const uint8_t* arena, int lane) {
  for (int c = lane; c < 256; c += 64) st->sqp[c] = 0;
  __syncthreads();
  uint32_t cum = 0xffffff00u;
  uint32_t mc = st->max_ctx;
  int num_masked;
  if (GMX_PP_NS(arena, mc)) {
    num_masked = (int)GMX_PP_NS(arena, mc);
    cum = ppmd_context_wave(st, arena, mc, cum, -1, lane);
  } else {
    const int bsumm = *gmx_pp_bin_slot(st, arena, mc);
    const uint32_t sym = gmx_pp_ld8(arena, mc + 2), b2 = (uint32_t)(bsumm + bsumm);
    if (lane == 0) {
      st->bsumm = bsumm;
      st->sqp[sym] = gmx_pp_scale(cum, b2, 32768u) + 1;
      st->char_mask[sym] = st->esc_count;
    }
    cum = gmx_pp_scale(cum, 32768u - b2, 32768u);
    num_masked = 0;
  }
  for (;;) {
    __syncthreads();  // the mask and sqp of the context before
    bool end = false;
    do {
      const uint32_t up = GMX_PP_SUFFIX(arena, mc);
      if (!up) {
        end = true;
        break;
      }
      mc = up;
    } while ((int)GMX_PP_NS(arena, mc) == num_masked);
    if (end) break;
    // (gmx_pp_see_of with the chain's NumMasked)
    const uint32_t cnum = GMX_PP_NS(arena, mc);
    int see_freq = 1;
    if (cnum != 0xffu) {
      const GmxPpmdSee* e = st->see2[st->qtable[cnum + 3] - 4];
      e += (GMX_PP_SUMM(arena, mc) > 10 * (cnum + 1));
      e += 2 * (2 * cnum < GMX_PP_NS(arena, GMX_PP_SUFFIX(arena, mc)) + (uint32_t)num_masked) + GMX_PP_FLAGS(arena, mc);
      see_freq = (int)((uint32_t)e->summ >> e->shift) + 1;
    }
    cum = ppmd_context_wave(st, arena, mc, cum, see_freq, lane);
    num_masked = (int)cnum;
  }
  if (lane == 0) {
    st->esc_count++;
    st->num_masked = 0;
  }
  __syncthreads();
}

__device__ __forceinline__ void state_copy(uint32_t* dst, const uint32_t* src, int lane) {
  for (uint32_t i = (uint32_t)lane; i < sizeof(GmxPpmdState) / 4; i += 64) dst[i] = src[i];
}

}  // namespace

static_assert(sizeof(GmxPpmdState) % 8 == 0, "the state block is copied in words");

__global__ void __launch_bounds__(64) gmx_ppmd_kernel(const GmxPpmdRunArgs a) {
  __shared__ GmxPpmdState st;
  __shared__ float w[256];
  __shared__ float sum;
  const int s = a.stream_base + (int)blockIdx.x;
  const int lane = (int)threadIdx.x;
  const uint64_t n = a.n_list ? a.n_list[s] : a.n;
  if (n == 0) return;
  uint8_t* arena = a.arena + (uint64_t)s * a.arena_stride;
  state_copy((uint32_t*)&st, (const uint32_t*)(a.states + s), lane);
  __syncthreads();
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t byte = a.bytes[(uint64_t)s * a.byte_pitch + i];
    if (lane == 0) {
      if (a.explicit_last) {
        gmx_ppmd_update_byte(&st, arena, byte);
        st.pending = 0;
      } else {
        if (st.pending) gmx_ppmd_update_byte(&st, arena, st.last_byte);
        st.last_byte = (uint8_t)byte;
        st.pending = 1;
      }
    }
    __syncthreads();
    ppmd_prepare_wave(&st, arena, lane);
    for (int c = lane; c < 256; c += 64) w[c] = gmx_ppmd_weight(st.sqp[c]);
    __syncthreads();
    if (lane == 0) {
      float t = 0.0f;
      for (int c = 0; c < 256; ++c) t += w[c];
      sum = t;
    }
    __syncthreads();
    const uint64_t rec = (uint64_t)s * a.rec_pitch + i;
    const float total = sum;
    for (int c = lane; c < 256; c += 64) {
      const float p = w[c] / total;
      w[c] = p;
      a.ppm_out[rec * 256 + c] = p;
    }
    __syncthreads();
    if (a.pred_out && lane < 8) {
      GmxCoderWalk walk;
      gmx_coder_walk_open(&walk);
      for (int j = 1; j <= lane; ++j) gmx_coder_walk_bit(&walk, (byte >> (8 - j)) & 1u);
      // (every element of w is positive, so the walk always writes)
      float slot = 0.0f;
      bool active = false;
      (void)gmx_coder_walk_predict(&walk, w, &slot, &active);
      a.pred_out[rec * 8 + lane] = slot;
      a.act_out[rec * 8 + lane] = active ? 1 : 0;
    }
    if (a.used_out && lane == 0) a.used_out[rec] = 16 + gmx_ppmd_used_memory(&st);
    __syncthreads();
  }
  state_copy((uint32_t*)(a.states + s), (const uint32_t*)&st, lane);
}

// A stream as the reference's Init leaves it.  The arena has been zeroed.
__global__ void __launch_bounds__(64) gmx_ppmd_init_kernel(GmxPpmdState* states, uint8_t* arena, uint64_t arena_stride,
                                                           uint64_t arena_bytes, int order, int stream_base) {
  __shared__ GmxPpmdState st;
  const int s = stream_base + (int)blockIdx.x;
  const int lane = (int)threadIdx.x;
  for (uint32_t i = (uint32_t)lane; i < sizeof(GmxPpmdState) / 4; i += 64) ((uint32_t*)&st)[i] = 0;
  __syncthreads();
  if (lane == 0) gmx_ppmd_init(&st, arena + (uint64_t)s * arena_stride, order, arena_bytes);
  __syncthreads();
  state_copy((uint32_t*)(states + s), (const uint32_t*)&st, lane);
}

// The batch's results into the downstream models' batches: ppm into the LSTM batch's ppm column, the eight
// predictions of byte n into slot `slot` of the mixers' records 8n .. 8n+7 with their active bits.
__global__ void __launch_bounds__(256) gmx_ppmd_feed_kernel(const GmxPpmdFeedArgs a) {
  const int s = (int)blockIdx.y;
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (a.lstm_ppm && i < a.n_bytes * 256) {
    const uint64_t n = i >> 8, c = i & 255;
    a.lstm_ppm[((uint64_t)s * a.lstm_pitch + n) * 256 + c] = a.ppm[((uint64_t)s * a.rec_pitch + n) * 256 + c];
  }
  if (a.mx_pred && i < a.n_bytes * 8) {
    const uint64_t r = (uint64_t)s * a.mx_pitch + i, from = ((uint64_t)s * a.rec_pitch + (i >> 3)) * 8 + (i & 7);
    a.mx_pred[r * a.mx_n_pad + a.slot] = a.pred[from];
    uint32_t* word = a.mx_mask + r * a.mx_mask_words + (a.slot >> 5);
    const uint32_t m = 1u << (a.slot & 31);
    *word = a.act[from] ? (*word | m) : (*word & ~m);
  }
}

extern "C" hipError_t gmx_launch_ppmd_init(GmxPpmdState* states, uint8_t* arena, uint64_t arena_stride,
                                           uint64_t arena_bytes, int order, int stream_base, int n_streams,
                                           hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ppmd_init_kernel, dim3(n_streams), dim3(64), 0, stream, states, arena, arena_stride, arena_bytes,
                     order, stream_base);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_ppmd_run(const GmxPpmdRunArgs* args, int n_streams, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ppmd_kernel, dim3(n_streams), dim3(64), 0, stream, *args);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_ppmd_feed(const GmxPpmdFeedArgs* args, int n_streams, hipStream_t stream) {
  (void)hipGetLastError();
  const uint64_t work = args->n_bytes * (args->lstm_ppm ? 256 : 8);
  hipLaunchKernelGGL(gmx_ppmd_feed_kernel, dim3((unsigned)((work + 255) / 256), n_streams), dim3(256), 0, stream, *args);
  return hipGetLastError();
}
