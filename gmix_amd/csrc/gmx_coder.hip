// gmx_coder.hip -- the arithmetic decoder and ModPPMD's range walk on the device (gmx_coder.h), as a phase in front of
// the context bank's lock-step bit: the kernels that let the lock-step chain decode a whole byte per call
// (gmx_chainstep_byte, gmx_coder.inc).
//
// A byte graph is eight steps of the chain and a tail.  Step j's first kernel is gmx_coder_step_kernel, a wave per
// stream, in place of gmx_ctx_step_kernel:
//   j > 1  lane 0 decodes bit j-1 from the probability the mixers' kernel of step j-1 left in device memory
//          (Decoder::Decode; the renormalisation reads the stream's resident compressed input)
//   all j  it writes what the host would have written into the step's device copy: bits, what_dev, dec, seq, tl_learn,
//          tl_pred, the stream's prediction row -- zero but for ModPPMD's slot, from the range walk -- and its mask
//          words, ModPPMD's bit alone
//   then   the context bank's bit with the decoded bit (gmx_ctx_step_core takes `what` and the bit as values)
// so a coded bit costs no graph node more than a per-bit step has.  gmx_coder_tail_kernel is the ninth launch: it
// decodes bit 7 and stores the byte, its eight p and the coder state into pinned host memory, the step number behind
// them, a lane per stream.  A stream that sits the byte out gets what_dev = 0 in all eight steps.
#include <hip/hip_runtime.h>

#include "gmx_coder_dev.h"
#include "gmx_ctx_step.h"

#define GMX_CODER_LEARN 1u
#define GMX_CODER_PREDICT 2u

// Lane 0's share of step j for stream s: the decoded bit and what the stream asks of the step.  sh: {what, bit, slot
// value, slot active}.
__device__ __forceinline__ void gmx_coder_lane0(const GmxCoderStepArgs& a, int s, const float* pr, uint32_t* sh) {
  GmxCoderStream* const cst = a.streams + s;
  uint32_t what = 0u, bit = 0u;
  // (read where it lies: a register copy of the block would be indexed by j, which is scratch)
  const GmxCoderByteIn* const cur = a.j == 1 ? a.byte_in + s : &cst->cur;
  const uint32_t take = cur->take, seq0 = cur->seq0;
  const float dec = cur->dec[a.j - 1];
  if (a.j == 1) {
    cst->cur = *cur;
    if (take) {
      what = cur->w_first;
      bit = cur->b_first & 1u;
      cst->acc = 0u;
      gmx_coder_walk_open(&cst->walk);
    }
  } else {
    if (take) {
      const float p = a.p_prev[s];
      GmxCoderState st = cst->st;
      bit = gmx_coder_decode(&st, p, cst->input, cst->in_len);
      cst->st = st;
      cst->p[a.j - 2] = p;
      cst->acc = (cst->acc << 1) | bit;
      what = GMX_CODER_LEARN | GMX_CODER_PREDICT;
      gmx_coder_walk_bit(&cst->walk, bit);
    }
  }
  float slot = 0.0f;
  bool active = false;
  if (take) {
    slot = cst->slot;
    const GmxCoderWalk w = cst->walk;
    if (gmx_coder_walk_predict(&w, pr, &slot, &active)) cst->slot = slot;
  }
  a.bits[s] = (uint8_t)bit;
  a.what[s] = (uint8_t)what;
  a.dec[s] = dec;
  a.seq[s] = seq0 + (uint32_t)a.j;
  a.tl_learn[s] = (what & GMX_CODER_LEARN) ? 1ull : 0ull;
  a.tl_pred[s] = (what & GMX_CODER_PREDICT) ? 1ull : 0ull;
  sh[0] = what;
  sh[1] = bit;
  sh[2] = __float_as_uint(slot);
  sh[3] = active ? 1u : 0u;
}

__global__ __launch_bounds__(64) void gmx_coder_step_kernel(const GmxCtxDev* __restrict__ dv, const GmxCoderStepArgs a) {
  __shared__ uint32_t stage[GMX_CTX_MAX_VARS];
  __shared__ __attribute__((aligned(16))) float pr[256];
  __shared__ uint32_t sh[4];
  const int s = (int)blockIdx.x, lane = (int)threadIdx.x;
  // the stream's byte distribution for the walk (the running byte's `take` is the first step's to read)
  const uint32_t take = a.j == 1 ? (uint32_t)a.byte_in[s].take : (uint32_t)a.streams[s].cur.take;
  if (take) ((float4*)pr)[lane] = ((const float4*)(a.ppm + (size_t)s * 256))[lane];
  __syncthreads();
  if (lane == 0) gmx_coder_lane0(a, s, pr, sh);
  __syncthreads();
  const uint32_t what = sh[0], bit = sh[1];
  if (!(what & (GMX_CODER_LEARN | GMX_CODER_PREDICT))) return;  // (block-uniform)
  // the record of the step: every slot but ModPPMD's is a device model's or inactive
  float* const row = a.pred + (size_t)s * a.n_pad;
  for (int c = lane; c < a.n_pad; c += 64) row[c] = c == a.slot ? __uint_as_float(sh[2]) : 0.0f;
  uint32_t* const mw = a.mask + (size_t)s * a.mask_words;
  for (int w = lane; w < a.mask_words; w += 64) mw[w] = (w == (a.slot >> 5) && sh[3]) ? 1u << (a.slot & 31) : 0u;
  gmx_ctx_step_core(dv, a.ctx.banks + (size_t)s * dv->bank_bytes, what, bit, lane, stage, a.ctx.tg, (size_t)s,
                    a.ctx.bc ? a.ctx.bc + s : nullptr);
}

// The ninth launch of a byte: bit 7 from step 8's probability, and the answers.  Every stream is stamped, also one that
// sat the byte out: the host waits for S stamps.
__global__ __launch_bounds__(64) void gmx_coder_tail_kernel(const GmxCoderStepArgs a) {
  const int s = (int)(blockIdx.x * 64u + threadIdx.x);  // (a lane per stream: nothing here is a wave's work)
  if (s >= a.ctx.n_streams) return;
  GmxCoderStream* const cst = a.streams + s;
  const uint32_t take = cst->cur.take, seq0 = cst->cur.seq0;
  if (take) {
    const float p = a.p_prev[s];
    GmxCoderState st = cst->st;
    const uint32_t bit = gmx_coder_decode(&st, p, cst->input, cst->in_len);
    cst->st = st;
    cst->p[7] = p;
    const uint32_t byte = ((cst->acc << 1) | bit) & 0xffu;
    cst->acc = byte;
    a.out_byte[s] = (uint8_t)byte;
    for (int i = 0; i < 8; ++i) a.out_p[8 * (size_t)s + i] = cst->p[i];
    a.out_state[4 * (size_t)s + 0] = st.x1;
    a.out_state[4 * (size_t)s + 1] = st.x2;
    a.out_state[4 * (size_t)s + 2] = st.x;
    a.out_state[4 * (size_t)s + 3] = st.pos;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __hip_atomic_store(a.stamp + s, seq0 + 8u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

extern "C" hipError_t gmx_launch_coder_step(const GmxCtxDev* dv, const GmxCoderStepArgs* args, hipStream_t stream) {
  (void)hipGetLastError();
  if (args->ctx.n_streams < 1 || args->j < 1 || args->j > 8 || args->slot < 0 || args->slot >= args->n_pad)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_coder_step_kernel, dim3((unsigned)args->ctx.n_streams), dim3(64), 0, stream, dv, *args);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_coder_tail(const GmxCoderStepArgs* args, hipStream_t stream) {
  (void)hipGetLastError();
  if (args->ctx.n_streams < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_coder_tail_kernel, dim3((unsigned)((args->ctx.n_streams + 63) / 64)), dim3(64), 0, stream, *args);
  return hipGetLastError();
}
