// gmx_ctx_step.h -- one lock-step bit of a context bank (gmx_chainstep_attach_ctx), as a function the 64 threads of a
// one-wave block call for one stream: gmx_ctx_step_kernel (gmx_ctx.hip) hosts it today; it is a header so that another
// launch of the step can host it in idle lanes later, as gmx_match_step.h is hosted.
//
// What the stream asks is in `what` (the values of GMX_STEP_*):
//   LEARN    the board's new_bit becomes bits[s]
//   PREDICT  exactly one record of gmx_ctx_run: new_bit is folded into recent_bits; when that completes a byte -- or on
//            the stream's very first Predict -- the ring takes the byte and every SKIP, INTERVAL and INDIRECT_HASH
//            variable fires; the routed columns of the step's records and bit_contexts[s] are written, and the board
// Lane v < V holds variable v.  RECENT_BYTE and BYTE_PLUS_RECENT are views of the ring (gmx_ctx_blackboard_set admits
// no other board), so the board keeps full values -- what gmx_ctx_blackboard_get returns -- and nothing has to be taken
// back out of them: a bit that opens no byte reads the board's SKIP / INTERVAL / INDIRECT_HASH values and adds the bit
// context where a variable moves within a byte.  No lane loops over anything but its own SKIP bytes.
#ifndef GMX_CTX_STEP_H_
#define GMX_CTX_STEP_H_

#include <hip/hip_runtime.h>

#include "gmx_ctx.h"

#define GMX_CTX_STEP_LEARN 1u    // GMX_STEP_LEARN
#define GMX_CTX_STEP_PREDICT 2u  // GMX_STEP_PREDICT

__device__ __forceinline__ uint32_t gmx_ctx_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ __forceinline__ uint32_t gmx_ctx_murmur_round(uint32_t h, uint32_t k) {
  k *= 0xcc9e2d51u;
  k = gmx_ctx_rotl32(k, 15);
  k *= 0x1b873593u;
  h ^= k;
  h = gmx_ctx_rotl32(h, 13);
  return h * 5u + 0xe6546b64u;
}
__device__ __forceinline__ uint32_t gmx_ctx_murmur_fmix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  return h ^ (h >> 16);
}
// MurmurHash3_x86_32 (public domain, A. Appleby) of the 4 / 8 little-endian bytes of a key, seed 0xDEADBEEF
__device__ __forceinline__ uint32_t gmx_ctx_murmur4(uint32_t k) {
  return gmx_ctx_murmur_fmix(gmx_ctx_murmur_round(0xDEADBEEFu, k) ^ 4u);
}
__device__ __forceinline__ uint32_t gmx_ctx_murmur8(uint64_t k) {
  return gmx_ctx_murmur_fmix(
      gmx_ctx_murmur_round(gmx_ctx_murmur_round(0xDEADBEEFu, (uint32_t)k), (uint32_t)(k >> 32)) ^ 8u);
}

// stage: GMX_CTX_MAX_VARS words of LDS.  Every thread of the block calls it (two block barriers for a stream that
// predicts; `what` is the stream's, so the branches around them are block-uniform).
__device__ __forceinline__ void gmx_ctx_step_body(const GmxCtxDev* __restrict__ dv, const GmxCtxStepArgs& a, int s,
                                                  int lane, uint32_t* stage) {
  const uint32_t w = a.what[s];
  if (!(w & (GMX_CTX_STEP_LEARN | GMX_CTX_STEP_PREDICT))) return;
  uint8_t* const bank = a.banks + (size_t)s * dv->bank_bytes;
  GmxCtxBoard* const bd = (GmxCtxBoard*)(bank + dv->board_off);
  const uint32_t nb = (w & GMX_CTX_STEP_LEARN) ? (uint32_t)a.bits[s] : bd->new_bit;
  if (!(w & GMX_CTX_STEP_PREDICT)) {
    if (lane == 0) bd->new_bit = nb;
    return;
  }
  // BasicContexts::Predict (basic-contexts.cpp:28-40): the first one returns early, nothing of the blackboard moves
  const uint32_t fp = bd->first_prediction;
  uint32_t rb = fp ? bd->recent_bits : 2u * bd->recent_bits + nb;
  uint32_t pos = bd->pos, byte = 0;
  const bool took = rb >= 256u;
  if (took) {
    byte = rb - 256u;
    rb = 1u;
    pos = pos + 1u == GMX_CTX_RING ? 0u : pos + 1u;
  }
  const bool opens = rb == 1u;
  const uint32_t bc = rb - 1u;
  // recent_bytes[k] as of this Predict (the completed byte is not in the ring yet)
  auto recent = [&](uint32_t k) -> uint32_t {
    const uint32_t at = pos >= k ? pos - k : pos + GMX_CTX_RING - k;
    return (took && k == 0u) ? byte : (uint32_t)bd->ring[at];
  };
  const int V = dv->v;
  uint32_t val = 0;
  if (lane < V) {
    const GmxCtxVarDev* const vd = &dv->var[lane];
    switch (vd->kind) {
      case GMX_CTXK_BIT_CONTEXT:
        val = bc;
        break;
      case GMX_CTXK_RECENT_BYTE:
        val = recent((uint32_t)vd->index);
        break;
      case GMX_CTXK_BYTE_PLUS_RECENT:
        val = (recent((uint32_t)vd->index) << 8) + bc;
        break;
      case GMX_CTXK_INTERVAL:
        val = bd->values[lane];
        if (opens)  // interval-context.cpp:15-18
          val = (uint32_t)((1ull << vd->num_bits) - 1ull) & ((val << vd->shift) + (uint32_t)dv->maps[vd->index][recent(0)]);
        break;
      case GMX_CTXK_SKIP:
        if (opens) {  // skip-context.cpp:9-18
          uint64_t key = 0;
          for (int i = 0; i < vd->n_bytes; ++i) key = (key << 8) + recent((uint32_t)vd->bytes_to_use[i]);
          val = gmx_ctx_murmur8(key);
        } else {
          val = bd->values[lane];
        }
        break;
      case GMX_CTXK_INDIRECT_HASH:
        if (opens) {
          // IndirectHash::Predict (indirect-hash.cpp:18-30), as in gmx_ctx_chain_kernel: the entry at the old index
          // takes the byte (its address is known from the stored state: that load waits for nothing of this step), the
          // state moves, and the entry at the new index is the one dependent load -- none when the index stays.  A
          // table is touched by its own lane only: the load behind the store is one lane's program order.
          const GmxCtxHashDev* const hd = &dv->hash[vd->index];
          uint32_t* const tab = (uint32_t*)(bank + hd->tab_off);
          GmxCtxHashState* const hs = (GmxCtxHashState*)(bank + dv->hstate_off) + vd->index;
          const uint32_t lb = recent(0), size = hd->table_size;
          const uint32_t idx = hs->outer_hash % size;
          uint32_t cur = ((tab[idx] & hd->inner_mask) << 8) + lb;
          tab[idx] = cur;
          const uint64_t oc = ((hs->outer_context & (uint64_t)hd->outer_mask) << 8) + lb;
          const uint32_t oh = gmx_ctx_murmur8(oc);
          const uint32_t idx2 = oh % size;
          if (idx2 != idx) cur = tab[idx2];
          hs->outer_context = oc;
          hs->outer_hash = oh;
          val = gmx_ctx_murmur4(cur);
        } else {
          val = bd->values[lane];
        }
        break;
      default:  // ZERO
        break;
    }
    stage[lane] = val;
  }
  __syncthreads();  // the values are staged, and every lane has read the board of the Predict before
  // the records of this step: lanes along the columns, column c takes the value of lane route[c]
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const GmxCtxTarget& tg = a.tg[k];
    if (!tg.ctx) continue;
    uint32_t* const out = tg.ctx + (size_t)s * (size_t)tg.n_cols;
    for (int c = lane; c < tg.n_cols; c += 64) {
      const int rt = tg.route[c];
      if (rt >= 0) out[c] = stage[rt];
    }
  }
  if (lane < V) bd->values[lane] = val;
  if (lane == 0) {
    if (a.bc) a.bc[s] = bc;
    if (took) bd->ring[pos] = (uint8_t)byte;
    bd->recent_bits = rb;
    bd->new_bit = nb;
    bd->first_prediction = 0;
    bd->pos = pos;
  }
  __syncthreads();  // (a host that goes on in the same block may reuse `stage`)
}

#endif  // GMX_CTX_STEP_H_
