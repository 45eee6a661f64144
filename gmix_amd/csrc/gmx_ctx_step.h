// gmx_ctx_step.h -- one lock-step bit of a context bank (gmx_chainstep_attach_ctx), as a function the 64 threads of a
// one-wave block call for one stream: gmx_ctx_step_kernel (gmx_ctx.hip) hosts it for the lock step, gmx_ctx_bit_kernel
// for the per-bit surface (gmx_ctx_forward / gmx_ctx_learn); and, at the end of the file, the same bit as a phase of a
// persistent wave that keeps the board's small state in registers (gmx_ctx_step_wave, hosted by
// gmx_indirect_session_kernel: gmx_indirect_attach_ctx).
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

// One bit of one stream whose bank is `bank`: `w` is what the stream asks (LEARN and / or PREDICT: the caller has seen to
// that), `bit` the bit a LEARN takes.  tg (nullable): the three targets of the step, their records indexed by `row`;
// bc_out (nullable): where bit_context goes.  stage: GMX_CTX_MAX_VARS words of LDS, which hold the V values of a
// Predict afterwards.  Every thread of the block calls it (two block barriers for a stream that predicts; `w` is the
// stream's, so the branches around them are block-uniform).
__device__ __forceinline__ void gmx_ctx_step_core(const GmxCtxDev* __restrict__ dv, uint8_t* const bank, uint32_t w,
                                                  uint32_t bit, int lane, uint32_t* stage, const GmxCtxTarget* tg,
                                                  size_t row, uint32_t* bc_out) {
  GmxCtxBoard* const bd = (GmxCtxBoard*)(bank + dv->board_off);
  const uint32_t nb = (w & GMX_CTX_STEP_LEARN) ? bit : bd->new_bit;
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
  if (tg) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (!tg[k].ctx) continue;
      uint32_t* const out = tg[k].ctx + row * (size_t)tg[k].n_cols;
      for (int c = lane; c < tg[k].n_cols; c += 64) {
        const int rt = tg[k].route[c];
        if (rt >= 0) out[c] = stage[rt];
      }
    }
  }
  if (lane < V) bd->values[lane] = val;
  if (lane == 0) {
    if (bc_out) *bc_out = bc;
    if (took) bd->ring[pos] = (uint8_t)byte;
    bd->recent_bits = rb;
    bd->new_bit = nb;
    bd->first_prediction = 0;
    bd->pos = pos;
  }
  __syncthreads();  // (a host that goes on in the same block may reuse `stage`)
}

// The lock step's bit of stream s: what it asks is in a.what[s], the bit a LEARN takes in a.bits[s].
__device__ __forceinline__ void gmx_ctx_step_body(const GmxCtxDev* __restrict__ dv, const GmxCtxStepArgs& a, int s,
                                                  int lane, uint32_t* stage) {
  const uint32_t w = a.what[s];
  if (!(w & (GMX_CTX_STEP_LEARN | GMX_CTX_STEP_PREDICT))) return;
  gmx_ctx_step_core(dv, a.banks + (size_t)s * dv->bank_bytes, w, (w & GMX_CTX_STEP_LEARN) ? (uint32_t)a.bits[s] : 0u,
                    lane, stage, a.tg, (size_t)s, a.bc ? a.bc + s : nullptr);
}

// ---- the same bit in a persistent wave (gmx_indirect_session_kernel<.., WITH_CTX>) ----------------------------------------
// The wave keeps a write-through copy of the board's small state in registers across commands: recent_bits, new_bit,
// first_prediction, pos, and per lane `base`, what the lane's variable is made of between byte openings -- the full
// value of an INTERVAL, SKIP or INDIRECT_HASH variable, the ring byte of a RECENT_BYTE / BYTE_PLUS_RECENT one (read
// from the ring, like gmx_ctx_step_core does, not from the board's values).  Every change is stored to the bank in the
// same command, so nothing of the stream lives outside the bank when the command is answered; a bit that opens no
// byte loads nothing from the bank.  At a byte opening the lanes read the ring and, per hash lane, the table: the
// old-index load waits for nothing of the step, the new-index load is the one dependent load.
struct GmxCtxWaveCopy {
  uint32_t rb, nb, fp, pos, base;
  bool loaded;
};

// All 64 lanes call it, from wave-uniform control flow; `what` is the command's ctx_what word (gmx_ctx.h) with PREDICT
// set or LEARN alone.  kind / index: of the lane's variable (lane < V), in registers.  Returns bit_context; stage[v]
// holds the V values afterwards (the caller puts a barrier between this and its reads).
__device__ __forceinline__ uint32_t gmx_ctx_step_wave(const GmxCtxDev* __restrict__ dv, uint8_t* const bank,
                                                      GmxCtxBoard* const bd, int V, int kind, int index,
                                                      GmxCtxWaveCopy& c, int lane, uint32_t what, uint32_t* stage) {
  const bool mine = lane < V;
  const bool bytevar = kind == GMX_CTXK_RECENT_BYTE || kind == GMX_CTXK_BYTE_PLUS_RECENT;
  if (!c.loaded || (what & GMX_CTX_WAVE_RELOAD)) {
    c.rb = bd->recent_bits;
    c.nb = bd->new_bit;
    c.fp = bd->first_prediction;
    c.pos = bd->pos;
    c.base = 0;
    if (mine) {
      const uint32_t k = (uint32_t)index;
      c.base = bytevar ? (uint32_t)bd->ring[c.pos >= k ? c.pos - k : c.pos + GMX_CTX_RING - k] : bd->values[lane];
    }
    c.loaded = true;
  }
  if (what & GMX_CTX_STEP_LEARN) c.nb = (what >> GMX_CTX_WAVE_BIT_SHIFT) & 1u;
  if (!(what & GMX_CTX_STEP_PREDICT)) {
    if (lane == 0) bd->new_bit = c.nb;
    return 0;
  }
  uint32_t rb = c.fp ? c.rb : 2u * c.rb + c.nb;
  uint32_t pos = c.pos, byte = 0;
  const bool took = rb >= 256u;
  if (took) {
    byte = rb - 256u;
    rb = 1u;
    pos = pos + 1u == GMX_CTX_RING ? 0u : pos + 1u;
  }
  const bool opens = rb == 1u;
  const uint32_t bc = rb - 1u;
  auto recent = [&](uint32_t k) -> uint32_t {  // (the completed byte is not in the ring yet)
    const uint32_t at = pos >= k ? pos - k : pos + GMX_CTX_RING - k;
    return (took && k == 0u) ? byte : (uint32_t)bd->ring[at];
  };
  uint32_t base = c.base, val = 0;
  if (mine) {
    if (opens) {
      const GmxCtxVarDev* const vd = &dv->var[lane];
      switch (kind) {
        case GMX_CTXK_RECENT_BYTE:
        case GMX_CTXK_BYTE_PLUS_RECENT:
          base = recent((uint32_t)index);
          break;
        case GMX_CTXK_INTERVAL:  // interval-context.cpp:15-18
          base = (uint32_t)((1ull << vd->num_bits) - 1ull) & ((base << vd->shift) + (uint32_t)dv->maps[index][recent(0)]);
          break;
        case GMX_CTXK_SKIP: {  // skip-context.cpp:9-18
          uint64_t key = 0;
          const int nbytes = vd->n_bytes;
          for (int i = 0; i < nbytes; ++i) key = (key << 8) + recent((uint32_t)vd->bytes_to_use[i]);
          base = gmx_ctx_murmur8(key);
          break;
        }
        case GMX_CTXK_INDIRECT_HASH: {  // indirect-hash.cpp:18-30, as in gmx_ctx_step_core
          const GmxCtxHashDev* const hd = &dv->hash[index];
          uint32_t* const tab = (uint32_t*)(bank + hd->tab_off);
          GmxCtxHashState* const hs = (GmxCtxHashState*)(bank + dv->hstate_off) + index;
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
          base = gmx_ctx_murmur4(cur);
          break;
        }
        default:
          break;
      }
    }
    val = kind == GMX_CTXK_BIT_CONTEXT        ? bc
          : kind == GMX_CTXK_BYTE_PLUS_RECENT ? (base << 8) + bc
          : kind == GMX_CTXK_ZERO             ? 0u
                                              : base;
    stage[lane] = val;
    bd->values[lane] = val;
  }
  if (lane == 0) {
    if (took) bd->ring[pos] = (uint8_t)byte;
    bd->recent_bits = rb;
    bd->new_bit = c.nb;
    bd->first_prediction = 0;
    bd->pos = pos;
  }
  c.rb = rb;
  c.fp = 0;
  c.pos = pos;
  c.base = base;
  return bc;
}

// A wave restarted between a forward and its learn does not step the bank again: the board holds the full values of
// that Predict, and recent_bits - 1 is its bit_context.
__device__ __forceinline__ uint32_t gmx_ctx_step_wave_replay(const GmxCtxBoard* bd, int V, int lane, uint32_t* stage) {
  if (lane < V) stage[lane] = bd->values[lane];
  return bd->recent_bits - 1u;
}

#endif  // GMX_CTX_STEP_H_
