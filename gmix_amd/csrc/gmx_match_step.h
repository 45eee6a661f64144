// gmx_match_step.h -- device code shared by gmx_match.hip and gmx_indirect.hip: the eight-lane reductions of the
// Match kernels, and ONE lock-step bit of the Match models of a stream for a group of eight lanes
// (gmx_chainstep.inc; lane k of the group = model k).
//
// The arithmetic is gmx_match_kernel's, restated for one step whose coded bit arrives a launch after its forward
// (coder/decoder.cpp:19-39).  What the stream asks of the step is in `what`:
//   GMX_STEP_LEARN (1)    the history push of BasicContexts::Learn (basic-contexts.cpp:44-53) and K x Match::Learn
//                         (match.cpp:76-109) with the coded bit, on the bit_context and match_length_ the stream's
//                         last Predict left in the bank; longest_match is recomputed from the stored match_length_s
//                         as the batched kernel's learn-only path does
//   GMX_STEP_PREDICT (2)  K x Match::Predict (match.cpp:25-74) on this step's bit_context; the context words are
//                         read when the bit opens a byte or when the host says so (8: the stream's first predict)
// Learn comes first.  Everything is loaded from and stored to the bank every step: a stream may move between the lock
// step, gmx_match_run and gmx_match_forward / _learn between bits.
//
// Three phases, so that a host kernel can put them beside its own trips to memory; every load of a phase depends
// only on what the phase before it brought:
//   begin  the model's and the stream's state, the step's context word, bit_context and bit
//   fetch  match_length_ of this step's Predict follows from the state alone, so both probabilities (the Learn's
//          and the Predict's), the Learn's count and the Predict's table entry are requested together
//   look   Match::Learn's arithmetic, cur_match_, and the request for the history byte
//   finish the prediction, longest_match, the stores
// The two hand-overs of the batched kernel go through registers here as well: the byte the Learn pushes may be
// history[cur_match_] of the Predict (never loaded: the store goes out in `finish`), and the table entry the Learn
// writes may be the one the Predict reads (the entry is requested before the store, and patched).  A third one is
// this file's own: at match_length_ 255 the Predict reads the probability the Learn has just moved.
//
// `fetch` and `finish` hold the reductions over the group: every lane of the wave must call them, from wave-uniform
// control flow.  Lanes of models beyond K, and lanes whose stream sits the step out, take part in the reductions and
// touch no memory.  No LDS, no scratch (`make report-match`).
#ifndef GMX_MATCH_STEP_H_
#define GMX_MATCH_STEP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmx_match.h"
#include "gmx_math.h"

// max / or over the eight lanes of a group (lanes 8g .. 8g+7 of a row of 16): xor 1, xor 2 by quad_perm, then the
// other quad by row_half_mirror.  Every lane of the wave must be executing.
template <bool OR>
__device__ __forceinline__ uint32_t gmx_match_grp8(uint32_t v) {
  uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
  v = OR ? (v | o) : (v > o ? v : o);
  o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);           // quad_perm [2,3,0,1]
  v = OR ? (v | o) : (v > o ? v : o);
  o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);          // row_half_mirror
  v = OR ? (v | o) : (v > o ? v : o);
  return v;
}

#define GMX_MATCH_STEP_LEARN 1u    // = GMX_STEP_LEARN
#define GMX_MATCH_STEP_PREDICT 2u  // = GMX_STEP_PREDICT
#define GMX_MATCH_STEP_TAKE_CTX 8u // the context words of the step's record are read whatever the bit_context

// One lane's share of a step, between the phases.
struct GmxMatchStepLane {
  GmxMatchModelDev md;
  uint32_t* tab;
  float* prob;
  int32_t* cnt;
  GmxMatchModelState* msp;
  GmxMatchStreamState* ssp;
  uint8_t* hist;
  uint64_t hist_cap;
  bool live, lead, do_learn, do_pred;
  // the step's record
  uint32_t bit, bc, rctx, take;
  // the bank's state
  uint32_t cur_match, ctx, cur_byte, bit_pos, ml, hist_size, new_bit, cur_bc;
  float slot_value;
  // between the phases
  bool pushed, opens, active;
  uint32_t push_pos, push_byte, idx_old, idx_new, entry, ml_new, ctx_new, hbyte;
  float p_old, p_new, p_upd;
  int32_t c_old, c_upd;
  bool cnt_moved;
};

// begin: `what` = the stream's control word (0: it sits the step out); in_group: this lane belongs to a stream.
__device__ __forceinline__ void gmx_match_step_begin(GmxMatchStepLane& m, const GmxMatchDev* __restrict__ dv,
                                                     const GmxMatchStepArgs& a, int s, int k, bool in_group,
                                                     uint32_t what) {
  const int K = dv->k;
  m.live = in_group && k < K && (what & (GMX_MATCH_STEP_LEARN | GMX_MATCH_STEP_PREDICT)) != 0;
  m.lead = m.live && k == 0;
  m.do_learn = m.live && (what & GMX_MATCH_STEP_LEARN) != 0;
  m.do_pred = m.live && (what & GMX_MATCH_STEP_PREDICT) != 0;
  m.take = what & GMX_MATCH_STEP_TAKE_CTX;
  const int kk = m.live ? k : 0;
  const uint64_t ss = (uint64_t)(m.live ? s : 0);
  uint8_t* const bank = a.banks + ss * dv->bank_bytes;
  m.md = dv->m[kk];
  m.tab = (uint32_t*)(bank + m.md.tab_off);
  m.prob = (float*)(bank + dv->pred_off) + 256 * kk;
  m.cnt = (int32_t*)(bank + dv->cnt_off) + 256 * kk;
  m.msp = (GmxMatchModelState*)(bank + dv->mstate_off) + kk;
  m.ssp = (GmxMatchStreamState*)(bank + dv->sstate_off);
  m.hist = a.hist + ss * dv->hist_cap;
  m.hist_cap = dv->hist_cap;
  m.bit = m.bc = m.rctx = 0;
  m.cur_match = m.ctx = m.cur_byte = m.ml = m.hist_size = m.new_bit = m.cur_bc = 0;
  m.bit_pos = 128;
  m.slot_value = 0.0f;
  if (m.live) {
    const GmxMatchModelState st = *m.msp;
    const GmxMatchStreamState sst = *m.ssp;
    m.bit = a.bits[ss] & 1u;
    m.bc = a.bc[ss];
    m.rctx = a.ctx[ss * (uint64_t)K + kk];
    m.cur_match = st.cur_match;
    m.ctx = st.ctx;
    m.slot_value = st.slot_value;
    m.cur_byte = st.cur_byte;
    m.bit_pos = st.bit_pos;
    m.ml = st.match_length;
    m.hist_size = sst.hist_size;
    m.new_bit = sst.new_bit;
    m.cur_bc = sst.bit_context;
  }
}

// fetch: (all lanes of the wave)
__device__ __forceinline__ void gmx_match_step_fetch(GmxMatchStepLane& m) {
  // ShortTermMemory::longest_match as the stream's last Predict left it
  const uint32_t lm_old = gmx_match_grp8<false>(m.live ? m.ml >> 5 : 0u);
  // ---- BasicContexts::Learn's push (basic-contexts.cpp:50-52): recent_bits >= 128 and longest_match < 2
  m.pushed = m.do_learn && m.cur_bc >= 127u && lm_old < 2u && (uint64_t)m.hist_size < m.hist_cap;
  m.push_pos = 0xffffffffu;
  m.push_byte = 0;
  m.idx_old = 0;
  if (m.pushed) {
    m.push_byte = (((m.cur_bc + 1u) << 1) | m.bit) & 255u;
    m.push_pos = m.hist_size;
    m.idx_old = m.ctx % m.md.table_size;
    ++m.hist_size;
  }
  m.p_old = 0.0f;
  m.c_old = 0;
  if (m.do_learn && m.ml > 2u) {
    m.p_old = m.prob[m.ml];
    m.c_old = m.cnt[m.ml];
  }
  // ---- Match::Predict up to where it reads memory (match.cpp:25-52)
  m.ml_new = m.ml;
  m.ctx_new = m.ctx;
  m.opens = false;
  m.entry = 0;
  m.idx_new = 0;
  m.p_new = 0.0f;
  if (m.do_pred) {
    const uint32_t nb = m.do_learn ? m.bit : m.new_bit;
    const uint32_t expect = (m.cur_byte & m.bit_pos) != 0 ? 1u : 0u;
    if (nb == expect) {
      if (m.ml_new < 255u) ++m.ml_new;
    } else {
      m.ml_new = 0;
    }
    m.opens = m.bc == 0;  // recent_bits == 1
    if (m.opens || m.take) m.ctx_new = m.rctx;
    if (m.opens) {
      if (m.hist_size != 0 && m.cur_match == m.hist_size - 1u) m.ml_new = 0;  // (an empty history compares with 2^64 - 1)
      if (m.ml_new < 8u) {
        m.idx_new = m.ctx_new % m.md.table_size;
        m.entry = m.tab[m.idx_new];
      }
    }
    if (m.ml_new > 2u) m.p_new = m.prob[m.ml_new];
  }
}

// look: Match::Learn's arithmetic, cur_match_, and the history byte on its way
__device__ __forceinline__ void gmx_match_step_look(GmxMatchStepLane& m) {
  m.p_upd = m.p_old;
  m.c_upd = m.c_old;
  m.cnt_moved = false;
  if (m.do_learn && m.ml > 2u) {  // ---- Match::Learn (match.cpp:76-99)
    const int match = (m.bit == ((m.cur_byte & m.bit_pos) != 0 ? 1u : 0u)) ? 1 : 0;
    float rate = m.md.rate_at_limit;
    if (m.c_old < m.md.limit) {
      m.c_upd = m.c_old + 1;
      m.cnt_moved = true;
      rate = (float)(1.0 / (double)m.c_upd);
    }
    const float d = (float)match - m.p_old;
    m.p_upd = m.p_old + d * rate;
    if (m.do_pred && m.ml_new == m.ml) m.p_new = m.p_upd;  // (match_length_ 255 stays 255)
  }
  m.hbyte = m.cur_byte;
  if (m.do_pred) {
    m.bit_pos >>= 1;
    if (m.opens) {
      if (m.ml_new < 8u)
        m.cur_match = (m.pushed && m.idx_new == m.idx_old) ? m.hist_size - 1u : m.entry;
      else
        ++m.cur_match;
      if (m.hist_size != 0) {
        if (m.cur_match == m.push_pos)
          m.hbyte = m.push_byte;
        else if (m.cur_match < m.hist_size)  // (always: no run produces a pointer at or beyond the size)
          m.hbyte = m.hist[m.cur_match];
      }
      m.bit_pos = 128;
    }
  }
}

// finish: (all lanes of the wave) the prediction and the stores.  Returns longest_match of the step's Predict;
// m.active: ShortTermMemory::SetPrediction marked the slot (the caller owns the mask words).
__device__ __forceinline__ uint32_t gmx_match_step_finish(GmxMatchStepLane& m, const GmxMatchStepArgs& a, int s) {
  m.active = false;
  const uint32_t ml_learnt = m.ml;  // where Match::Learn counts and moves the probability
  if (m.do_pred) {
    m.cur_byte = m.hbyte;
    m.ml = m.ml_new;
    m.ctx = m.ctx_new;
    if (m.ml > 2u) {
      const float p = (m.cur_byte & m.bit_pos) ? m.p_new : 1.0f - m.p_new;
      m.slot_value = gmx_logit(p);  // ShortTermMemory::SetPrediction (short-term-memory.cpp:187-191):
      m.active = p != 0.5f;         // the slot is written, but a prediction of exactly 0.5 is not marked active
    }
    m.cur_bc = m.bc;
  }
  // ShortTermMemory::longest_match: BasicContexts::Predict zeroes it, every Match raises it
  const uint32_t lm = gmx_match_grp8<false>(m.do_pred ? m.ml >> 5 : 0u);
  if (m.do_pred) {
    const uint64_t ss = (uint64_t)s;
    a.mx_pred[ss * (uint64_t)a.mx_n_pad + (uint32_t)m.md.slot] = m.slot_value;
    if (m.lead)
      for (int c = 0; c < a.n_ctx_cols; ++c) a.mx_ctx[ss * (uint64_t)a.mx_m + a.ctx_cols[c]] = lm;
  }
  if (m.do_learn) {
    if (m.pushed && m.lead) m.hist[m.push_pos] = (uint8_t)m.push_byte;
    if (ml_learnt > 2u) {
      if (m.cnt_moved) m.cnt[ml_learnt] = m.c_upd;
      m.prob[ml_learnt] = m.p_upd;
    }
    if (m.pushed) m.tab[m.idx_old] = m.hist_size - 1u;  // match.cpp:100-108
    m.new_bit = m.bit;
  }
  if (m.live) {
    GmxMatchModelState st;
    st.cur_match = m.cur_match;
    st.ctx = m.ctx;
    st.slot_value = m.slot_value;
    st.cur_byte = (uint8_t)m.cur_byte;
    st.bit_pos = (uint8_t)m.bit_pos;
    st.match_length = (uint8_t)m.ml;
    st.pad = 0;
    *m.msp = st;
  }
  if (m.lead) {
    GmxMatchStreamState st;
    st.hist_size = m.hist_size;
    st.new_bit = m.new_bit;
    st.bit_context = m.cur_bc;
    st.pad = 0;
    *m.ssp = st;
  }
  return lm;
}

#endif  // GMX_MATCH_STEP_H_
