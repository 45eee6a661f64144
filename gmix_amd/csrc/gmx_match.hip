// gmx_match.hip -- the reference's Match models (models/match.cpp) and the history rule of
// BasicContexts::Learn (contexts/basic-contexts.cpp:44-53) for S streams on gfx950.
//
// Lane mapping: lane = (stream, model), eight lanes per stream, eight streams per wave, one wave per block.  A
// model's table, its 256 probabilities and its 256 counts are touched by its own lane only; the lanes of a stream
// share the history (pushed by the stream's lane 0, read by all eight) and longest_match (a maximum over the eight
// lanes by DPP, no LDS).
//
// Order of one bit, as Predictor runs it (predictor.cpp:366-368, :383-387; BasicContexts comes before the Match
// objects in both loops):
//   Predict  match test against the previous bit, match_length_, bit_pos_ /= 2; at a byte's first bit the
//            end-of-history reset, the table lookup or ++cur_match_, the history byte; the prediction when
//            match_length_ > 2; longest_match = max(match_length_ / 32).
//   Learn    the history push when the byte is complete and longest_match < 2; count and probability at
//            match_length_; the table entry of this byte's context when the byte was pushed.
//
// The two read-after-write cases:
//   * table[ctx % size] written at a byte's last Learn and read at the next byte's first Predict may be one entry
//     (runs of one byte value).  Writer and reader are the same lane and the entry is not fetched ahead: program
//     order of one lane.
//   * history[cur_match_] may be the byte the stream's lane 0 pushed at the preceding Learn: another lane's store.
//     Every lane of the group knows the newest pushed byte and its position and takes it from registers; before a
//     push is issued the wave waits for all its earlier memory operations (an explicit `s_waitcnt vmcnt(0)`; on
//     gfx9 stores count in vmcnt), so every push but the newest is complete -- written to the L2 through the CU's
//     write-through L1, which the wave's own later loads go through -- when a history byte is loaded.  The wait sits
//     directly in front of the global_store_byte in the generated code (checked in the ISA; `make report-match`).
//
// Arithmetic: one float subtraction and one multiply-add pair per learned bit, a double division for the rate
// (match.cpp:84-90), Sigmoid::Logit (gmx_math.h) for the prediction.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmx_ckpt_walk.h"
#include "gmx_match.h"
#include "gmx_match_step.h"
#include "gmx_math.h"

__global__ void __launch_bounds__(64) gmx_match_kernel(const GmxMatchDev* __restrict__ dv, const GmxMatchRunArgs a) {
  const int lane = (int)threadIdx.x;
  const int k = lane & 7;
  const int ls = (int)blockIdx.x * 8 + (lane >> 3);  // stream of the launch
  const int K = dv->k;
  const bool in_range = ls < a.n_streams;
  const bool live = in_range && k < K;
  const bool lead = in_range && k == 0;
  const uint64_t s = (uint64_t)(a.stream_base + (in_range ? ls : 0));
  const uint64_t rec = (uint64_t)(a.rec_base + (in_range ? ls : 0));
  const bool do_predict = (a.what & GMX_MATCH_PREDICT) != 0, do_learn = (a.what & GMX_MATCH_LEARN) != 0;

  // bits of this lane's stream, and the most any stream of the wave has (uniform loop bound)
  uint64_t T = 0, Tmax = 0;
  if (a.T_list) {
    for (int i = 0; i < 8; ++i) {
      const int q = (int)blockIdx.x * 8 + i;
      const uint64_t tq = q < a.n_streams ? a.T_list[q] : 0;
      Tmax = tq > Tmax ? tq : Tmax;
      if (i == (lane >> 3)) T = tq;
    }
  } else {
    Tmax = a.T;
    T = in_range ? a.T : 0;
  }

  uint8_t* const bank = a.banks + s * dv->bank_bytes;
  const GmxMatchModelDev md = dv->m[live ? k : 0];
  uint32_t* const tab = (uint32_t*)(bank + md.tab_off);
  float* const prob = (float*)(bank + dv->pred_off) + 256 * (live ? k : 0);
  int32_t* const cnt = (int32_t*)(bank + dv->cnt_off) + 256 * (live ? k : 0);
  GmxMatchModelState* const msp = (GmxMatchModelState*)(bank + dv->mstate_off) + k;
  GmxMatchStreamState* const ssp = (GmxMatchStreamState*)(bank + dv->sstate_off);
  uint8_t* const hist = a.hist + s * dv->hist_cap;

  const uint32_t* const ctx_s = a.ctx + rec * a.rec_stride * (uint64_t)K + (live ? k : 0);
  const uint32_t* const bc_s = a.bc + rec * a.rec_stride;
  const uint8_t* const bits_s = a.bits + rec * a.rec_stride;

  uint32_t cur_match = 0, ctx = 0, cur_byte = 0, bit_pos = 128, ml = 0;
  float slot_value = 0.0f;
  uint32_t hist_size = 0, new_bit = 0, cur_bc = 0;
  if (live) {
    const GmxMatchModelState st = *msp;
    cur_match = st.cur_match;
    ctx = st.ctx;
    slot_value = st.slot_value;
    cur_byte = st.cur_byte;
    bit_pos = st.bit_pos;
    ml = st.match_length;
  }
  if (in_range) {
    const GmxMatchStreamState st = *ssp;
    hist_size = st.hist_size;
    new_bit = st.new_bit;
    cur_bc = st.bit_context;
  }
  uint32_t push_pos = 0xffffffffu, push_byte = 0;  // the newest push of this launch

  // bits of the attached mask that belong to this lane's slot
  const int MW = a.mx_mask ? a.mx_mask_words : 0;
  const uint32_t my_word = (uint32_t)md.slot >> 5, my_bit = 1u << ((uint32_t)md.slot & 31u);

  // the records of the next bit travel while this one is worked on
  uint32_t n_bc = 0, n_bit = 0, n_ctx = 0;
  if (T > 0) {
    if (do_predict) {
      n_bc = bc_s[0];
      if (live) n_ctx = ctx_s[0];
    }
    n_bit = bits_s[0];
  }

  for (uint64_t t = 0; t < Tmax; ++t) {
    const bool on = t < T;
    const uint32_t bc = do_predict ? n_bc : cur_bc, bit = n_bit & 1u, rctx = n_ctx;
    if (t + 1 < T) {
      if (do_predict) {
        n_bc = bc_s[t + 1];
        if (live) n_ctx = ctx_s[(t + 1) * (uint64_t)K];
      }
      n_bit = bits_s[t + 1];
    }
    float p_cur = 0.0f;  // predictions[match_length_], read once per bit
    bool active = false;
    if (do_predict && on && live) {
      // ---- Match::Predict (match.cpp:25-74)
      const uint32_t expect = (cur_byte & bit_pos) != 0 ? 1u : 0u;
      if (new_bit == expect) {
        if (ml < 255u) ++ml;
      } else {
        ml = 0;
      }
      bit_pos >>= 1;
      // the aliased variable does not move within a byte; a launch that begins inside one takes it from its
      // first record, so that nothing but Match's own fields has to survive a checkpoint
      if (bc == 0 || t == 0) ctx = rctx;
      if (bc == 0) {  // recent_bits == 1
        if (hist_size != 0 && cur_match == hist_size - 1u) ml = 0;  // (an empty history compares with 2^64 - 1)
        if (ml < 8u)
          cur_match = tab[ctx % md.table_size];
        else
          ++cur_match;
        if (hist_size != 0) {
          if (cur_match == push_pos)
            cur_byte = push_byte;
          else if (cur_match < hist_size)  // (always: no run produces a pointer at or beyond the size)
            cur_byte = hist[cur_match];
        }
        bit_pos = 128;
      }
      if (ml > 2u) {
        p_cur = prob[ml];
        const float p = (cur_byte & bit_pos) ? p_cur : 1.0f - p_cur;
        slot_value = gmx_logit(p);  // ShortTermMemory::SetPrediction (short-term-memory.cpp:187-191):
        active = p != 0.5f;         // the slot is written, but a prediction of exactly 0.5 is not marked active
      }
      cur_bc = bc;
    } else if (on && live && ml > 2u) {
      p_cur = prob[ml];  // learn alone: the forward of this bit ran in an earlier launch
    }
    // ShortTermMemory::longest_match: BasicContexts::Predict zeroes it, every Match raises it
    const uint32_t lm = gmx_match_grp8<false>(live ? ml >> 5 : 0u);

    if (do_predict && on) {
      const uint64_t r = rec * a.rec_stride + t;
      if (live) {
        if (a.pred_out) {
          a.pred_out[r * (uint64_t)K + k] = slot_value;
          a.act_out[r * (uint64_t)K + k] = active ? 1 : 0;
        }
      }
      if (lead && a.longest_out) a.longest_out[r] = lm;
    }
    if (a.mx_pred && do_predict) {  // (uniform)
      const uint64_t r = rec * a.mx_rec_stride + t;
      if (on && live) a.mx_pred[r * (uint64_t)a.mx_n_pad + (uint32_t)md.slot] = slot_value;
      for (int w = 0; w < MW; ++w) {
        const uint32_t clr = gmx_match_grp8<true>(live && my_word == (uint32_t)w ? my_bit : 0u);
        const uint32_t set = gmx_match_grp8<true>(live && active && my_word == (uint32_t)w ? my_bit : 0u);
        if (on && lead && clr) {
          uint32_t* const mw = a.mx_mask + r * (uint64_t)MW + w;
          *mw = (*mw & ~clr) | set;
        }
      }
      if (on && lead)
        for (int c = 0; c < a.n_ctx_cols; ++c) a.mx_ctx[r * (uint64_t)a.mx_m + a.ctx_cols[c]] = lm;
    }

    if (do_learn && on && in_range) {
      const bool byte_done = cur_bc >= 127u;          // recent_bits >= 128: this bit completes the byte
      const bool pushed = byte_done && lm < 2u;       // basic-contexts.cpp:50-52
      if (pushed) {
        const uint32_t byte = (((cur_bc + 1u) << 1) | bit) & 255u;
        if (lead) {
          // The pushes before this one are complete: a counted wait, spelled out.  (A workgroup-scope fence
          // compiles to nothing here -- the workgroup is one wave.)  The memory clobber keeps the compiler from
          // moving the store across it.
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          hist[hist_size] = (uint8_t)byte;
        }
        push_pos = hist_size;
        push_byte = byte;
        ++hist_size;
      }
      if (live) {
        // ---- Match::Learn (match.cpp:76-109)
        if (ml > 2u) {
          const int match = (bit == ((cur_byte & bit_pos) != 0 ? 1u : 0u)) ? 1 : 0;
          float rate = md.rate_at_limit;
          int c = cnt[ml];
          if (c < md.limit) {
            ++c;
            cnt[ml] = c;
            rate = (float)(1.0 / (double)c);
          }
          const float d = (float)match - p_cur;
          prob[ml] = p_cur + d * rate;
        }
        if (pushed) tab[ctx % md.table_size] = hist_size - 1u;
      }
      new_bit = bit;
    }
  }

  if (live) {
    GmxMatchModelState st;
    st.cur_match = cur_match;
    st.ctx = ctx;
    st.slot_value = slot_value;
    st.cur_byte = (uint8_t)cur_byte;
    st.bit_pos = (uint8_t)bit_pos;
    st.match_length = (uint8_t)ml;
    st.pad = 0;
    *msp = st;
  }
  if (lead) {
    GmxMatchStreamState st;
    st.hist_size = hist_size;
    st.new_bit = new_bit;
    st.bit_context = cur_bc;
    st.pad = 0;
    *ssp = st;
  }
}

// One lock-step bit of every stream (gmx_chainstep.inc) where the Indirect models' step kernel cannot carry the Match
// lanes (no Indirect models, or more than 56 of them): gmx_match_step.h's group of eight lanes, eight streams per wave
// as above, one node of the step's graph in front of the mixers' kernel.  The mask words of the mixers' record are
// read-modify-written in place: nobody else writes them in this node (the LSTM's bit step ran in an earlier one), and
// the host left the models' bits clear.
__global__ void __launch_bounds__(64) gmx_match_step_kernel(const GmxMatchDev* __restrict__ dv, const GmxMatchStepArgs a) {
  const int lane = (int)threadIdx.x;
  const int k = lane & 7;
  const int s = (int)blockIdx.x * 8 + (lane >> 3);
  const bool in_range = s < a.n_streams && k < dv->k;
  const uint32_t what = in_range ? a.what[s] : 0u;
  GmxMatchStepLane m;
  gmx_match_step_begin(m, dv, a, s, k, in_range, what);
  gmx_match_step_fetch(m);
  gmx_match_step_look(m);
  gmx_match_step_finish(m, a, s);
  const int MW = a.mx_mask_words;  // (uniform)
  const uint32_t my_word = (uint32_t)m.md.slot >> 5, my_bit = 1u << ((uint32_t)m.md.slot & 31u);
  for (int w = 0; w < MW; ++w) {
    const uint32_t set = gmx_match_grp8<true>(m.active && my_word == (uint32_t)w ? my_bit : 0u);
    if (m.lead && m.do_pred && set) a.mx_mask[(uint64_t)s * (uint64_t)MW + w] |= set;
  }
}

// Constructed state (match.cpp:3-23, long-term-memory.h:42-53): tables zero, predictions[i] =
// float(0.5 + (i + 0.5) / 512) computed in double, counts 1, bit_pos_ 128, everything else 0.
// grid: x = blocks striding over the bank, y = stream
__global__ void __launch_bounds__(256) gmx_match_init_kernel(const GmxMatchDev* __restrict__ dv, uint8_t* banks,
                                                            int stream_base) {
  uint8_t* const bank = banks + (uint64_t)(stream_base + (int)blockIdx.y) * dv->bank_bytes;
  const uint64_t first = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
  uint4* const t4 = (uint4*)bank;  // (table offsets and sizes are multiples of 256 bytes)
  for (uint64_t i = first; i < dv->tab_bytes / 16; i += stride) t4[i] = make_uint4(0, 0, 0, 0);
  if (blockIdx.x == 0) {
    const int i = (int)threadIdx.x;
    const float p0 = (float)(0.5 + ((double)i + 0.5) / 512.0);
    for (int k = 0; k < GMX_MATCH_MAX_MODELS; ++k) {
      if (k < dv->k) {
        ((float*)(bank + dv->pred_off))[256 * k + i] = p0;
        ((int32_t*)(bank + dv->cnt_off))[256 * k + i] = 1;
      }
    }
    if (i < GMX_MATCH_MAX_MODELS) {
      GmxMatchModelState st;
      st.cur_match = 0;
      st.ctx = 0;
      st.slot_value = 0.0f;
      st.cur_byte = 0;
      st.bit_pos = 128;
      st.match_length = 0;
      st.pad = 0;
      ((GmxMatchModelState*)(bank + dv->mstate_off))[i] = st;
    }
    if (i == 0) {
      GmxMatchStreamState st;
      st.hist_size = 0;
      st.new_bit = 0;
      st.bit_context = 0;
      st.pad = 0;
      *(GmxMatchStreamState*)(bank + dv->sstate_off) = st;
    }
  }
}

// ---- checkpoint: count, pack, scatter (cf. gmx_ind_ckpt.hip) ------------------------------------------------
__global__ void __launch_bounds__(256) gmx_match_ckpt_count_kernel(const GmxMatchCkptArgs a) {
  __shared__ uint32_t wsum[4];
  const GmxMatchCkptChunk ch = a.chunks[blockIdx.x];
  const GmxMatchModelDev& x = a.dev->m[ch.model];
  const uint32_t* tab = (const uint32_t*)(a.bank + x.tab_off) + ch.first_entry;
  const uint32_t end = gmx_walk_chunk_end(x.table_size, ch.first_entry, GMX_MATCH_CKPT_CHUNK);
  const uint32_t total = gmx_walk_block_count_u32(tab, end, wsum);
  if (threadIdx.x == 0) a.chunk_cnt[blockIdx.x] = total;
}

// Sparse model: records {u32 key, 5 pointer bytes} in ascending key order, ranked by the walk of gmx_ckpt_walk.h.
// Dense model: five bytes per entry.  Records are 9 and 5 bytes long: byte stores, every byte written by exactly
// one lane.
__global__ void __launch_bounds__(256) gmx_match_ckpt_pack_kernel(const GmxMatchCkptArgs a) {
  __shared__ uint32_t wsum[2][4];
  const uint32_t c = blockIdx.x;
  const GmxMatchCkptChunk ch = a.chunks[c];
  const GmxMatchModelDev& x = a.dev->m[ch.model];
  const uint32_t* tab = (const uint32_t*)(a.bank + x.tab_off) + ch.first_entry;
  const uint32_t end = gmx_walk_chunk_end(x.table_size, ch.first_entry, GMX_MATCH_CKPT_CHUNK);
  uint8_t* const out = a.buf + a.model_off[ch.model];
  if (a.model_dense[ch.model]) {
    for (uint32_t e = threadIdx.x; e < end; e += 256u) {
      uint8_t* o = out + 5ull * (ch.first_entry + e);
      gmx_walk_put_u32(o, tab[e]);
      o[4] = 0;
    }
    return;
  }
  uint8_t* const recs = out + 9ull * a.chunk_base[c];
  const uint32_t room = a.chunk_cnt[c];
  gmx_walk_pack_sparse_u32(tab, end, ch.first_entry, room, wsum, [recs](uint32_t r, uint32_t key, uint32_t v) {
    uint8_t* o = recs + 9ull * r;
    gmx_walk_put_u32(o, key);
    gmx_walk_put_u32(o + 4, v);
    o[8] = 0;
  });
}

// (the tables have been zeroed; the host has validated the section: keys ascending and below the table size)
// grid: x = blocks striding over a model's records or entries, y = model
__global__ void __launch_bounds__(256) gmx_match_ckpt_scatter_kernel(const GmxMatchCkptArgs a) {
  const uint32_t j = blockIdx.y;
  const GmxMatchModelDev& x = a.dev->m[j];
  uint32_t* tab = (uint32_t*)(a.bank + x.tab_off);
  const uint32_t size = x.table_size, mc = a.model_cnt[j];
  const uint8_t* in = a.buf + a.model_off[j];
  const uint64_t first = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
  if (!a.model_dense[j]) {
    for (uint64_t r = first; r < mc; r += stride) {
      const uint8_t* p = in + 9ull * r;
      const uint32_t key = gmx_walk_get_u32(p);
      if (key < size) tab[key] = gmx_walk_get_u32(p + 4);
    }
  } else {
    for (uint64_t e = first; e < size; e += stride) tab[e] = gmx_walk_get_u32(in + 5ull * e);
  }
}

extern "C" hipError_t gmx_launch_match_kernel(const GmxMatchDev* dv, const GmxMatchRunArgs* args, hipStream_t stream) {
  (void)hipGetLastError();
  if (args->n_streams < 1) return hipErrorInvalidValue;
  if (args->mx_pred && (args->mx_mask_words < 1 || args->mx_mask_words > GMX_MATCH_MAX_MASK_WORDS))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_match_kernel, dim3((unsigned)((args->n_streams + 7) / 8)), dim3(64), 0, stream, dv, *args);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_match_step(const GmxMatchDev* dv, const GmxMatchStepArgs* args, hipStream_t stream) {
  (void)hipGetLastError();
  if (args->n_streams < 1 || args->mx_mask_words < 1 || args->mx_mask_words > GMX_MATCH_MAX_MASK_WORDS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_match_step_kernel, dim3((unsigned)((args->n_streams + 7) / 8)), dim3(64), 0, stream, dv,
                     *args);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_match_init(const GmxMatchDev* dv, uint8_t* banks, int stream_base, int n_streams,
                                            hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_match_init_kernel, dim3(1024, (unsigned)n_streams), dim3(256), 0, stream, dv, banks,
                     stream_base);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_match_ckpt_count(const GmxMatchCkptArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_match_ckpt_count_kernel, dim3(a->n_chunks), dim3(256), 0, stream, *a);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_match_ckpt_pack(const GmxMatchCkptArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_match_ckpt_pack_kernel, dim3(a->n_chunks), dim3(256), 0, stream, *a);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_match_ckpt_scatter(const GmxMatchCkptArgs* a, int n_models, unsigned blocks_x,
                                                    hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_match_ckpt_scatter_kernel, dim3(blocks_x, (unsigned)n_models), dim3(256), 0, stream, *a);
  return hipGetLastError();
}
