// gmx_coder.inc -- a whole byte per call in the lock-step chain (included by gmx_capi.cpp behind gmx_chainstep.inc;
// include/gmxmix_decoder.h, DESIGN.md section 4.20).
//
// With every bank attached, what a per-bit step still needs from the host is the bit it decoded from the last p and
// ModPPMD's bit prediction.  gmx_chainstep_attach_decoder puts Decoder::Decode and ModPPMD's range walk on the device
// (gmx_coder.h, gmx_coder.hip) and captures two BYTE graphs, one per parity of the byte's first step: cs_record(opens)
// and seven times cs_record(!opens) with gmx_coder_step_kernel in place of the context bank's node, and the tail --
// one linear chain of kernels.  Inside a byte graph nothing comes from the host: the coder phase writes the step's
// control words and records into the device copy, the mixers' kernel leaves p in device memory for the next step's
// decode, and only the tail stores into pinned host memory (the byte, its eight p, the coder state, the stamps).
//
// gmx_chainstep_byte_launch does gmx_chainstep_launch's bookkeeping for eight steps at once, after a validation that
// touches nothing; per byte the host writes take[s], PPMd's distribution, and eight decay factors per stream.

#include <unordered_map>

static void cs_decoder_free(gmx_chainstep* cs) {
  gmx_cs_decoder* dc = cs->dc;
  if (!dc) return;
  for (int p = 0; p < 2; ++p) {
    if (dc->exec[p]) (void)hipGraphExecDestroy(dc->exec[p]);
    if (dc->graph[p]) (void)hipGraphDestroy(dc->graph[p]);
  }
  for (uint8_t* q : dc->input)
    if (q) (void)hipFree(q);
  void* dv[] = {dc->streams, dc->in_bar, dc->p_dev, dc->outs_dev, dc->stamp_dev};
  for (void* q : dv)
    if (q) (void)hipFree(q);
  if (dc->h_in) (void)hipHostFree(dc->h_in);
  if (dc->h_ans) (void)hipHostFree(dc->h_ans);
  delete dc;
  cs->dc = nullptr;
}

// The arguments of step j's coder phase (j = 9: the tail) on the device copy of parity `par`.
static hipError_t cs_coder_args(gmx_chainstep* cs, int par, int j, GmxCoderStepArgs* ca) {
  gmx_cs_decoder* dc = cs->dc;
  if (!dc || !cs->cb) return hipErrorInvalidValue;
  const GmxTopoDev& t = cs->g->topo;
  auto cur = [&](const void* host_ptr) { return cs->d_in[par] + ((const uint8_t*)host_ptr - cs->h_in); };
  auto ans = [&](const void* host_ptr) { return dc->ans_dev + ((const uint8_t*)host_ptr - dc->h_ans); };
  memset(ca, 0, sizeof *ca);
  ca->streams = dc->streams;
  ca->byte_in = dc->in_dev;
  ca->p_prev = dc->p_dev;
  ca->ppm = (const float*)(cs->d_bd + cs->bd_ppm_off);
  ca->bits = cur(cs->bits);
  ca->what = cur(cs->what_dev);
  ca->dec = (float*)cur(cs->dec);
  ca->seq = (uint32_t*)cur(cs->seq);
  ca->tl_learn = (uint64_t*)cur(cs->tl_learn);
  ca->tl_pred = (uint64_t*)cur(cs->tl_pred);
  ca->pred = (float*)cur(cs->pred);
  ca->mask = (uint32_t*)cur(cs->mask);
  ca->n_pad = t.n_pad;
  ca->mask_words = t.mask_words;
  ca->slot = dc->ppmd_slot;
  ca->j = j;
  ca->out_byte = ans(dc->decoded);
  ca->out_p = (float*)ans(dc->byte_p);
  ca->out_state = (uint32_t*)ans(dc->state);
  ca->stamp = (uint32_t*)(cs->d_out + ((const uint8_t*)cs->stamp - cs->h_out));
  GmxCtxStepArgs& x = ca->ctx;
  x.banks = cs->cb->banks;
  x.bits = (const uint8_t*)cur(cs->bits);
  x.what = (const uint8_t*)cur(cs->what_dev);
  x.bc = (cs->ib || cs->mb) ? (uint32_t*)cur(cs->ibc) : nullptr;
  x.n_streams = cs->S;
  const void* const rec[3] = {cs->ctx, cs->ictx, cs->mctx};
  for (int k = 0; k < 3; ++k) {
    x.tg[k] = cs->c_tg[k];
    x.tg[k].ctx = cs->c_tg[k].n_cols > 0 ? (uint32_t*)cur(rec[k]) : nullptr;
  }
  return hipSuccess;
}

// One byte as a stream of work on `st`: par0 is the parity of its first step.
static hipError_t cs_record_byte(gmx_chainstep* cs, hipStream_t st, int par0) {
  gmx_cs_decoder* dc = cs->dc;
  hipError_t e = hipSuccess;
  if (!cs->bar) {  // the distributions (and the LSTM's lists): the byte's first kernel reads them
    e = gmx_launch_copy16(cs->d_bd, cs->h_bd_dev, cs->bd_bytes / 16, st);
    if (e != hipSuccess) return e;
  }
  for (int j = 1; j <= 8; ++j) {
    const CsByteRoute br = {j, dc->p_dev, dc->outs_dev, dc->stamp_dev};
    e = cs_record(cs, st, j == 1, par0 ^ ((j - 1) & 1), &br);
    if (e != hipSuccess) return e;
  }
  GmxCoderStepArgs ca;
  e = cs_coder_args(cs, par0, 9, &ca);
  if (e != hipSuccess) return e;
  return gmx_launch_coder_tail(&ca, st);
}

extern "C" int gmx_chainstep_attach_decoder(gmx_chainstep* cs, int ppmd_slot) {
  if (!cs || !cs->g) return GMX_ERR_INVALID;
  if (cs->dc || cs->steps != 0 || cs->in_flight || cs->broken || cs->cb_gone || cs->mb_gone) return GMX_ERR_STATE;
  gmx_group* g = cs->g;
  const GmxTopoDev& t = g->topo;
  if (!cs->cb) return GMX_ERR_INVALID;  // the coder phase hosts the context bank's bit
  // every context word of a step has a writer on the device
  for (int c = 0; c < t.m; ++c) {
    bool owned = cs->c_tg[0].route[c] >= 0 || c == cs->mixer_ctx_col;
    for (int i = 0; i < cs->n_mcols; ++i) owned = owned || cs->mcols[i] == c;
    if (!owned) return GMX_ERR_INVALID;
  }
  if (cs->ib)
    for (int c = 0; c < cs->ib->dev.k; ++c)
      if (cs->c_tg[1].route[c] < 0 && c != cs->ind_ctx_col) return GMX_ERR_INVALID;
  if (cs->mb)
    for (int c = 0; c < cs->mb->dev.k; ++c)
      if (cs->c_tg[2].route[c] < 0) return GMX_ERR_INVALID;
  if (ppmd_slot < 0 || ppmd_slot >= t.n) return GMX_ERR_INVALID;
  if (cs->l && ppmd_slot == cs->lstm_slot) return GMX_ERR_INVALID;
  if (cs->ib)
    for (int i = 0; i < cs->ib->dev.k; ++i)
      if (cs->ib->dev.m[i].slot_a == ppmd_slot || cs->ib->dev.m[i].slot_b == ppmd_slot) return GMX_ERR_INVALID;
  if (cs->mb)
    for (int i = 0; i < cs->mb->dev.k; ++i)
      if (cs->mb->dev.m[i].slot == ppmd_slot) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(g->device));
  HIPCHK(hipStreamSynchronize(g->stream));
  gmx_cs_decoder* dc = new (std::nothrow) gmx_cs_decoder();
  if (!dc) return GMX_ERR_NOMEM;
  cs->dc = dc;
  dc->ppmd_slot = ppmd_slot;
  const size_t S = (size_t)cs->S;
#define DCHK(call)                                           \
  do {                                                       \
    hipError_t e_ = (call);                                  \
    if (e_ != hipSuccess) {                                  \
      int r_ = hip_fail(e_, #call);                          \
      cs_decoder_free(cs);                                   \
      return e_ == hipErrorOutOfMemory ? GMX_ERR_NOMEM : r_; \
    }                                                        \
  } while (0)
  dc->input.assign(S, nullptr);
  dc->st.assign(S, GmxCoderState{0u, 0xffffffffu, 0u, 0u});
  dc->has_input.assign(S, 0);
  dc->via_byte.assign(S, 0);
  dc->taking.assign(S, 0);
  DCHK(hipMalloc((void**)&dc->streams, S * sizeof(GmxCoderStream)));
  DCHK(hipMemset(dc->streams, 0, S * sizeof(GmxCoderStream)));
  DCHK(hipMalloc((void**)&dc->p_dev, S * sizeof(float)));
  DCHK(hipMemset(dc->p_dev, 0, S * sizeof(float)));
  DCHK(hipMalloc((void**)&dc->outs_dev, S * (size_t)t.m * sizeof(float)));
  DCHK(hipMalloc((void**)&dc->stamp_dev, S * sizeof(uint32_t)));
  const unsigned hflags = hipHostMallocMapped | hipHostMallocCoherent;
  DCHK(hipHostMalloc((void**)&dc->h_in, S * sizeof(GmxCoderByteIn), hflags));
  memset(dc->h_in, 0, S * sizeof(GmxCoderByteIn));
  if (cs->bar) {
    void* q = nullptr;
    DCHK(hipExtMallocWithFlags(&q, S * sizeof(GmxCoderByteIn), hipDeviceMallocFinegrained));
    dc->in_bar = (GmxCoderByteIn*)q;
    DCHK(hipMemset(dc->in_bar, 0, S * sizeof(GmxCoderByteIn)));
    dc->in_dev = dc->in_bar;
  } else {
    DCHK(hipHostGetDevicePointer((void**)&dc->in_dev, dc->h_in, 0));
  }
  {
    size_t o = 0;
    auto take = [&o](size_t n) {
      const size_t at = o;
      o += cs_round(n);
      return at;
    };
    const size_t a_take = take(S), a_dec = take(S), a_p = take(S * 8 * 4), a_st = take(S * 4 * 4);
    DCHK(hipHostMalloc((void**)&dc->h_ans, o, hflags));
    memset(dc->h_ans, 0, o);
    DCHK(hipHostGetDevicePointer((void**)&dc->ans_dev, dc->h_ans, 0));
    dc->take = dc->h_ans + a_take;
    dc->decoded = dc->h_ans + a_dec;
    dc->byte_p = (float*)(dc->h_ans + a_p);
    dc->state = (uint32_t*)(dc->h_ans + a_st);
  }
  // once outside a capture, with every stream sitting the byte out (take = 0 everywhere), as cs_capture does ...
  hipStream_t st = g->stream;
  DCHK(cs_record_byte(cs, st, 0));
  DCHK(hipStreamSynchronize(st));
  memset(cs->stamp, 0, S * sizeof(uint32_t));  // (... which stamped step 8: the object's steps count from 1)
  for (int par = 0; par < 2; ++par) {
    DCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const hipError_t e = cs_record_byte(cs, st, par);
    const hipError_t e2 = hipStreamEndCapture(st, &dc->graph[par]);
    DCHK(e);
    DCHK(e2);
    DCHK(hipGraphInstantiate(&dc->exec[par], dc->graph[par], nullptr, nullptr, 0));
  }
#undef DCHK
  return GMX_OK;
}

extern "C" float* gmx_chainstep_decoder_ppm(gmx_chainstep* cs) { return (cs && cs->dc) ? cs->ppm : nullptr; }
extern "C" uint8_t* gmx_chainstep_take(gmx_chainstep* cs) { return (cs && cs->dc) ? cs->dc->take : nullptr; }
extern "C" const uint8_t* gmx_chainstep_decoded(gmx_chainstep* cs) { return (cs && cs->dc) ? cs->dc->decoded : nullptr; }
extern "C" const float* gmx_chainstep_byte_p(gmx_chainstep* cs) { return (cs && cs->dc) ? cs->dc->byte_p : nullptr; }
extern "C" int64_t gmx_debug_chainstep_bit_launches(const gmx_chainstep* cs) {
  return cs ? (int64_t)cs->bit_launches : (int64_t)GMX_ERR_INVALID;
}

extern "C" int gmx_chainstep_decoder_set_input(gmx_chainstep* cs, int s, const void* data, size_t n,
                                               const uint32_t* state) {
  if (!cs || !cs->g || !cs->dc || s < 0 || s >= cs->S || (!data && n) || n > 0xffffffffull) return GMX_ERR_INVALID;
  if (state && state[3] > n) return GMX_ERR_INVALID;
  if (cs->in_flight) return GMX_ERR_STATE;
  gmx_cs_decoder* dc = cs->dc;
  gmx_group* g = cs->g;
  HIPCHK(hipSetDevice(g->device));
  HIPCHK(hipStreamSynchronize(g->stream));
  uint8_t* buf = nullptr;
  HIPCHK(hipMalloc((void**)&buf, n + 16));  // (never empty)
  hipError_t e = hipMemset(buf, 0, n + 16);
  if (e == hipSuccess && n) e = hipMemcpy(buf, data, n, hipMemcpyHostToDevice);
  GmxCoderState st;
  if (state) {
    st = GmxCoderState{state[0], state[1], state[2], state[3]};
  } else {
    gmx_coder_init(&st, (const uint8_t*)data, (uint32_t)n);
  }
  GmxCoderStream cst;
  if (e == hipSuccess) e = hipMemcpy(&cst, dc->streams + s, sizeof cst, hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    cst.st = st;
    cst.input = buf;
    cst.in_len = (uint32_t)n;
    e = hipMemcpy(dc->streams + s, &cst, sizeof cst, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    (void)hipFree(buf);
    HIPCHK(e);
  }
  if (dc->input[s]) (void)hipFree(dc->input[s]);
  dc->input[s] = buf;
  dc->st[s] = st;
  dc->has_input[s] = 1;
  return GMX_OK;
}

extern "C" int gmx_chainstep_decoder_state(gmx_chainstep* cs, int s, uint32_t out[4]) {
  if (!cs || !cs->dc || s < 0 || s >= cs->S || !out) return GMX_ERR_INVALID;
  if (cs->in_flight) return GMX_ERR_STATE;
  const GmxCoderState& st = cs->dc->st[s];
  out[0] = st.x1;
  out[1] = st.x2;
  out[2] = st.x;
  out[3] = st.pos;
  return GMX_OK;
}

// Behind the wait of a byte: what the per-bit bookkeeping knows of a stream after seven learned bits of its byte.
static void cs_decoder_answered(gmx_chainstep* cs) {
  gmx_cs_decoder* dc = cs->dc;
  dc->in_flight = false;
  for (int s = 0; s < cs->S; ++s) {
    if (!dc->taking[s]) continue;
    cs->acc[s] = (uint8_t)(dc->decoded[s] >> 1);
    const uint32_t* q = dc->state + 4 * (size_t)s;
    dc->st[s] = GmxCoderState{q[0], q[1], q[2], q[3]};
  }
}

extern "C" int gmx_chainstep_byte_launch(gmx_chainstep* cs) {
  if (!cs || !cs->g) return GMX_ERR_INVALID;
  if (!cs->dc || cs->in_flight || cs->mb_gone || cs->cb_gone || cs->broken || !cs->cb) return GMX_ERR_STATE;
  gmx_cs_decoder* dc = cs->dc;
  gmx_group* g = cs->g;
  const int S = cs->S;
  HIPCHK(hipSetDevice(g->device));
  // whatever gmx_ctx_* calls queued on the bank's own stream between the steps, and where they left the streams
  if (hipStreamQuery(cs->cb->stream) != hipSuccess) HIPCHK(hipStreamSynchronize(cs->cb->stream));
  (void)hipGetLastError();
  if (cs->cb->moved) {
    const int rcp = cs_read_positions(cs, cs->cb);
    if (rcp) return rcp;
    cs->cb->moved = false;
  }
  // validation: nothing is written before it has passed
  bool any = false;
  std::vector<uint8_t> first_bit(S, 0);
  for (int s = 0; s < S; ++s) {
    const uint8_t tk = dc->take[s];
    if (tk > 1) return GMX_ERR_INVALID;
    if (!tk) {
      if (cs->pending[s]) return GMX_ERR_STATE;  // (its record would be two copies old: as in gmx_chainstep_launch)
      continue;
    }
    any = true;
    if (!dc->has_input[s]) return GMX_ERR_STATE;
    if (cs->nbits[s] != (cs->pending[s] ? 7 : 0) || cs->c_pos[s] != 0) return GMX_ERR_STATE;  // not at a byte boundary
    if (cs->pending[s]) {
      if (dc->via_byte[s]) {
        first_bit[s] = dc->decoded[s] & 1u;
      } else {
        if (cs->bits[s] > 1) return GMX_ERR_INVALID;
        first_bit[s] = cs->bits[s];
      }
    }
  }
  if (!any) return GMX_OK;  // (nothing queued: the wait returns at once)
  if (cs->mb) {
    std::vector<uint64_t> add(S, 0);
    for (int s = 0; s < S; ++s) add[s] = (dc->take[s] && cs->pending[s] && cs->m_bc[s] >= 127u) ? 1 : 0;
    int rc = match_reserve(cs->mb, 0, S, add.data());
    if (rc) return rc;
    if (hipStreamQuery(cs->mb->stream) != hipSuccess) HIPCHK(hipStreamSynchronize(cs->mb->stream));
    (void)hipGetLastError();
  }
  {  // nobody else holds rows or table entries in registers, nothing of the banks' own is still in flight
    int rc = sessions_close(g, false);
    if (rc) return rc;
    if (cs->ib) {
      rc = ind_sessions_close(cs->ib);
      if (rc) return rc;
      if (hipStreamQuery(cs->ib->stream) != hipSuccess) HIPCHK(hipStreamSynchronize(cs->ib->stream));
    }
    if (cs->l) {
      rc = lstm_sessions_close(cs->l);
      if (rc) return rc;
      if (hipStreamQuery(cs->l->stream) != hipSuccess) HIPCHK(hipStreamSynchronize(cs->l->stream));
    }
    (void)hipGetLastError();
  }
  // the bookkeeping of gmx_chainstep_launch for the byte's eight steps
  std::unordered_map<uint64_t, float> decay;  // one libm call per distinct learn count
  auto dec_of = [&decay](uint64_t at) {
    auto it = decay.find(at);
    if (it != decay.end()) return it->second;
    const float v = decay_base(at);
    decay.emplace(at, v);
    return v;
  };
  for (int s = 0; s < S; ++s) {
    GmxCoderByteIn& in = dc->h_in[s];
    memset(&in, 0, sizeof in);
    in.seq0 = cs->seq_no;
    cs->nl_perceive[s] = 0;
    cs->nl_forward[s] = 0;
    dc->taking[s] = dc->take[s];
    if (!dc->take[s]) continue;
    const bool learn = cs->pending[s] != 0;
    uint64_t k = g->steps[s];
    in.take = 1;
    in.b_first = first_bit[s];
    in.w_first = (uint8_t)((learn ? GMX_STEP_LEARN : 0) | GMX_STEP_PREDICT | 4u);
    if (learn) {
      in.dec[0] = dec_of(k++);
      // the byte that Learn completes: LstmModel::Learn perceives it (lstm-model.cpp:51-60)
      cs->bytes[s] = (uint8_t)((cs->acc[s] << 1) | first_bit[s]);
      cs->nl_perceive[s] = 1;
    }
    for (int j = 1; j < 8; ++j) in.dec[j] = dec_of(k++);
    cs->nl_forward[s] = 1;
    if (cs->mb) {
      if (!cs->m_seen[s]) in.w_first |= 8u;
      cs->m_seen[s] = 1;
      cs->m_bc[s] = 127u;  // the outstanding Predict is of the byte's last bit
    }
    g->steps[s] = k;
    cs->pending[s] = 1;
    cs->nbits[s] = 7;  // (acc: when the byte is known, cs_decoder_answered)
    cs->acc[s] = 0;
    dc->via_byte[s] = 1;
    cs->cb->outstanding[s] = 1;
    g->fwd_done[s] = 0;
    if (cs->ib) cs->ib->fwd_done[s] = 0;
    if (cs->mb) cs->mb->fwd_done[s] = 0;
    if (cs->l) {
      cs->l->fwd_done[s] = 0;
      cs->l->range_read[s].valid = false;
    }
  }
  cs->seq_no += 8;
  if (cs->l) {
    lstm_stage_rows(cs->l, 0, S, 1, 1, 4u, cs->nl_perceive, cs->adam_host, 2);
    lstm_stage_rows(cs->l, 0, S, 1, 0, 1u, cs->nl_forward, cs->adam_host, 2);
  }
  if (cs->bar) {
    memcpy(dc->in_bar, dc->h_in, (size_t)S * sizeof(GmxCoderByteIn));
    for (int s = 0; s < S; ++s)
      if (dc->take[s]) {
        const size_t at = cs->bd_ppm_off + (size_t)s * GMX_L_NI * 4;
        memcpy(cs->d_bd + at, cs->h_bd + at, GMX_L_NI * 4);
      }
    if (cs->l) {
      const size_t at = (const uint8_t*)cs->bytes - cs->h_bd;  // bytes | nl_perceive | nl_forward
      memcpy(cs->d_bd + at, cs->h_bd + at, cs->bd_bytes - at);
    }
    mb_store_fence();
  }
  if (cs->timed) HIPCHK(hipEventRecord(cs->t_ev[0], g->stream));
  HIPCHK(hipGraphLaunch(dc->exec[cs->steps & 1], g->stream));
  if (cs->timed) {
    HIPCHK(hipEventRecord(cs->t_ev[1], g->stream));
    cs->timed_ok = true;
  }
  cs->in_flight = true;
  dc->in_flight = true;
  for (gmx_lockstep* o : g->locksteps) o->predicted = false;
  cs->steps += 8;
  return GMX_OK;
}

extern "C" int gmx_chainstep_byte_wait(gmx_chainstep* cs) { return gmx_chainstep_wait(cs); }

extern "C" int gmx_chainstep_byte(gmx_chainstep* cs) {
  const int rc = gmx_chainstep_byte_launch(cs);
  return rc ? rc : gmx_chainstep_wait(cs);
}

extern "C" int gmx_chainstep_timed_byte(gmx_chainstep* cs, float* device_ms) {
  if (!cs || !cs->g || !device_ms) return GMX_ERR_INVALID;
  *device_ms = 0.0f;
  HIPCHK(hipSetDevice(cs->g->device));
  for (hipEvent_t& ev : cs->t_ev)
    if (!ev) HIPCHK(hipEventCreate(&ev));
  cs->timed = true;
  cs->timed_ok = false;
  int rc = gmx_chainstep_byte_launch(cs);
  cs->timed = false;
  if (!rc) rc = gmx_chainstep_wait(cs);
  if (rc || !cs->timed_ok) return rc;
  HIPCHK(hipEventSynchronize(cs->t_ev[1]));
  HIPCHK(hipEventElapsedTime(device_ms, cs->t_ev[0], cs->t_ev[1]));
  return GMX_OK;
}
