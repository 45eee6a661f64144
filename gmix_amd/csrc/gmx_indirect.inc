// gmx_indirect.inc -- host side of the Indirect-model banks (included by gmx_capi.cpp).
//
// Replaces the reference's 41 `Indirect` objects (models/indirect.{h,cpp}, constructed in
// predictor.cpp:78-120, :122-185, :210-250) and their IndirectMemory (long-term-memory.h:11-25)
// for S independent streams.  Compute is gmx_indirect.hip; nothing here falls back to the CPU.

struct gmx_ind_batch : GmxBatchCore {
  gmx_indirect* ib = nullptr;
  uint64_t& max_bits = max_rows;
  uint32_t* d_ctx = nullptr;
  uint32_t* d_bc = nullptr;
  uint8_t* d_bits = nullptr;
  float* d_pred = nullptr;
  uint8_t* d_act = nullptr;
  uint64_t* d_rng = nullptr;     // synthetic generator state: xorshift64, recent_bits, contexts
  uint32_t* d_recent = nullptr;
  uint32_t* d_cstate = nullptr;
  uint32_t* h_ctx = nullptr;
  uint32_t* h_bc = nullptr;
  uint8_t* h_bits = nullptr;
  float* h_pred = nullptr;
  uint8_t* h_act = nullptr;
};

struct gmx_indirect {
  int device = 0, S = 0;
  GmxIndDev dev;                 // host copy
  GmxIndDev* dev_d = nullptr;
  uint8_t* banks = nullptr;
  uint64_t tab_bytes = 0;        // leading part of a bank: the u16 tables
  unsigned lds_bytes = 0;
  hipStream_t stream = nullptr;
  hipStream_t up_stream = nullptr, down_stream = nullptr;  // record batches beside the kernels
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<uint32_t> table_size;
  GmxBatchBank bb;               // its record batches
  gmx_ind_batch* one = nullptr;  // 1-bit batch of the per-bit surface
  std::vector<uint8_t> fwd_done;
  GmxCountList counts;                          // per-stream bit counts of ragged launches
  std::vector<struct GmxIndSession*> sessions;  // per-bit sessions (gmx_indirect_session_kernel), per stream
  bool use_sessions = true;
  bool banks_in_use_by_dead_kernel = false;  // a session wave that stopped answering may still hold them: never freed
  struct GmxIndCkptState* ckpt = nullptr;  // gmx_indirect_group_export / _import: chunk list and staging (gmx_ind_ckpt.inc), lazily
  // gmx_indirect_attach_match: the streams of this Match bank ride in lanes 56..63 of the session waves.  What a
  // wave needs of the bank is copied here at the attach (gmx_match.inc comes later in the translation unit); the two
  // objects register with each other, and whichever is destroyed first detaches (match_host_detach).
  gmx_match* match = nullptr;
  const GmxMatchDev* match_dev_d = nullptr;
  uint8_t* match_banks = nullptr;
  uint8_t* match_hist = nullptr;
  uint64_t match_bank_bytes = 0, match_hist_cap = 0;
  int match_k = 0, match_n_cols = 0;
  int32_t match_slot[GMX_MATCH_MAX_MODELS] = {};
  int32_t match_cols[GMX_MATCH_MAX_CTX_COLS] = {};
  // gmx_indirect_attach_ctx: the streams of this context bank step at the head of a chained forward in the same
  // waves.  As for the Match bank, what a wave needs is copied here at the attach (gmx_ctx.inc comes later), the two
  // objects register with each other, and whichever is destroyed first detaches (ctx_host_detach).
  gmx_ctx* ctx = nullptr;
  const GmxCtxDev* ctx_dev_d = nullptr;
  uint8_t* ctx_banks = nullptr;
  uint64_t ctx_bank_bytes = 0;
  const int32_t* ctx_routes_d = nullptr;  // [GMX_CTX_WAVE_ROUTE_WORDS]
  int ctx_v = 0, ctx_n_mixer_cols = 0;
};
static void ind_ckpt_free(gmx_indirect* ib);
static int match_host_detach(gmx_match* mb);  // gmx_match.inc
static int ctx_host_detach(gmx_ctx* cb);      // gmx_ctx.inc
static_assert(sizeof(((GmxIndMbCmd*)nullptr)->match_ctx[0]) == GMX_MATCH_MAX_MODELS * 4 &&
                  sizeof(((GmxIndMbReply*)nullptr)->match_pred) == GMX_MATCH_MAX_MODELS * 4,
              "the Match fields of the Indirect mailbox hold one lane group");

static const uint32_t kMatchStepLearn = 1u, kMatchStepPredict = 2u, kMatchStepTakeCtx = 8u;  // GMX_MATCH_STEP_*
// What the Match lanes do in a chained forward, and what they answer (ind_session_forward).
struct GmxIndMatchCmd {
  const uint32_t* ctx;     // [K_match]
  uint32_t what;           // GMX_MATCH_STEP_* | coded bit << GMX_IND_MB_MATCH_BIT_SHIFT
  float* predictions;      // [K_match], nullable
  uint8_t* active;         // [K_match], nullable
  uint32_t* longest_match; // nullable
};
// What the context variables do at the head of a chained forward, and what they answer.
struct GmxIndCtxCmd {
  uint32_t what;           // the command's ctx_what word (gmx_ctx.h)
  uint32_t* values;        // [V], nullable
  uint32_t* bit_context;   // nullable
};

// ---- per-bit sessions: gmx_indirect_forward / gmx_indirect_learn without a kernel launch per call -----
// The protocol and its bounded waits are gmx_mailbox.h, the blocks and the stream of a session GmxSessionHw
// (gmx_session.inc), as for the mixers: the learn is only noted and travels with the next forward as one command;
// every other entry point that touches the bank first stops the session, which writes the logit tables back.
struct GmxIndSession : GmxSessionHw {
  GmxIndMbCmd* mc = nullptr;
  GmxIndMbReply* mb = nullptr;
  uint32_t slot = 0, live_slot = 0;  // payload slot of the newest forward published / completed
  int pending_learn = 0;       // 1 + bit: noted by gmx_indirect_learn, not yet published
  bool fwd_live = false, learn_inflight = false;
  uint32_t ctx_what[2] = {0, 0};  // host copy of the command block's ctx_what words (the block may be device memory)
};
static int ind_sessions_close(gmx_indirect* ib);
static void ind_sessions_free(gmx_indirect* ib);
// The bank's content is about to change under a (stopped) session -- a copy into it, a batched run, a reset, an
// import: a forward it still held for its learn is void, and must not be recomputed on the new tables when the
// session comes back (stream < 0: every stream).
static void ind_sessions_drop_forward(gmx_indirect* ib, int stream);

struct GmxIndSynthArgs {
  uint32_t* ctx;
  uint32_t* bc;
  uint8_t* bits;
  uint64_t* rng;
  uint32_t* recent;
  uint32_t* cstate;
  uint64_t rec_stride, n_bits, seed;
  int32_t k, n_streams, restart;
  uint32_t ctx_mod[4];
};

extern "C" {
hipError_t gmx_launch_indirect_kernel(const GmxIndDev* dv, const GmxIndRunArgs* args, int n_streams,
                                      unsigned lds_bytes, hipStream_t stream);
hipError_t gmx_launch_indirect_init(uint8_t* banks, uint64_t bank_bytes, uint64_t tab_bytes, int n_streams,
                                    hipStream_t stream);
hipError_t gmx_launch_ind_synth_kernel(const GmxIndSynthArgs* args, hipStream_t stream);
hipError_t gmx_launch_indirect_session(const GmxIndDev* dv, uint8_t* banks, int stream_idx, GmxIndMbCmd* mc,
                                       GmxIndMbReply* mr, unsigned long long idle_ticks, int replay_forward,
                                       unsigned lds_bytes, hipStream_t stream);
hipError_t gmx_launch_indirect_session_match(const GmxIndDev* dv, int k_ind, uint8_t* banks, int stream_idx,
                                             GmxIndMbCmd* mc, GmxIndMbReply* mr, unsigned long long idle_ticks,
                                             int replay_forward, const GmxMatchDev* mdv, const GmxMatchStepArgs* margs,
                                             unsigned lds_bytes, hipStream_t stream);
hipError_t gmx_launch_indirect_session_ctx(const GmxIndDev* dv, int k_ind, uint8_t* banks, int stream_idx,
                                           GmxIndMbCmd* mc, GmxIndMbReply* mr, unsigned long long idle_ticks,
                                           int replay_forward, const GmxMatchDev* mdv, const GmxMatchStepArgs* margs,
                                           const GmxCtxWaveArgs* cargs, unsigned lds_bytes, hipStream_t stream);
}

static void ind_batch_free(gmx_ind_batch* b) {
  if (!b) return;
  batch_core_free(*b);
  delete b;
}

extern "C" void gmx_indirect_destroy(gmx_indirect* ib) {
  if (!ib) return;
  (void)hipSetDevice(ib->device);
  if (ib->ctx) (void)ctx_host_detach(ib->ctx);        // (stops the sessions; a noted learn takes the launch path)
  if (ib->match) (void)match_host_detach(ib->match);  // (stops the sessions; a noted Match learn takes the launch path)
  ind_sessions_free(ib);
  if (ib->stream) (void)hipStreamSynchronize(ib->stream);
  if (ib->one) {
    ind_batch_free(ib->one);
    ib->one = nullptr;
  }
  ind_ckpt_free(ib);
  batch_bank_detach_all(ib->bb);  // shells, as for gmx_batch
  if (!ib->banks_in_use_by_dead_kernel) {  // (as gmx_group_destroy: leaked rather than freed under a running kernel)
    if (ib->banks) (void)hipFree(ib->banks);
    if (ib->dev_d) (void)hipFree(ib->dev_d);
  }
  if (ib->ev0) (void)hipEventDestroy(ib->ev0);
  if (ib->ev1) (void)hipEventDestroy(ib->ev1);
  hipStream_t xs[] = {ib->up_stream, ib->down_stream};
  for (hipStream_t x : xs)
    if (x) {
      (void)hipStreamSynchronize(x);
      (void)hipStreamDestroy(x);
    }
  count_list_free(ib->counts);
  if (ib->stream) (void)hipStreamDestroy(ib->stream);
  delete ib;
}

extern "C" int gmx_indirect_reset(gmx_indirect* ib) {
  if (!ib) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(ib->device));
  {
    int rcs = ind_sessions_close(ib);
    if (rcs) return rcs;
  }
  HIPCHK(gmx_launch_indirect_init(ib->banks, ib->dev.bank_bytes, ib->tab_bytes, ib->S, ib->stream));
  HIPCHK(hipStreamSynchronize(ib->stream));
  std::fill(ib->fwd_done.begin(), ib->fwd_done.end(), 0);
  ind_sessions_drop_forward(ib, -1);
  return GMX_OK;
}

extern "C" int gmx_indirect_create(gmx_indirect** out, const gmx_indirect_desc* models, int n_models,
                                   const uint8_t* nonstationary_next, const uint8_t* run_map_next,
                                   int n_streams, int device) {
  if (!out) return GMX_ERR_INVALID;
  *out = nullptr;
  if (!models || n_models < 1 || n_models > GMX_IND_MAX_MODELS || !nonstationary_next || !run_map_next ||
      n_streams < 1)
    return GMX_ERR_INVALID;
  GmxIndDev d;
  memset(&d, 0, sizeof d);
  d.k = n_models;
  uint64_t off = 0;
  std::vector<char> used(2048, 0);
  for (int i = 0; i < n_models; ++i) {
    const gmx_indirect_desc& m = models[i];
    // the reference supports contexts up to 24 bits (indirect.h:11-13): 256*table_size+1 fits 32 bits
    if (m.table_size == 0 || m.table_size > (1u << 24) - 1) return GMX_ERR_INVALID;
    if (m.slot_indirect < 0 || m.slot_indirect >= 2048 || m.slot_run_map < 0 || m.slot_run_map >= 2048 ||
        m.slot_indirect == m.slot_run_map || used[m.slot_indirect] || used[m.slot_run_map])
      return GMX_ERR_INVALID;
    used[m.slot_indirect] = used[m.slot_run_map] = 1;
    d.m[i].size = m.table_size * 256u + 1u;
    d.m[i].lr = m.learning_rate;
    d.m[i].slot_a = m.slot_indirect;
    d.m[i].slot_b = m.slot_run_map;
    d.m[i].tab_off = off;
    off += round_up64(2ull * d.m[i].size, 256);
    d.n_slots = std::max(d.n_slots, std::max(m.slot_indirect, m.slot_run_map) + 1);
  }
  const uint64_t tab_bytes = off;
  d.pred_off = off;
  off += (uint64_t)n_models * 512 * sizeof(float);
  d.slots_off = off;
  off += round_up64((uint64_t)n_models * 2 * sizeof(float), 256);
  d.bank_bytes = off;
  for (int s = 0; s < 512; ++s) {
    d.ns_next[s] = nonstationary_next[s];
    d.rm_next[s] = run_map_next[s];
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return GMX_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(device));
  gmx_indirect* ib = new (std::nothrow) gmx_indirect();
  if (!ib) return GMX_ERR_NOMEM;
  ib->device = device;
  batch_bank_init(ib->bb, ib, device, &ib->stream, &ib->up_stream, &ib->down_stream);
  ib->S = n_streams;
  ib->dev = d;
  ib->tab_bytes = tab_bytes;
  ib->fwd_done.assign(n_streams, 0);
  for (int i = 0; i < n_models; ++i) ib->table_size.push_back(models[i].table_size);
  // LDS: k x 512 logits, expf table, two next-state tables, mask words
  ib->lds_bytes = (unsigned)(n_models * 2048 + 256 + 1024 + 64);
#define ICHK(call)                                 \
  do {                                             \
    hipError_t e_ = (call);                        \
    if (e_ != hipSuccess) {                        \
      int r_ = hip_fail(e_, #call);                \
      gmx_indirect_destroy(ib);                    \
      return e_ == hipErrorOutOfMemory ? GMX_ERR_NOMEM : r_; \
    }                                              \
  } while (0)
  ICHK(bank_stream_create(&ib->stream, 1));
  ICHK(hipEventCreate(&ib->ev0));
  ICHK(hipEventCreate(&ib->ev1));
  ICHK(hipMalloc((void**)&ib->dev_d, sizeof(GmxIndDev)));
  ICHK(hipMemcpy(ib->dev_d, &ib->dev, sizeof(GmxIndDev), hipMemcpyHostToDevice));
  ICHK(hipMalloc((void**)&ib->banks, (size_t)n_streams * d.bank_bytes));
#undef ICHK
  int rc = gmx_indirect_reset(ib);
  if (rc) {
    gmx_indirect_destroy(ib);
    return rc;
  }
  *out = ib;
  return GMX_OK;
}

extern "C" int gmx_indirect_n_streams(const gmx_indirect* ib) { return ib ? ib->S : GMX_ERR_INVALID; }
extern "C" int gmx_indirect_n_models(const gmx_indirect* ib) { return ib ? ib->dev.k : GMX_ERR_INVALID; }
extern "C" uint64_t gmx_indirect_bank_bytes(const gmx_indirect* ib) { return ib ? ib->dev.bank_bytes : 0; }
extern "C" int gmx_indirect_sync(gmx_indirect* ib) {
  if (!ib) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(ib->device));
  {
    int rcs = ind_sessions_close(ib);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(ib->stream));
  return GMX_OK;
}

// ---- record batches ------------------------------------------------------------------------
static int ind_batch_alloc(gmx_ind_batch** out, gmx_indirect* ib, uint64_t max_bits) {
  if (!out || !ib || max_bits == 0) return GMX_ERR_INVALID;
  *out = nullptr;
  gmx_ind_batch* b = new (std::nothrow) gmx_ind_batch();
  if (!b) return GMX_ERR_NOMEM;
  b->back = (void**)&b->ib;
  gmx_ind_batch_cols(b->cols, b, ib->dev.k);
  int rc = batch_core_alloc(*b, &ib->bb, ib->S, max_bits, false);
  if (rc) {
    ind_batch_free(b);
    return rc;
  }
  *out = b;
  return GMX_OK;
}

extern "C" int gmx_ind_batch_create(gmx_ind_batch** out, gmx_indirect* ib, uint64_t max_bits) {
  int rc = ind_batch_alloc(out, ib, max_bits);
  if (rc) return rc;
  return xfer_streams_ready(ib->stream, &ib->up_stream, &ib->down_stream);
}
extern "C" void gmx_ind_batch_destroy(gmx_ind_batch* b) { ind_batch_free(b); }
extern "C" uint64_t gmx_ind_batch_max_bits(const gmx_ind_batch* b) { return b ? b->max_bits : 0; }

extern "C" uint32_t* gmx_ind_batch_contexts(gmx_ind_batch* b) {
  return b ? (uint32_t*)batch_core_host(*b, &b->h_ctx) : nullptr;
}
extern "C" uint32_t* gmx_ind_batch_bit_contexts(gmx_ind_batch* b) {
  return b ? (uint32_t*)batch_core_host(*b, &b->h_bc) : nullptr;
}
extern "C" uint8_t* gmx_ind_batch_bits(gmx_ind_batch* b) { return b ? (uint8_t*)batch_core_host(*b, &b->h_bits) : nullptr; }
extern "C" const float* gmx_ind_batch_predictions(gmx_ind_batch* b) {
  return b ? (float*)batch_core_host(*b, &b->h_pred) : nullptr;
}
extern "C" const uint8_t* gmx_ind_batch_active(gmx_ind_batch* b) {
  return b ? (uint8_t*)batch_core_host(*b, &b->h_act) : nullptr;
}

// beside the kernels, on streams of their own (see gmx_batch_upload)
extern "C" int gmx_ind_batch_upload(gmx_ind_batch* b, uint64_t n_bits) { return batch_core_transfer(b, n_bits, GMX_COL_UP); }
extern "C" int gmx_ind_batch_download(gmx_ind_batch* b, uint64_t n_bits) {
  return batch_core_transfer(b, n_bits, GMX_COL_DOWN);
}
extern "C" int gmx_ind_batch_wait(gmx_ind_batch* b) { return batch_core_wait(b); }  // this batch's upload, runs and download

extern "C" int gmx_ind_batch_fill_synthetic(gmx_ind_batch* b, uint64_t n_bits, uint64_t seed, uint64_t restart,
                                            const uint32_t* ctx_mod) {
  if (!b || !b->ib || n_bits > b->max_bits || !ctx_mod) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(b->ib->device));
  if (!b->d_rng) {
    if (!restart) return GMX_ERR_STATE;
    HIPCHK(hipMalloc((void**)&b->d_rng, (size_t)b->S * 8));
    HIPCHK(hipMalloc((void**)&b->d_recent, (size_t)b->S * 4));
    HIPCHK(hipMalloc((void**)&b->d_cstate, (size_t)b->S * b->ib->dev.k * 4));
  }
  GmxIndSynthArgs a;
  a.ctx = b->d_ctx;
  a.bc = b->d_bc;
  a.bits = b->d_bits;
  a.rng = b->d_rng;
  a.recent = b->d_recent;
  a.cstate = b->d_cstate;
  a.rec_stride = b->max_bits;
  a.n_bits = n_bits;
  a.seed = seed;
  a.k = b->ib->dev.k;
  a.n_streams = b->S;
  a.restart = restart ? 1 : 0;
  for (int i = 0; i < 4; ++i) a.ctx_mod[i] = ctx_mod[i];
  HIPCHK(gmx_launch_ind_synth_kernel(&a, b->ib->stream));
  return xfer_note_device_use(b->x, b->ib->stream);
}

// ---- compute -------------------------------------------------------------------------------
static int ind_launch(gmx_indirect* ib, gmx_ind_batch* b, int s0, int rec0, int ns, uint64_t T, int learn,
                      gmx_batch* into, float* kernel_ms, const uint64_t* n_list = nullptr) {
  // n_list (host, [ns]): bits of each stream of the range, at most T (one launch for streams of different lengths)
  if (T == 0) return GMX_OK;
  GmxIndRunArgs a;
  memset(&a, 0, sizeof a);
  a.banks = ib->banks;
  a.ctx = b->d_ctx;
  a.bc = b->d_bc;
  a.bits = b->d_bits;
  a.pred_out = b->d_pred;
  a.act_out = b->d_act;
  a.rec_stride = b->max_bits;
  a.T = T;
  if (n_list) {
    int rcl = count_list_stage(ib->counts, n_list, ns, ib->stream, &a.T_list);
    if (rcl) return rcl;
  }
  a.learn = learn ? 1u : 0u;
  a.stream_base = s0;
  a.rec_base = rec0;
  if (into) {
    a.mx_pred = into->d_pred;
    a.mx_mask = into->d_mask;
    a.mx_bits = into->d_bits;
    a.mx_rec_stride = into->max_bits;
    a.mx_n_pad = into->g->topo.n_pad;
    a.mx_mask_words = into->g->topo.mask_words;
    // the mixer batch's own uploads (other models' predictions, contexts) and whoever wrote it last come first ...
    int rcw = xfer_writer_waits(into->x, ib->stream);
    if (rcw) return rcw;
  }
  {
    int rcx = xfer_before_run(b->x, ib->stream);  // the results of the previous run are out
    if (rcx) return rcx;
  }
  if (kernel_ms) HIPCHK(hipEventRecord(ib->ev0, ib->stream));
  HIPCHK(gmx_launch_indirect_kernel(ib->dev_d, &a, ns, ib->lds_bytes, ib->stream));
  if (n_list) {
    int rcl = count_list_used(ib->counts, ib->stream);
    if (rcl) return rcl;
  }
  {
    int rcx = xfer_note_device_use(b->x, ib->stream);
    if (rcx) return rcx;
  }
  if (kernel_ms) {
    HIPCHK(hipEventRecord(ib->ev1, ib->stream));
    HIPCHK(hipEventSynchronize(ib->ev1));
    HIPCHK(hipEventElapsedTime(kernel_ms, ib->ev0, ib->ev1));
  }
  if (into) {
    // ... and the mixers run after the models have written their part of the records
    int rcn = xfer_writer_done(into->x, ib->stream, into->g->stream);
    if (rcn) return rcn;
  }
  return GMX_OK;
}

extern "C" int gmx_indirect_run(gmx_indirect* ib, gmx_ind_batch* b, uint64_t n_bits, int learn, gmx_batch* into,
                                float* kernel_ms) {
  if (!ib || !b || b->ib != ib || n_bits > b->max_bits) return GMX_ERR_INVALID;
  if (into) {
    if (!into->g || into->S != ib->S || into->g->device != ib->device || n_bits > into->max_bits || !into->d_mask ||
        ib->dev.n_slots > into->g->topo.n)
      return GMX_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(ib->device));
  {
    int rcs = ind_sessions_close(ib);
    if (rcs) return rcs;
  }
  std::fill(ib->fwd_done.begin(), ib->fwd_done.end(), 0);
  ind_sessions_drop_forward(ib, -1);
  return ind_launch(ib, b, 0, 0, ib->S, n_bits, learn, into, kernel_ms);
}

// The same for streams that stand at different lengths, in one launch (the kernel takes a count per block); a stream
// with 0 bits sits out.
extern "C" int gmx_indirect_run_ragged(gmx_indirect* ib, gmx_ind_batch* b, const uint64_t* n_bits, int learn,
                                       gmx_batch* into) {
  if (!ib || !b || b->ib != ib || !n_bits) return GMX_ERR_INVALID;
  for (int s = 0; s < ib->S; ++s)
    if (n_bits[s] > b->max_bits || (into && n_bits[s] > into->max_bits)) return GMX_ERR_INVALID;
  if (into) {
    if (!into->g || into->S != ib->S || into->g->device != ib->device || !into->d_mask ||
        ib->dev.n_slots > into->g->topo.n)
      return GMX_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(ib->device));
  {
    int rcs = ind_sessions_close(ib);
    if (rcs) return rcs;
  }
  std::fill(ib->fwd_done.begin(), ib->fwd_done.end(), 0);
  ind_sessions_drop_forward(ib, -1);
  uint64_t maxn = 0;
  bool same = true;
  for (int s = 0; s < ib->S; ++s) {
    maxn = std::max(maxn, n_bits[s]);
    same = same && n_bits[s] == n_bits[0];
  }
  return ind_launch(ib, b, 0, 0, ib->S, maxn, learn, into, nullptr, same ? nullptr : n_bits);
}

// ---- per-bit sessions (see GmxIndSession above) ------------------------------------------------
static void ind_session_note_done(GmxIndSession* se) {
  if (se->learn_inflight && mb_load(se->done_seq) == se->word) {
    se->learn_inflight = false;
    se->fwd_live = false;
  }
}

static int ind_session_start(gmx_indirect* ib, int s) {
  GmxIndSession* se = ib->sessions[s];
  int rc = session_hw_start_prologue(se);
  if (rc) return rc;
  ind_session_note_done(se);
  const int replay = se->fwd_live ? 1 + (int)se->live_slot : 0;
  GmxMatchStepArgs ma;
  memset(&ma, 0, sizeof ma);
  if (ib->match) {  // the stream's Match models in lanes 56..63: the wave steps them as "stream 0" of these arguments
    ma.banks = ib->match_banks + (uint64_t)s * ib->match_bank_bytes;
    ma.hist = ib->match_hist + (uint64_t)s * ib->match_hist_cap;
    ma.n_ctx_cols = ib->match_n_cols;
    for (int c = 0; c < ib->match_n_cols; ++c) ma.ctx_cols[c] = ib->match_cols[c];
    ma.n_streams = 1;
  }
  if (ib->ctx) {  // the stream's context variables at the head of a chained forward (a fresh wave reads the board itself)
    GmxCtxWaveArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.dev = ib->ctx_dev_d;
    ca.bank = ib->ctx_banks + (uint64_t)s * ib->ctx_bank_bytes;
    ca.routes = ib->ctx_routes_d;
    ca.n_mixer_cols = ib->ctx_n_mixer_cols;
    HIPCHK(gmx_launch_indirect_session_ctx(ib->dev_d, ib->dev.k, ib->banks, s, se->mc, se->mb, kIdleTicks, replay,
                                           ib->match ? ib->match_dev_d : nullptr, ib->match ? &ma : nullptr, &ca,
                                           ib->lds_bytes + 4u * GMX_CTX_MAX_VARS, se->stream));
    return GMX_OK;
  }
  if (ib->match) {
    HIPCHK(gmx_launch_indirect_session_match(ib->dev_d, ib->dev.k, ib->banks, s, se->mc, se->mb, kIdleTicks, replay,
                                             ib->match_dev_d, &ma, ib->lds_bytes, se->stream));
    return GMX_OK;
  }
  HIPCHK(gmx_launch_indirect_session(ib->dev_d, ib->banks, s, se->mc, se->mb, kIdleTicks, replay, ib->lds_bytes,
                                     se->stream));
  return GMX_OK;
}

static int ind_session_dead(GmxIndSession* se) {
  g_last_error = "per-bit Indirect session does not answer";
  se->pending_learn = 0;
  se->fwd_live = false;
  return GMX_ERR_HIP;
}

// Wait until the newest command has been completed, restarting the session if it left first (bounded).
static int ind_session_wait(gmx_indirect* ib, int s) {
  GmxIndSession* se = ib->sessions[s];
  int rc = mb_wait(se, kSessionTimeoutS, [&] { return ind_session_start(ib, s); });
  if (rc) return rc == kMbDead ? ind_session_dead(se) : rc;
  ind_session_note_done(se);
  return GMX_OK;
}

// Make sure session s exists and runs.  GMX_ERR_STATE: no session slot is free (the caller uses the
// launch-per-call path); `force` starts one beyond the limit (a noted learn has no other way).
static int ind_session_ensure(gmx_indirect* ib, int s, bool force) {
  if (ib->sessions.empty()) ib->sessions.assign(ib->S, nullptr);
  GmxIndSession* se = ib->sessions[s];
  if (se && se->dead) return ind_session_dead(se);
  const bool running = se && se->launched && mb_load(se->state) == GMX_MB_RUNNING;
  if (!running && !(se && se->launched) && g_open_sessions.load() >= kMaxOpenSessions && !force) return GMX_ERR_STATE;
  if (!se) {
    se = new (std::nothrow) GmxIndSession();
    if (!se) return GMX_ERR_NOMEM;
    ib->sessions[s] = se;
    int rc = session_hw_alloc(se, sizeof(GmxIndMbCmd), sizeof(GmxIndMbReply), true, ib->device);
    se->mc = (GmxIndMbCmd*)se->cmd_seq;
    se->mb = (GmxIndMbReply*)se->done_seq;
    if (rc) return rc;
  }
  if (!running) {
    HIPCHK(hipStreamSynchronize(ib->stream));  // batched work on the bank is finished
    return ind_session_start(ib, s);
  }
  return GMX_OK;
}

// A learn that gmx_indirect_learn noted and no forward has taken along yet: send it on its own.
static int ind_session_flush_learn(gmx_indirect* ib, int s) {
  GmxIndSession* se = s < (int)ib->sessions.size() ? ib->sessions[s] : nullptr;
  if (!se || !se->pending_learn) return GMX_OK;
  int rc = ind_session_ensure(ib, s, true);  // restarts (with a replay of the forward) a session that left
  if (rc) return rc;
  const int bit = se->pending_learn - 1;
  se->pending_learn = 0;
  se->learn_inflight = true;
  mb_publish(se, se->slot, bit ? GMX_MB_LEARN1 : GMX_MB_LEARN0);
  return GMX_OK;
}

static int ind_session_stop(gmx_indirect* ib, int s) {
  GmxIndSession* se = s < (int)ib->sessions.size() ? ib->sessions[s] : nullptr;
  if (!se) return GMX_OK;
  if (se->dead) return ind_session_dead(se);
  int rc = ind_session_flush_learn(ib, s);
  if (rc) return rc;
  return session_hw_stop(se, [&] { return ind_session_wait(ib, s); });
}

// The board of the context bank that rides here is about to be moved for stream s by something that is not a command
// of the stream's wave (a launch of the per-bit surface, a run, a board written, a copy, a reset).  A forward that took
// its table indices from the board and still waits for its learn would be recomputed from the MOVED board by a wave
// restarted in between (gmx_ctx_step_wave_replay), and its learn would land on other entries.  So a noted learn is run
// now -- the wave, restarted if it has left, replays from the board as it still stands -- and without one the forward
// is void from here on, as after a change of the Indirect bank's own content (ind_sessions_drop_forward): it is what a
// perceived bit leaves behind (generation: no learn ever comes), and a gmx_indirect_learn that does come for it
// returns GMX_ERR_STATE with no table touched.  s < 0: every stream.
static int ind_ctx_board_moves(gmx_indirect* ib, int s) {
  for (int i = 0; i < (int)ib->sessions.size(); ++i) {
    GmxIndSession* se = ib->sessions[i];
    if (!se || se->dead || (s >= 0 && i != s)) continue;
    ind_session_note_done(se);
    if (!se->fwd_live || !(se->ctx_what[se->live_slot] & GMX_STEP_PREDICT)) continue;
    if (se->pending_learn) {
      int rc = ind_session_flush_learn(ib, i);
      if (rc) return rc;
    }
    if (se->learn_inflight) {
      int rc = ind_session_wait(ib, i);
      if (rc) return rc;
    }
    se->fwd_live = false;  // (no learn was noted for it)
  }
  return GMX_OK;
}

static void ind_sessions_drop_forward(gmx_indirect* ib, int stream) {
  for (size_t s = 0; s < ib->sessions.size(); ++s) {
    GmxIndSession* se = ib->sessions[s];
    if (!se || (stream >= 0 && (int)s != stream)) continue;
    se->fwd_live = false;
    se->pending_learn = 0;
  }
}

static int ind_sessions_close(gmx_indirect* ib) {
  return sessions_stop_each(ib->sessions.size(), [&](int s) { return ind_session_stop(ib, s); });
}

static void ind_sessions_free(gmx_indirect* ib) {
  (void)ind_sessions_close(ib);
  // (a wave that is still there writes the bank's tables: gmx_indirect_destroy leaks them)
  if (!sessions_release_each(ib->sessions)) ib->banks_in_use_by_dead_kernel = true;
}

// `chain`: after its Predict the wave hands the predictions to the mixers' session whose command block is
// chain_mc (payload slot chain_slot) and rings it with chain_word (GmxIndMbCmd); 0 = an ordinary forward.
static int ind_session_forward(gmx_indirect* ib, int s, const uint32_t* contexts, uint32_t bit_context,
                               float* predictions, uint8_t* active, uint32_t chain_word = 0,
                               uint32_t chain_slot = 0, void* chain_mc = nullptr,
                               const GmxIndMatchCmd* match = nullptr, const GmxIndCtxCmd* ctx = nullptr) {
  {
    // a noted learn rides along only if the wave that made its forward is still there
    GmxIndSession* se0 = s < (int)ib->sessions.size() ? ib->sessions[s] : nullptr;
    if (se0 && se0->pending_learn && !(se0->launched && mb_load(se0->state) == GMX_MB_RUNNING)) {
      int rc = ind_session_flush_learn(ib, s);
      if (rc) return rc;
    }
  }
  int rc = ind_session_ensure(ib, s, false);
  if (rc) return rc;
  GmxIndSession* se = ib->sessions[s];
  rc = ind_session_wait(ib, s);  // the previous command (a learn on its own) is done with the payload
  if (rc) return rc;
  const int K = ib->dev.k;
  uint32_t img[GMX_IND_MAX_MODELS];
  memset(img, 0, sizeof img);
  if (contexts) memcpy(img, contexts, (size_t)K * 4);  // (null: every column is the context bank's)
  // the other payload slot: the one of the forward still waiting for its learn stays intact (a wave
  // restarted in between recomputes that forward from it)
  se->slot ^= 1u;
  memcpy(se->mc->ctx[se->slot], img, sizeof img);
  se->mc->bit_context[se->slot] = bit_context;
  if (ib->match) {  // (every forward says what the Match lanes do: nothing, unless this is their chained forward)
    if (match) {
      uint32_t mimg[GMX_MATCH_MAX_MODELS] = {0};
      if (match->ctx) memcpy(mimg, match->ctx, (size_t)ib->match_k * 4);
      memcpy(se->mc->match_ctx[se->slot], mimg, sizeof mimg);
    }
    se->mc->match_what[se->slot] = (match && chain_word) ? match->what : 0u;
  }
  // (likewise, and whatever is attached: a slot never keeps the word of an earlier forward, which a wave with the
  // context phase, started after a later attach, would take for this forward's in a replay)
  se->ctx_what[se->slot] = (ib->ctx && ctx && chain_word) ? ctx->what : 0u;
  se->mc->ctx_what[se->slot] = se->ctx_what[se->slot];
  se->mc->chain_slot = chain_slot;
  se->mc->chain_mc = (uint64_t)(uintptr_t)chain_mc;
  se->mc->chain_word = chain_word;
  uint32_t cmd = GMX_MB_FORWARD;
  if (se->pending_learn) {
    cmd = se->pending_learn == 2 ? GMX_MB_LEARN1_FWD : GMX_MB_LEARN0_FWD;
    se->pending_learn = 0;
  }
  mb_publish(se, se->slot, cmd);
  rc = ind_session_wait(ib, s);
  if (rc) return rc;
  se->fwd_live = true;
  se->live_slot = se->slot;
  if (predictions) memcpy(predictions, se->mb->pred, (size_t)2 * K * 4);
  if (active) {
    const uint64_t a = se->mb->active_a, b = se->mb->active_b;
    for (int i = 0; i < K; ++i) {
      active[2 * i] = (uint8_t)((a >> i) & 1u);
      active[2 * i + 1] = (uint8_t)((b >> i) & 1u);
    }
  }
  if (ib->match && match && chain_word) {
    for (int i = 0; i < ib->match_k; ++i) {
      if (match->predictions) match->predictions[i] = se->mb->match_pred[i];
      if (match->active) match->active[i] = (uint8_t)(se->mb->match_active[i] != 0u);
    }
    if (match->longest_match) *match->longest_match = se->mb->longest_match;
  }
  if (ib->ctx && ctx && chain_word) {
    if (ctx->bit_context) *ctx->bit_context = se->mb->ctx_bit_context;
    if (ctx->values && (ctx->what & GMX_CTX_WAVE_VALUES)) memcpy(ctx->values, se->mb->ctx_values, (size_t)ib->ctx_v * 4);
  }
  return GMX_OK;
}

// ---- per-bit surface: K x Indirect::Predict / K x Indirect::Learn ---------------------------
static int ind_ensure_one(gmx_indirect* ib) {
  if (ib->one) return GMX_OK;
  int rc = ind_batch_alloc(&ib->one, ib, 1);
  if (rc) return rc;
  gmx_ind_batch* b = ib->one;
  if (!gmx_ind_batch_contexts(b) || !gmx_ind_batch_bit_contexts(b) || !gmx_ind_batch_bits(b) ||
      !gmx_ind_batch_predictions(b) || !gmx_ind_batch_active(b))
    return GMX_ERR_NOMEM;
  return GMX_OK;
}

extern "C" int gmx_indirect_forward(gmx_indirect* ib, int stream, const uint32_t* contexts, uint32_t bit_context,
                                    float* predictions, uint8_t* active) {
  if (!ib || stream < 0 || stream >= ib->S || !contexts) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(ib->device));
  if (ib->use_sessions) {
    int rcs = ind_session_forward(ib, stream, contexts, bit_context, predictions, active);
    if (rcs == GMX_OK) {
      ib->fwd_done[stream] = 2;  // this forward's learn goes the same way
      return GMX_OK;
    }
    if (rcs != GMX_ERR_STATE) return rcs;  // GMX_ERR_STATE: no session slot free -> a launch per call
  }
  {
    int rcs = ind_sessions_close(ib);
    if (rcs) return rcs;
  }
  int rc = ind_ensure_one(ib);
  if (rc) return rc;
  gmx_ind_batch* b = ib->one;
  const size_t K = ib->dev.k, s = (size_t)stream;
  HIPCHK(hipStreamSynchronize(ib->stream));
  memcpy(b->h_ctx + s * K, contexts, K * 4);
  b->h_bc[s] = bit_context;
  b->h_bits[s] = 0;
  HIPCHK(hipMemcpyAsync(b->d_ctx + s * K, b->h_ctx + s * K, K * 4, hipMemcpyHostToDevice, ib->stream));
  HIPCHK(hipMemcpyAsync(b->d_bc + s, b->h_bc + s, 4, hipMemcpyHostToDevice, ib->stream));
  rc = ind_launch(ib, b, stream, stream, 1, 1, 0, nullptr, nullptr);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(b->h_pred + s * 2 * K, b->d_pred + s * 2 * K, 8 * K, hipMemcpyDeviceToHost, ib->stream));
  HIPCHK(hipMemcpyAsync(b->h_act + s * 2 * K, b->d_act + s * 2 * K, 2 * K, hipMemcpyDeviceToHost, ib->stream));
  HIPCHK(hipStreamSynchronize(ib->stream));
  if (predictions) memcpy(predictions, b->h_pred + s * 2 * K, 8 * K);
  if (active) memcpy(active, b->h_act + s * 2 * K, 2 * K);
  ib->fwd_done[stream] = 1;
  return GMX_OK;
}

// Learn re-reads the contexts latched by the forward call: the reference's context variables do
// not move between Predict and Learn of a bit (they are updated in Predict, basic-contexts.cpp:21).
extern "C" int gmx_indirect_learn(gmx_indirect* ib, int stream, int bit) {
  if (!ib || stream < 0 || stream >= ib->S || (bit != 0 && bit != 1)) return GMX_ERR_INVALID;
  if (!ib->fwd_done[stream]) return GMX_ERR_STATE;
  if (ib->fwd_done[stream] == 2) {  // the forward went through a session: note the bit, it travels with the next command
    GmxIndSession* se = stream < (int)ib->sessions.size() ? ib->sessions[stream] : nullptr;
    if (!se || !se->fwd_live || se->pending_learn) return GMX_ERR_STATE;
    se->pending_learn = 1 + bit;
    ib->fwd_done[stream] = 0;
    return GMX_OK;
  }
  if (!ib->one) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(ib->device));
  gmx_ind_batch* b = ib->one;
  HIPCHK(hipStreamSynchronize(ib->stream));
  b->h_bits[stream] = (uint8_t)bit;
  HIPCHK(hipMemcpyAsync(b->d_bits + stream, b->h_bits + stream, 1, hipMemcpyHostToDevice, ib->stream));
  // same table entries, same slot values: the forward is recomputed, then learned from
  int rc = ind_launch(ib, b, stream, stream, 1, 1, 1, nullptr, nullptr);
  if (rc) return rc;
  // Not waited for: between Predictor::Learn of this bit and the Indirect models' Predict of the next the
  // host has the other feature models to run.  Every entry point that touches the bank or the staging
  // record synchronises the bank's stream first (the next forward included), so nothing sees a half-learned bit.
  ib->fwd_done[stream] = 0;
  return GMX_OK;
}

// ---- persistence: the indirect section of LongTermMemory (long-term-memory.cpp:8-32, :111-132)
static int ind_fetch(gmx_indirect* ib, int stream, std::vector<uint8_t>& img) {
  img.resize(ib->dev.bank_bytes);
  HIPCHK(hipSetDevice(ib->device));
  {
    int rcs = ind_sessions_close(ib);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(ib->stream));
  HIPCHK(hipMemcpy(img.data(), ib->banks + (size_t)stream * ib->dev.bank_bytes, img.size(), hipMemcpyDeviceToHost));
  return GMX_OK;
}

extern "C" int gmx_indirect_export(gmx_indirect* ib, int stream, void* buf, size_t* bytes) {
  if (!ib || stream < 0 || stream >= ib->S || !bytes) return GMX_ERR_INVALID;
  std::vector<uint8_t> img;
  int rc = ind_fetch(ib, stream, img);
  if (rc) return rc;
  const GmxIndDev& d = ib->dev;
  std::vector<uint32_t> cnt(d.k, 0);
  size_t need = 0;
  for (int i = 0; i < d.k; ++i) {
    const uint16_t* tab = (const uint16_t*)(img.data() + d.m[i].tab_off);
    uint32_t c = 0;
    for (uint32_t j = 0; j < d.m[i].size; ++j) c += (tab[j] & 255u) != 255u;
    cnt[i] = c;
    need += 4 + (c < d.m[i].size / 3 ? 6ull * c : 2ull * d.m[i].size) + 2048;
  }
  const bool fits = buf && *bytes >= need;
  *bytes = need;
  if (!buf) return GMX_OK;
  if (!fits) return GMX_ERR_INVALID;
  uint8_t* o = (uint8_t*)buf;
  for (int i = 0; i < d.k; ++i) {
    const uint16_t* tab = (const uint16_t*)(img.data() + d.m[i].tab_off);
    const uint32_t size = d.m[i].size;
    memcpy(o, &cnt[i], 4);
    o += 4;
    if (cnt[i] < size / 3) {  // sparse: key, nonstationary state, run-map state
      for (uint32_t j = 0; j < size; ++j)
        if ((tab[j] & 255u) != 255u) {
          memcpy(o, &j, 4);
          o[4] = (uint8_t)(tab[j] & 255u);
          o[5] = (uint8_t)(tab[j] >> 8);
          o += 6;
        }
    } else {  // dense: the two byte tables one after the other
      for (uint32_t j = 0; j < size; ++j) o[j] = (uint8_t)(tab[j] & 255u);
      o += size;
      for (uint32_t j = 0; j < size; ++j) o[j] = (uint8_t)(tab[j] >> 8);
      o += size;
    }
    memcpy(o, img.data() + d.pred_off + (size_t)i * 2048, 2048);
    o += 2048;
  }
  return GMX_OK;
}

extern "C" int gmx_indirect_import(gmx_indirect* ib, int stream, const void* buf, size_t bytes) {
  if (!ib || stream < 0 || stream >= ib->S || !buf) return GMX_ERR_INVALID;
  const GmxIndDev& d = ib->dev;
  std::vector<uint8_t> img(d.bank_bytes, 0);
  for (uint64_t j = 0; j < ib->tab_bytes / 2; ++j) ((uint16_t*)img.data())[j] = 0x00ffu;
  const uint8_t* p = (const uint8_t*)buf;
  const uint8_t* end = p + bytes;
  for (int i = 0; i < d.k; ++i) {
    uint16_t* tab = (uint16_t*)(img.data() + d.m[i].tab_off);
    const uint32_t size = d.m[i].size;
    if (end - p < 4) return GMX_ERR_FORMAT;
    uint32_t cnt;
    memcpy(&cnt, p, 4);
    p += 4;
    if (cnt > size) return GMX_ERR_FORMAT;
    if (cnt < size / 3) {
      if ((size_t)(end - p) < 6ull * cnt) return GMX_ERR_FORMAT;
      for (uint32_t c = 0; c < cnt; ++c) {
        uint32_t key;
        memcpy(&key, p, 4);
        if (key >= size) return GMX_ERR_FORMAT;
        tab[key] = (uint16_t)(p[4] | (p[5] << 8));
        p += 6;
      }
    } else {
      if ((size_t)(end - p) < 2ull * size) return GMX_ERR_FORMAT;
      for (uint32_t j = 0; j < size; ++j) tab[j] = (uint16_t)(p[j] | (p[size + j] << 8));
      p += 2ull * size;
    }
    if (end - p < 2048) return GMX_ERR_FORMAT;
    memcpy(img.data() + d.pred_off + (size_t)i * 2048, p, 2048);
    p += 2048;
  }
  if (p != end) return GMX_ERR_FORMAT;
  HIPCHK(hipSetDevice(ib->device));
  {
    int rcs = ind_sessions_close(ib);
    if (rcs) return rcs;
    ind_sessions_drop_forward(ib, stream);
  }
  HIPCHK(hipStreamSynchronize(ib->stream));
  HIPCHK(hipMemcpy(ib->banks + (size_t)stream * d.bank_bytes, img.data(), img.size(), hipMemcpyHostToDevice));
  ib->fwd_done[stream] = 0;
  return GMX_OK;
}

// LongTermMemory::Copy, indirect part (long-term-memory.cpp:193-199).
extern "C" int gmx_indirect_copy(gmx_indirect* dst, int dst_stream, gmx_indirect* src, int src_stream) {
  if (!dst || !src || dst_stream < 0 || dst_stream >= dst->S || src_stream < 0 || src_stream >= src->S)
    return GMX_ERR_INVALID;
  if (dst->dev.k != src->dev.k || dst->dev.bank_bytes != src->dev.bank_bytes) return GMX_ERR_INVALID;
  for (int i = 0; i < dst->dev.k; ++i)
    if (dst->dev.m[i].size != src->dev.m[i].size) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(src->device));
  {
    int rcs = ind_sessions_close(src);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(src->stream));
  HIPCHK(hipSetDevice(dst->device));
  {
    int rcs = ind_sessions_close(dst);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(dst->stream));
  // tables and logits; the blackboard slots belong to ShortTermMemory, whose Copy also copies them
  HIPCHK(hipMemcpy(dst->banks + (size_t)dst_stream * dst->dev.bank_bytes,
                   src->banks + (size_t)src_stream * src->dev.bank_bytes, dst->dev.bank_bytes,
                   hipMemcpyDeviceToDevice));
  dst->fwd_done[dst_stream] = 0;
  ind_sessions_drop_forward(dst, dst_stream);
  return GMX_OK;
}

// The models' blackboard slots as the bank holds them (see include/gmxmix.h).
static int ind_slots_move(gmx_indirect* ib, int stream, float* get, const float* set) {
  if (!ib || stream < 0 || stream >= ib->S || (!get && !set)) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(ib->device));
  {
    int rcs = ind_sessions_close(ib);  // (a session keeps them in registers)
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(ib->stream));
  uint8_t* const at = ib->banks + (size_t)stream * ib->dev.bank_bytes + ib->dev.slots_off;
  const size_t n = 2 * (size_t)ib->dev.k * sizeof(float);
  if (get) HIPCHK(hipMemcpy(get, at, n, hipMemcpyDeviceToHost));
  if (set) HIPCHK(hipMemcpy(at, set, n, hipMemcpyHostToDevice));
  return GMX_OK;
}
extern "C" int gmx_indirect_slots_get(gmx_indirect* ib, int stream, float* values) {
  return ind_slots_move(ib, stream, values, nullptr);
}
extern "C" int gmx_indirect_slots_set(gmx_indirect* ib, int stream, const float* values) {
  return ind_slots_move(ib, stream, nullptr, values);
}

// Indirect::GetMemoryUsage (indirect.cpp:71-78): a constant of the table size.
extern "C" int gmx_indirect_memory_usage(gmx_indirect* ib, int model, uint64_t* bytes) {
  if (!ib || model < 0 || model >= ib->dev.k || !bytes) return GMX_ERR_INVALID;
  *bytes = 12ull + 256 * 4 * 2 + 2ull * ib->dev.m[model].size;
  return GMX_OK;
}
