// gmx_match.inc -- host side of the Match-model banks (included by gmx_capi.cpp).
//
// Replaces the reference's `Match` objects (models/match.{h,cpp}, constructed in predictor.cpp:187-208), their
// MatchMemory and the deduplicated history (long-term-memory.h:42-53, :82), and the history rule of
// BasicContexts::Learn (basic-contexts.cpp:44-53), for S independent streams.  Compute is gmx_match.hip; nothing
// here falls back to the CPU.

struct gmx_match_batch : GmxBatchCore {
  gmx_match* mb = nullptr;
  uint64_t& max_bits = max_rows;
  uint32_t* d_ctx = nullptr;
  uint32_t* d_bc = nullptr;
  uint8_t* d_bits = nullptr;
  float* d_pred = nullptr;
  uint8_t* d_act = nullptr;
  uint32_t* d_long = nullptr;
  uint32_t* h_ctx = nullptr;
  uint32_t* h_bc = nullptr;
  uint8_t* h_bits = nullptr;
  float* h_pred = nullptr;
  uint8_t* h_act = nullptr;
  uint32_t* h_long = nullptr;
};

struct gmx_match {
  int device = 0, S = 0;
  GmxMatchDev dev;                 // host copy
  GmxMatchDev* dev_d = nullptr;
  uint8_t* banks = nullptr;        // [S][bank_bytes]
  uint8_t* hist = nullptr;         // [S][hist_cap]
  hipStream_t stream = nullptr;    // kernels AND record transfers: the bank adds ONE stream to its priority level
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  GmxBatchBank bb;                 // its record batches
  gmx_match_batch* one = nullptr;  // 1-bit batch of the per-bit surface
  std::vector<uint8_t> fwd_done;   // per-bit protocol: forward seen, learn allowed
  std::vector<uint32_t> fwd_bc;    // bit_context of that forward
  std::vector<uint64_t> hist_bound;  // upper bound of every stream's history size
  GmxCountList counts;
  // checkpoint: the chunk list (the same for every stream) and its device arrays, lazily
  std::vector<GmxMatchCkptChunk> chunks;
  GmxMatchCkptChunk* chunks_d = nullptr;
  uint32_t* chunk_cnt_d = nullptr;
  uint32_t* chunk_base_d = nullptr;
  uint32_t* model_cnt_d = nullptr;
  uint8_t* model_dense_d = nullptr;
  uint64_t* model_off_d = nullptr;
  uint64_t gck_ops = 0;  // launches, transfers, synchronisations, allocations of the group checkpoint calls so far
  // gmx_indirect_attach_match: the bank's streams ride in the per-bit session waves of `host` (lanes 56..63 of
  // gmx_indirect_session_kernel<true>).  fwd_done[s] == 2: the stream's newest forward went that way, and its
  // gmx_match_learn only notes the bit (noted[s] = 1 + bit), which travels with the next chained forward.  Nothing of
  // a stream's state lives outside the bank, so "up to date" means: no wave running, no learn noted (match_settle).
  gmx_indirect* host = nullptr;
  std::vector<uint8_t> noted;
  std::vector<gmx_chainstep*> chainsteps;  // the lock-step objects this bank is attached to, each registered here:
                                           // whichever of the two is destroyed first tells the other
};
static void chainstep_match_gone(gmx_chainstep* cs);  // gmx_chainstep.inc
static int match_settle(gmx_match* mb);

extern "C" {
hipError_t gmx_launch_match_kernel(const GmxMatchDev* dv, const GmxMatchRunArgs* args, hipStream_t stream);
hipError_t gmx_launch_match_init(const GmxMatchDev* dv, uint8_t* banks, int stream_base, int n_streams,
                                 hipStream_t stream);
hipError_t gmx_launch_match_ckpt_count(const GmxMatchCkptArgs* a, hipStream_t stream);
hipError_t gmx_launch_match_ckpt_pack(const GmxMatchCkptArgs* a, hipStream_t stream);
hipError_t gmx_launch_match_ckpt_scatter(const GmxMatchCkptArgs* a, int n_models, unsigned blocks_x,
                                         hipStream_t stream);
}
static int stream_with_cu_mask(hipStream_t* st, const uint32_t* mask, int n_words);

static void match_batch_free(gmx_match_batch* b) {
  if (!b) return;
  batch_core_free(*b);
  delete b;
}

extern "C" void gmx_match_destroy(gmx_match* mb) {
  if (!mb) return;
  (void)hipSetDevice(mb->device);
  if (mb->host) (void)match_host_detach(mb);  // (no wave of the host's reads this bank any more)
  for (gmx_chainstep* cs : mb->chainsteps) chainstep_match_gone(cs);
  mb->chainsteps.clear();
  if (mb->stream) (void)hipStreamSynchronize(mb->stream);
  if (mb->one) {
    match_batch_free(mb->one);
    mb->one = nullptr;
  }
  batch_bank_detach_all(mb->bb);  // shells, as for gmx_batch
  void* dv[] = {mb->banks,       mb->hist,          mb->dev_d,       mb->chunks_d, mb->chunk_cnt_d, mb->chunk_base_d,
                mb->model_cnt_d, mb->model_dense_d, mb->model_off_d};
  for (void* p : dv)
    if (p) (void)hipFree(p);
  if (mb->ev0) (void)hipEventDestroy(mb->ev0);
  if (mb->ev1) (void)hipEventDestroy(mb->ev1);
  count_list_free(mb->counts);
  if (mb->stream) (void)hipStreamDestroy(mb->stream);
  delete mb;
}

extern "C" int gmx_match_reset(gmx_match* mb) {
  if (!mb) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(mb->device));
  if (mb->host) {  // (a noted learn is void with the state it would have moved)
    int rcs = ind_sessions_close(mb->host);
    if (rcs) return rcs;
  }
  std::fill(mb->noted.begin(), mb->noted.end(), 0);
  HIPCHK(gmx_launch_match_init(mb->dev_d, mb->banks, 0, mb->S, mb->stream));
  HIPCHK(hipStreamSynchronize(mb->stream));
  std::fill(mb->fwd_done.begin(), mb->fwd_done.end(), 0);
  std::fill(mb->hist_bound.begin(), mb->hist_bound.end(), 0);
  return GMX_OK;
}

extern "C" int gmx_match_create(gmx_match** out, const gmx_match_desc* models, int n_models,
                                uint64_t history_capacity, int n_streams, int device) {
  if (!out) return GMX_ERR_INVALID;
  *out = nullptr;
  if (!models || n_models < 1 || n_models > GMX_MATCH_MAX_MODELS || n_streams < 1 || history_capacity == 0 ||
      history_capacity >= (1ull << 32))
    return GMX_ERR_INVALID;
  GmxMatchDev d;
  memset(&d, 0, sizeof d);
  d.k = n_models;
  uint64_t off = 0;
  std::vector<char> used(2048, 0);
  for (int i = 0; i < n_models; ++i) {
    const gmx_match_desc& m = models[i];
    if (m.table_size == 0 || m.limit < 1 || m.slot < 0 || m.slot >= 2048 || used[m.slot]) return GMX_ERR_INVALID;
    used[m.slot] = 1;
    d.m[i].tab_off = off;
    d.m[i].table_size = m.table_size;
    d.m[i].limit = m.limit;
    d.m[i].slot = m.slot;
    d.m[i].rate_at_limit = (float)(1.0 / m.limit);  // match.cpp:13
    off += round_up64(4ull * m.table_size, 256);
    d.n_slots = std::max(d.n_slots, m.slot + 1);
  }
  d.tab_bytes = off;
  d.pred_off = off;
  off += (uint64_t)n_models * 1024;
  d.cnt_off = off;
  off += (uint64_t)n_models * 1024;
  d.mstate_off = off;
  off += GMX_MATCH_MAX_MODELS * sizeof(GmxMatchModelState);
  d.sstate_off = off;
  off += sizeof(GmxMatchStreamState);
  d.bank_bytes = round_up64(off, 256);
  d.hist_cap = history_capacity;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return GMX_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(device));
  gmx_match* mb = new (std::nothrow) gmx_match();
  if (!mb) return GMX_ERR_NOMEM;
  mb->device = device;
  batch_bank_init(mb->bb, mb, device, &mb->stream);  // (no transfer streams: see gmx_match_batch_upload)
  mb->S = n_streams;
  mb->dev = d;
  mb->fwd_done.assign(n_streams, 0);
  mb->fwd_bc.assign(n_streams, 0);
  mb->noted.assign(n_streams, 0);
  mb->hist_bound.assign(n_streams, 0);
  for (int i = 0; i < n_models; ++i)
    for (uint32_t e = 0; e < d.m[i].table_size; e += GMX_MATCH_CKPT_CHUNK) {
      mb->chunks.push_back(GmxMatchCkptChunk{(uint32_t)i, e});
      if (d.m[i].table_size - e <= (uint32_t)GMX_MATCH_CKPT_CHUNK) break;  // (no wrap for sizes near 2^32)
    }
#define MCHK(call)                                 \
  do {                                             \
    hipError_t e_ = (call);                        \
    if (e_ != hipSuccess) {                        \
      int r_ = hip_fail(e_, #call);                \
      gmx_match_destroy(mb);                       \
      return e_ == hipErrorOutOfMemory ? GMX_ERR_NOMEM : r_; \
    }                                              \
  } while (0)
  MCHK(bank_stream_create(&mb->stream, 1));
  MCHK(hipEventCreate(&mb->ev0));
  MCHK(hipEventCreate(&mb->ev1));
  MCHK(hipMalloc((void**)&mb->dev_d, sizeof(GmxMatchDev)));
  MCHK(hipMemcpy(mb->dev_d, &mb->dev, sizeof(GmxMatchDev), hipMemcpyHostToDevice));
  MCHK(hipMalloc((void**)&mb->banks, (size_t)n_streams * d.bank_bytes));
  MCHK(hipMalloc((void**)&mb->hist, (size_t)n_streams * d.hist_cap));
#undef MCHK
  int rc = gmx_match_reset(mb);
  if (rc) {
    gmx_match_destroy(mb);
    return rc;
  }
  *out = mb;
  return GMX_OK;
}

extern "C" int gmx_match_n_streams(const gmx_match* mb) { return mb ? mb->S : GMX_ERR_INVALID; }
extern "C" int gmx_match_n_models(const gmx_match* mb) { return mb ? mb->dev.k : GMX_ERR_INVALID; }
extern "C" uint64_t gmx_match_bank_bytes(const gmx_match* mb) { return mb ? mb->dev.bank_bytes + mb->dev.hist_cap : 0; }
extern "C" int gmx_match_sync(gmx_match* mb) {
  if (!mb) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(mb->device));
  {
    int rcs = match_settle(mb);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(mb->stream));
  return GMX_OK;
}
extern "C" int gmx_match_set_cu_mask(gmx_match* mb, const uint32_t* mask, int n_words) {
  if (!mb || n_words < 0 || (n_words > 0 && !mask)) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(mb->device));
  {
    int rcs = match_settle(mb);
    if (rcs) return rcs;
  }
  return stream_with_cu_mask(&mb->stream, mask, n_words);
}

// ---- record batches ------------------------------------------------------------------------
static int match_batch_alloc(gmx_match_batch** out, gmx_match* mb, uint64_t max_bits) {
  if (!out) return GMX_ERR_INVALID;
  *out = nullptr;
  if (!mb || max_bits == 0) return GMX_ERR_INVALID;
  gmx_match_batch* b = new (std::nothrow) gmx_match_batch();
  if (!b) return GMX_ERR_NOMEM;
  b->back = (void**)&b->mb;
  gmx_match_batch_cols(b->cols, b, mb->dev.k);
  int rc = batch_core_alloc(*b, &mb->bb, mb->S, max_bits, false);
  if (rc) {
    match_batch_free(b);
    return rc;
  }
  *out = b;
  return GMX_OK;
}

extern "C" int gmx_match_batch_create(gmx_match_batch** out, gmx_match* mb, uint64_t max_bits) {
  return match_batch_alloc(out, mb, max_bits);
}
extern "C" void gmx_match_batch_destroy(gmx_match_batch* b) { match_batch_free(b); }
extern "C" uint64_t gmx_match_batch_max_bits(const gmx_match_batch* b) { return b ? b->max_bits : 0; }

extern "C" uint32_t* gmx_match_batch_contexts(gmx_match_batch* b) {
  return b ? (uint32_t*)batch_core_host(*b, &b->h_ctx) : nullptr;
}
extern "C" uint32_t* gmx_match_batch_bit_contexts(gmx_match_batch* b) {
  return b ? (uint32_t*)batch_core_host(*b, &b->h_bc) : nullptr;
}
extern "C" uint8_t* gmx_match_batch_bits(gmx_match_batch* b) {
  return b ? (uint8_t*)batch_core_host(*b, &b->h_bits) : nullptr;
}
extern "C" const float* gmx_match_batch_predictions(gmx_match_batch* b) {
  return b ? (float*)batch_core_host(*b, &b->h_pred) : nullptr;
}
extern "C" const uint8_t* gmx_match_batch_active(gmx_match_batch* b) {
  return b ? (uint8_t*)batch_core_host(*b, &b->h_act) : nullptr;
}
extern "C" const uint32_t* gmx_match_batch_longest(gmx_match_batch* b) {
  return b ? (uint32_t*)batch_core_host(*b, &b->h_long) : nullptr;
}

// On the bank's own stream: the Match bank shares its priority level with the Indirect banks, whose three streams
// leave one of the level's four hardware queues (see bank_stream_create), and its records are 29 bytes a bit.
extern "C" int gmx_match_batch_upload(gmx_match_batch* b, uint64_t n_bits) {
  return batch_core_transfer(b, n_bits, GMX_COL_UP);
}
extern "C" int gmx_match_batch_download(gmx_match_batch* b, uint64_t n_bits) {
  return batch_core_transfer(b, n_bits, GMX_COL_DOWN);
}
extern "C" int gmx_match_batch_wait(gmx_match_batch* b) { return batch_core_wait(b); }

// ---- capacity --------------------------------------------------------------------------------
// The true history sizes from the device (the bank's stream is drained first).
static int match_refresh_sizes(gmx_match* mb) {
  HIPCHK(hipStreamSynchronize(mb->stream));
  for (int s = 0; s < mb->S; ++s) {
    GmxMatchStreamState st;
    HIPCHK(hipMemcpy(&st, mb->banks + (size_t)s * mb->dev.bank_bytes + mb->dev.sstate_off, sizeof st,
                     hipMemcpyDeviceToHost));
    mb->hist_bound[s] = st.hist_size;
  }
  return GMX_OK;
}
// A launch of add[i] bytes at most for stream s0 + i: GMX_ERR_INVALID, and nothing queued, when a history could
// overflow; the bounds are raised otherwise.
static int match_reserve(gmx_match* mb, int s0, int ns, const uint64_t* add) {
  bool tight = false;
  for (int i = 0; i < ns; ++i) tight = tight || mb->hist_bound[s0 + i] + add[i] > mb->dev.hist_cap;
  if (tight) {
    int rc = match_refresh_sizes(mb);
    if (rc) return rc;
    for (int i = 0; i < ns; ++i)
      if (mb->hist_bound[s0 + i] + add[i] > mb->dev.hist_cap) return GMX_ERR_INVALID;
  }
  for (int i = 0; i < ns; ++i) mb->hist_bound[s0 + i] += add[i];
  return GMX_OK;
}

// ---- compute -------------------------------------------------------------------------------
static int match_launch(gmx_match* mb, gmx_match_batch* b, int s0, int rec0, int ns, uint64_t T, unsigned what,
                        gmx_batch* into, const int32_t* ctx_columns, int n_ctx_columns, float* kernel_ms,
                        const uint64_t* n_list = nullptr) {
  if (T == 0) return GMX_OK;
  GmxMatchRunArgs a;
  memset(&a, 0, sizeof a);
  a.banks = mb->banks;
  a.hist = mb->hist;
  a.ctx = b->d_ctx;
  a.bc = b->d_bc;
  a.bits = b->d_bits;
  a.pred_out = b->d_pred;
  a.act_out = b->d_act;
  a.longest_out = b->d_long;
  a.rec_stride = b->max_bits;
  a.T = T;
  a.what = what;
  a.stream_base = s0;
  a.rec_base = rec0;
  a.n_streams = ns;
  if (n_list) {
    int rcl = count_list_stage(mb->counts, n_list, ns, mb->stream, &a.T_list);
    if (rcl) return rcl;
  }
  if (into) {
    a.mx_pred = into->d_pred;
    a.mx_mask = into->d_mask;
    a.mx_ctx = into->d_ctx;
    a.mx_rec_stride = into->max_bits;
    a.mx_n_pad = into->g->topo.n_pad;
    a.mx_mask_words = into->g->topo.mask_words;
    a.mx_m = into->g->topo.m;
    a.n_ctx_cols = n_ctx_columns;
    for (int c = 0; c < n_ctx_columns; ++c) a.ctx_cols[c] = ctx_columns[c];
    int rcw = xfer_writer_waits(into->x, mb->stream);
    if (rcw) return rcw;
  }
  {
    int rcx = xfer_before_run(b->x, mb->stream);
    if (rcx) return rcx;
  }
  if (kernel_ms) HIPCHK(hipEventRecord(mb->ev0, mb->stream));
  HIPCHK(gmx_launch_match_kernel(mb->dev_d, &a, mb->stream));
  if (n_list) {
    int rcl = count_list_used(mb->counts, mb->stream);
    if (rcl) return rcl;
  }
  {
    int rcx = xfer_note_device_use(b->x, mb->stream);
    if (rcx) return rcx;
  }
  if (kernel_ms) {
    HIPCHK(hipEventRecord(mb->ev1, mb->stream));
    HIPCHK(hipEventSynchronize(mb->ev1));
    HIPCHK(hipEventElapsedTime(kernel_ms, mb->ev0, mb->ev1));
  }
  if (into) {
    int rcn = xfer_writer_done(into->x, mb->stream, into->g->stream);
    if (rcn) return rcn;
  }
  return GMX_OK;
}

static int match_into_ok(const gmx_match* mb, const gmx_batch* into, const int32_t* ctx_columns, int n_ctx_columns) {
  if (!into) return (n_ctx_columns == 0) ? GMX_OK : GMX_ERR_INVALID;
  if (!into->g || into->S != mb->S || into->g->device != mb->device || !into->d_mask ||
      mb->dev.n_slots > into->g->topo.n || into->g->topo.mask_words > GMX_MATCH_MAX_MASK_WORDS)
    return GMX_ERR_INVALID;
  if (n_ctx_columns < 0 || n_ctx_columns > GMX_MATCH_MAX_CTX_COLS || (n_ctx_columns > 0 && !ctx_columns))
    return GMX_ERR_INVALID;
  for (int c = 0; c < n_ctx_columns; ++c)
    if (ctx_columns[c] < 0 || ctx_columns[c] >= into->g->topo.m) return GMX_ERR_INVALID;
  return GMX_OK;
}

extern "C" int gmx_match_run_ragged(gmx_match* mb, gmx_match_batch* b, const uint64_t* n_bits, gmx_batch* into,
                                    const int32_t* ctx_columns, int n_ctx_columns) {
  if (!mb || !b || b->mb != mb || !n_bits) return GMX_ERR_INVALID;
  for (int s = 0; s < mb->S; ++s)
    if (n_bits[s] > b->max_bits || (into && n_bits[s] > into->max_bits)) return GMX_ERR_INVALID;
  int rc = match_into_ok(mb, into, ctx_columns, n_ctx_columns);
  if (rc) return rc;
  HIPCHK(hipSetDevice(mb->device));
  rc = match_settle(mb);
  if (rc) return rc;
  uint64_t maxn = 0;
  bool same = true;
  std::vector<uint64_t> add(mb->S);
  for (int s = 0; s < mb->S; ++s) {
    maxn = std::max(maxn, n_bits[s]);
    same = same && n_bits[s] == n_bits[0];
    add[s] = (n_bits[s] + 7) / 8;  // bytes a run of n bits may complete, wherever in a byte it begins
  }
  rc = match_reserve(mb, 0, mb->S, add.data());
  if (rc) return rc;
  std::fill(mb->fwd_done.begin(), mb->fwd_done.end(), 0);
  return match_launch(mb, b, 0, 0, mb->S, maxn, GMX_MATCH_PREDICT | GMX_MATCH_LEARN, into, ctx_columns,
                      n_ctx_columns, nullptr, same ? nullptr : n_bits);
}

extern "C" int gmx_match_run(gmx_match* mb, gmx_match_batch* b, uint64_t n_bits, gmx_batch* into,
                             const int32_t* ctx_columns, int n_ctx_columns, float* kernel_ms) {
  if (!mb || !b || b->mb != mb || n_bits > b->max_bits || (into && n_bits > into->max_bits)) return GMX_ERR_INVALID;
  int rc = match_into_ok(mb, into, ctx_columns, n_ctx_columns);
  if (rc) return rc;
  HIPCHK(hipSetDevice(mb->device));
  rc = match_settle(mb);
  if (rc) return rc;
  std::vector<uint64_t> add(mb->S, (n_bits + 7) / 8);
  rc = match_reserve(mb, 0, mb->S, add.data());
  if (rc) return rc;
  std::fill(mb->fwd_done.begin(), mb->fwd_done.end(), 0);
  if (kernel_ms) *kernel_ms = 0.0f;
  return match_launch(mb, b, 0, 0, mb->S, n_bits, GMX_MATCH_PREDICT | GMX_MATCH_LEARN, into, ctx_columns,
                      n_ctx_columns, kernel_ms);
}

// ---- per-bit surface: K x Match::Predict / the history push + K x Match::Learn, a launch per call ---------
static int match_ensure_one(gmx_match* mb) {
  if (mb->one) return GMX_OK;
  int rc = match_batch_alloc(&mb->one, mb, 1);
  if (rc) return rc;
  gmx_match_batch* b = mb->one;
  if (!gmx_match_batch_contexts(b) || !gmx_match_batch_bit_contexts(b) || !gmx_match_batch_bits(b) ||
      !gmx_match_batch_predictions(b) || !gmx_match_batch_active(b) || !gmx_match_batch_longest(b))
    return GMX_ERR_NOMEM;
  return GMX_OK;
}

// (the launch path itself; the caller has seen to the protocol and, where the bank is hosted, to the sessions)
static int match_forward_launch(gmx_match* mb, int stream, const uint32_t* contexts, uint32_t bit_context,
                                float* predictions, uint8_t* active, uint32_t* longest_match) {
  int rc = match_ensure_one(mb);
  if (rc) return rc;
  gmx_match_batch* b = mb->one;
  const size_t K = mb->dev.k, s = (size_t)stream;
  HIPCHK(hipStreamSynchronize(mb->stream));
  memcpy(b->h_ctx + s * K, contexts, K * 4);
  b->h_bc[s] = bit_context;
  HIPCHK(hipMemcpyAsync(b->d_ctx + s * K, b->h_ctx + s * K, K * 4, hipMemcpyHostToDevice, mb->stream));
  HIPCHK(hipMemcpyAsync(b->d_bc + s, b->h_bc + s, 4, hipMemcpyHostToDevice, mb->stream));
  rc = match_launch(mb, b, stream, stream, 1, 1, GMX_MATCH_PREDICT, nullptr, nullptr, 0, nullptr);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(b->h_pred + s * K, b->d_pred + s * K, 4 * K, hipMemcpyDeviceToHost, mb->stream));
  HIPCHK(hipMemcpyAsync(b->h_act + s * K, b->d_act + s * K, K, hipMemcpyDeviceToHost, mb->stream));
  HIPCHK(hipMemcpyAsync(b->h_long + s, b->d_long + s, 4, hipMemcpyDeviceToHost, mb->stream));
  HIPCHK(hipStreamSynchronize(mb->stream));
  if (predictions) memcpy(predictions, b->h_pred + s * K, 4 * K);
  if (active) memcpy(active, b->h_act + s * K, K);
  if (longest_match) *longest_match = b->h_long[s];
  mb->fwd_done[stream] = 1;
  mb->fwd_bc[stream] = bit_context;
  return GMX_OK;
}

extern "C" int gmx_match_forward(gmx_match* mb, int stream, const uint32_t* contexts, uint32_t bit_context,
                                 float* predictions, uint8_t* active, uint32_t* longest_match) {
  if (!mb || stream < 0 || stream >= mb->S || !contexts || bit_context > 254u) return GMX_ERR_INVALID;
  if (mb->fwd_done[stream]) return GMX_ERR_STATE;  // Match::Predict moves state: one per bit
  HIPCHK(hipSetDevice(mb->device));
  int rc = match_settle(mb);
  if (rc) return rc;
  return match_forward_launch(mb, stream, contexts, bit_context, predictions, active, longest_match);
}

// The history push and K x Match::Learn of the stream's newest forward, on what that forward left in the bank.
static int match_learn_launch(gmx_match* mb, int stream, int bit) {
  const uint64_t add = mb->fwd_bc[stream] >= 127u ? 1 : 0;
  int rc = match_reserve(mb, stream, 1, &add);
  if (rc) return rc;
  rc = match_ensure_one(mb);
  if (rc) return rc;
  gmx_match_batch* b = mb->one;
  HIPCHK(hipStreamSynchronize(mb->stream));
  b->h_bits[stream] = (uint8_t)bit;
  HIPCHK(hipMemcpyAsync(b->d_bits + stream, b->h_bits + stream, 1, hipMemcpyHostToDevice, mb->stream));
  return match_launch(mb, b, stream, stream, 1, 1, GMX_MATCH_LEARN, nullptr, nullptr, 0, nullptr);
}

extern "C" int gmx_match_learn(gmx_match* mb, int stream, int bit) {
  if (!mb || stream < 0 || stream >= mb->S || (bit != 0 && bit != 1)) return GMX_ERR_INVALID;
  if (mb->fwd_done[stream] == 2 && mb->host) {
    // the forward went through a session wave: the bit is noted and travels with the stream's next chained forward
    // as one command (or takes the launch path when something else needs the bank first: match_settle).  The history
    // byte it may push is reserved now, as on the launch path: refused here, nothing is noted and no bank moves
    HIPCHK(hipSetDevice(mb->device));
    const uint64_t add = mb->fwd_bc[stream] >= 127u ? 1 : 0;
    int rc = match_reserve(mb, stream, 1, &add);
    if (rc) return rc;
    mb->noted[stream] = (uint8_t)(1 + bit);
    mb->fwd_done[stream] = 0;
    return GMX_OK;
  }
  if (!mb->fwd_done[stream]) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(mb->device));
  int rc = match_learn_launch(mb, stream, bit);
  if (rc) return rc;
  mb->fwd_done[stream] = 0;  // not waited for: every entry point that touches the bank synchronises first
  return GMX_OK;
}

// A learn gmx_match_learn noted for stream s: run it through the launch path now.
static int match_flush_noted(gmx_match* mb, int s) {
  if (!mb->noted[s]) return GMX_OK;
  int rc = match_learn_launch(mb, s, mb->noted[s] - 1);
  if (rc) return rc;
  mb->noted[s] = 0;
  return GMX_OK;
}

// The bank is about to be read or written by something that is not a session wave: the host's waves stop (they keep
// nothing of a stream's Match state, so there is nothing to write back) and every noted learn is run.
static int match_settle(gmx_match* mb) {
  if (!mb->host) return GMX_OK;
  HIPCHK(hipSetDevice(mb->device));
  int first = ind_sessions_close(mb->host);
  for (int s = 0; s < mb->S; ++s) {
    int rc = match_flush_noted(mb, s);
    if (rc && !first) first = rc;
  }
  return first;
}

// Either object goes, or the attachment is given up: the waves stop, a noted learn is run, and a forward that went
// through a wave is from now on an ordinary pending forward of the launch path.
static int match_host_detach(gmx_match* mb) {
  if (!mb || !mb->host) return GMX_OK;
  const int rc = match_settle(mb);
  for (int s = 0; s < mb->S; ++s)
    if (mb->fwd_done[s] == 2) mb->fwd_done[s] = 1;
  gmx_indirect* ib = mb->host;
  ib->match = nullptr;
  ib->match_dev_d = nullptr;
  ib->match_banks = ib->match_hist = nullptr;
  ib->match_k = ib->match_n_cols = 0;
  mb->host = nullptr;
  return rc;
}

extern "C" int gmx_indirect_attach_match(gmx_indirect* ib, gmx_match* mb, const int32_t* ctx_columns,
                                         int n_ctx_columns) {
  if (!ib) return GMX_ERR_INVALID;
  if (!mb) {  // detach
    HIPCHK(hipSetDevice(ib->device));
    return ib->match ? match_host_detach(ib->match) : GMX_OK;
  }
  if (ib->dev.k > 56 || mb->S != ib->S || mb->device != ib->device) return GMX_ERR_INVALID;
  if (n_ctx_columns < 0 || n_ctx_columns > GMX_MATCH_MAX_CTX_COLS || (n_ctx_columns > 0 && !ctx_columns))
    return GMX_ERR_INVALID;
  for (int c = 0; c < n_ctx_columns; ++c)
    if (ctx_columns[c] < 0) return GMX_ERR_INVALID;  // (the upper bound is the mixer group's: checked at the call)
  for (int i = 0; i < mb->dev.k; ++i)
    for (int j = 0; j < ib->dev.k; ++j)
      if (mb->dev.m[i].slot == ib->dev.m[j].slot_a || mb->dev.m[i].slot == ib->dev.m[j].slot_b) return GMX_ERR_INVALID;
  if (!mb->chainsteps.empty()) return GMX_ERR_STATE;            // one host of its per-bit state at a time
  if (mb->host && mb->host != ib) return GMX_ERR_STATE;
  if (ib->ctx) return GMX_ERR_STATE;  // (gmx_indirect_attach_ctx's routes were made for the banks there were: Match first)
  HIPCHK(hipSetDevice(ib->device));
  int rc = ib->match ? match_host_detach(ib->match) : GMX_OK;  // (another bank, or this one with other columns)
  if (rc) return rc;
  rc = ind_sessions_close(ib);  // the waves that run are the build without the Match lanes
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(mb->stream));
  ib->match = mb;
  ib->match_dev_d = mb->dev_d;
  ib->match_banks = mb->banks;
  ib->match_hist = mb->hist;
  ib->match_bank_bytes = mb->dev.bank_bytes;
  ib->match_hist_cap = mb->dev.hist_cap;
  ib->match_k = mb->dev.k;
  ib->match_n_cols = n_ctx_columns;
  for (int i = 0; i < mb->dev.k; ++i) ib->match_slot[i] = mb->dev.m[i].slot;
  for (int c = 0; c < n_ctx_columns; ++c) ib->match_cols[c] = ctx_columns[c];
  mb->host = ib;
  return GMX_OK;
}

// ---- what the bank carries of ShortTermMemory ------------------------------------------------
static int match_read_states(gmx_match* mb, int stream, GmxMatchModelState* ms, GmxMatchStreamState* ss) {
  HIPCHK(hipSetDevice(mb->device));
  {
    int rcs = match_settle(mb);  // (no wave steps the stream, no learn is still noted)
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(mb->stream));
  const uint8_t* bank = mb->banks + (size_t)stream * mb->dev.bank_bytes;
  HIPCHK(hipMemcpy(ms, bank + mb->dev.mstate_off, GMX_MATCH_MAX_MODELS * sizeof(GmxMatchModelState),
                   hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ss, bank + mb->dev.sstate_off, sizeof(GmxMatchStreamState), hipMemcpyDeviceToHost));
  return GMX_OK;
}
static int match_write_states(gmx_match* mb, int stream, const GmxMatchModelState* ms, const GmxMatchStreamState* ss) {
  uint8_t* bank = mb->banks + (size_t)stream * mb->dev.bank_bytes;
  HIPCHK(hipMemcpy(bank + mb->dev.mstate_off, ms, GMX_MATCH_MAX_MODELS * sizeof(GmxMatchModelState),
                   hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(bank + mb->dev.sstate_off, ss, sizeof(GmxMatchStreamState), hipMemcpyHostToDevice));
  return GMX_OK;
}

extern "C" int gmx_match_slots_get(gmx_match* mb, int stream, float* values, int* new_bit) {
  if (!mb || stream < 0 || stream >= mb->S || (!values && !new_bit)) return GMX_ERR_INVALID;
  GmxMatchModelState ms[GMX_MATCH_MAX_MODELS];
  GmxMatchStreamState ss;
  int rc = match_read_states(mb, stream, ms, &ss);
  if (rc) return rc;
  if (values)
    for (int i = 0; i < mb->dev.k; ++i) values[i] = ms[i].slot_value;
  if (new_bit) *new_bit = (int)ss.new_bit;
  return GMX_OK;
}
extern "C" int gmx_match_slots_set(gmx_match* mb, int stream, const float* values, int new_bit) {
  if (!mb || stream < 0 || stream >= mb->S || !values || (new_bit != 0 && new_bit != 1)) return GMX_ERR_INVALID;
  GmxMatchModelState ms[GMX_MATCH_MAX_MODELS];
  GmxMatchStreamState ss;
  int rc = match_read_states(mb, stream, ms, &ss);
  if (rc) return rc;
  for (int i = 0; i < mb->dev.k; ++i) ms[i].slot_value = values[i];
  ss.new_bit = (uint32_t)new_bit;
  // A new blackboard: the bit a pending forward predicted was perceived without being learned (the reference's
  // generation loop, Perceive -> Predict with no Learn, tester.cpp:296-302), so the next forward is that bit's successor
  mb->fwd_done[stream] = 0;
  return match_write_states(mb, stream, ms, &ss);
}

extern "C" int gmx_match_history_size(gmx_match* mb, int stream, uint64_t* size) {
  if (!mb || stream < 0 || stream >= mb->S || !size) return GMX_ERR_INVALID;
  GmxMatchModelState ms[GMX_MATCH_MAX_MODELS];
  GmxMatchStreamState ss;
  int rc = match_read_states(mb, stream, ms, &ss);
  if (rc) return rc;
  *size = ss.hist_size;
  mb->hist_bound[stream] = ss.hist_size;
  return GMX_OK;
}

// ---- persistence: the match section of LongTermMemory (long-term-memory.cpp:70-106, :162-190) and
// Match::WriteToDisk / ReadFromDisk (match.cpp:111-123) ---------------------------------------------
static bool match_is_dense(uint32_t cnt, uint32_t size) { return !((double)cnt < (5.0 / 9.0) * (double)size); }

static int match_ckpt_ready(gmx_match* mb) {
  if (mb->chunks_d) return GMX_OK;
  const size_t n = mb->chunks.size();
  HIPCHK(hipMalloc((void**)&mb->chunks_d, n * sizeof(GmxMatchCkptChunk)));
  HIPCHK(hipMemcpy(mb->chunks_d, mb->chunks.data(), n * sizeof(GmxMatchCkptChunk), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc((void**)&mb->chunk_cnt_d, n * 4));
  HIPCHK(hipMalloc((void**)&mb->chunk_base_d, n * 4));
  HIPCHK(hipMalloc((void**)&mb->model_cnt_d, GMX_MATCH_MAX_MODELS * 4));
  HIPCHK(hipMalloc((void**)&mb->model_dense_d, GMX_MATCH_MAX_MODELS));
  HIPCHK(hipMalloc((void**)&mb->model_off_d, GMX_MATCH_MAX_MODELS * 8));
  return GMX_OK;
}

extern "C" int gmx_match_export(gmx_match* mb, int stream, void* long_buf, size_t* long_bytes, void* short_buf,
                                size_t* short_bytes) {
  if (!mb || stream < 0 || stream >= mb->S || !long_bytes || !short_bytes) return GMX_ERR_INVALID;
  const GmxMatchDev& d = mb->dev;
  const int K = d.k;
  GmxMatchModelState ms[GMX_MATCH_MAX_MODELS];
  GmxMatchStreamState ss;
  int rc = match_read_states(mb, stream, ms, &ss);  // (drains the bank's stream)
  if (rc) return rc;
  rc = match_ckpt_ready(mb);
  if (rc) return rc;
  uint8_t* const bank = mb->banks + (size_t)stream * d.bank_bytes;
  const size_t n_chunks = mb->chunks.size();
  GmxMatchCkptArgs a;
  memset(&a, 0, sizeof a);
  a.bank = bank;
  a.dev = mb->dev_d;
  a.chunks = mb->chunks_d;
  a.n_chunks = (uint32_t)n_chunks;
  a.chunk_cnt = mb->chunk_cnt_d;
  a.chunk_base = mb->chunk_base_d;
  a.model_cnt = mb->model_cnt_d;
  a.model_dense = mb->model_dense_d;
  a.model_off = mb->model_off_d;
  // count on the device, scan on the host
  HIPCHK(gmx_launch_match_ckpt_count(&a, mb->stream));
  std::vector<uint32_t> cc(n_chunks), base(n_chunks);
  HIPCHK(hipMemcpyAsync(cc.data(), mb->chunk_cnt_d, n_chunks * 4, hipMemcpyDeviceToHost, mb->stream));
  HIPCHK(hipStreamSynchronize(mb->stream));
  uint32_t cnt[GMX_MATCH_MAX_MODELS] = {};
  uint8_t dense[GMX_MATCH_MAX_MODELS] = {};
  uint64_t moff[GMX_MATCH_MAX_MODELS] = {}, body[GMX_MATCH_MAX_MODELS] = {};
  for (size_t c = 0; c < n_chunks; ++c) {
    base[c] = cnt[mb->chunks[c].model];
    cnt[mb->chunks[c].model] += cc[c];
  }
  uint64_t packed = 0;
  size_t need = 8 + (size_t)ss.hist_size;
  for (int i = 0; i < K; ++i) {
    dense[i] = match_is_dense(cnt[i], d.m[i].table_size) ? 1 : 0;
    body[i] = dense[i] ? 5ull * d.m[i].table_size : 9ull * cnt[i];
    moff[i] = packed;
    packed += body[i];
    need += 4 + body[i] + 2048;
  }
  const size_t need_short = 11 * (size_t)K;
  const bool sizing = !long_buf && !short_buf;
  const bool fits = (!long_buf || *long_bytes >= need) && (!short_buf || *short_bytes >= need_short);
  *long_bytes = need;
  *short_bytes = need_short;
  if (sizing) return GMX_OK;
  if (!fits) return GMX_ERR_INVALID;
  if (short_buf) {
    uint8_t* o = (uint8_t*)short_buf;
    for (int i = 0; i < K; ++i) {
      const uint64_t cm = ms[i].cur_match;
      memcpy(o, &cm, 8);
      o[8] = ms[i].cur_byte;
      o[9] = ms[i].bit_pos;
      o[10] = ms[i].match_length;
      o += 11;
    }
  }
  if (!long_buf) return GMX_OK;
  // pack on the device: the host reads only what it writes out
  uint8_t* pk = nullptr;
  if (packed) {
    hipError_t e = hipMalloc((void**)&pk, packed);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? GMX_ERR_NOMEM : hip_fail(e, "hipMalloc(packed)");
  }
  a.buf = pk;
  int ret = GMX_OK;
#define XCHK(call)                        \
  do {                                    \
    hipError_t e_ = (call);               \
    if (e_ != hipSuccess) {               \
      ret = hip_fail(e_, #call);          \
      goto out;                           \
    }                                     \
  } while (0)
  {
    uint8_t* o = (uint8_t*)long_buf;
    if (packed) {
      XCHK(hipMemcpyAsync(mb->chunk_base_d, base.data(), n_chunks * 4, hipMemcpyHostToDevice, mb->stream));
      XCHK(hipMemcpyAsync(mb->model_cnt_d, cnt, sizeof cnt, hipMemcpyHostToDevice, mb->stream));
      XCHK(hipMemcpyAsync(mb->model_dense_d, dense, sizeof dense, hipMemcpyHostToDevice, mb->stream));
      XCHK(hipMemcpyAsync(mb->model_off_d, moff, sizeof moff, hipMemcpyHostToDevice, mb->stream));
      XCHK(gmx_launch_match_ckpt_pack(&a, mb->stream));
      XCHK(hipStreamSynchronize(mb->stream));
    }
    const uint64_t hs = ss.hist_size;
    memcpy(o, &hs, 8);
    o += 8;
    if (hs) XCHK(hipMemcpy(o, mb->hist + (size_t)stream * d.hist_cap, (size_t)hs, hipMemcpyDeviceToHost));
    o += hs;
    for (int i = 0; i < K; ++i) {
      memcpy(o, &cnt[i], 4);
      o += 4;
      if (body[i]) XCHK(hipMemcpy(o, pk + moff[i], (size_t)body[i], hipMemcpyDeviceToHost));
      o += body[i];
      XCHK(hipMemcpy(o, bank + d.pred_off + 1024ull * i, 1024, hipMemcpyDeviceToHost));
      o += 1024;
      XCHK(hipMemcpy(o, bank + d.cnt_off + 1024ull * i, 1024, hipMemcpyDeviceToHost));
      o += 1024;
    }
  }
out:
#undef XCHK
  if (pk) (void)hipFree(pk);
  mb->hist_bound[stream] = ss.hist_size;
  return ret;
}

// What gmx_match_import and gmx_match_group_import demand of one stream's two sections, and where its parts lie.
struct GmxMatchSection {
  uint64_t hs = 0;                               // history size
  const uint8_t* hist_src = nullptr;
  uint32_t cnt[GMX_MATCH_MAX_MODELS] = {};
  uint8_t dense[GMX_MATCH_MAX_MODELS] = {};
  uint64_t moff[GMX_MATCH_MAX_MODELS] = {};      // byte offset of a model's body (behind its count) in the section
  const uint8_t* tail[GMX_MATCH_MAX_MODELS] = {};
  uint64_t cms[GMX_MATCH_MAX_MODELS] = {};       // cur_match_ of the short section
};
static int match_validate_section(const GmxMatchDev& d, const uint8_t* lb, size_t long_bytes, const uint8_t* sb,
                                  size_t short_bytes, GmxMatchSection* out) {
  const int K = d.k;
  if (short_bytes != 11 * (size_t)K) return GMX_ERR_FORMAT;
  const uint8_t* p = lb;
  const uint8_t* const end = p + long_bytes;
  if (end - p < 8) return GMX_ERR_FORMAT;
  uint64_t hs;
  memcpy(&hs, p, 8);
  p += 8;
  if (hs > d.hist_cap || (uint64_t)(end - p) < hs) return GMX_ERR_FORMAT;
  out->hs = hs;
  out->hist_src = p;
  p += hs;
  uint32_t* const cnt = out->cnt;
  uint8_t* const dense = out->dense;
  for (int i = 0; i < K; ++i) {
    const uint32_t size = d.m[i].table_size;
    if (end - p < 4) return GMX_ERR_FORMAT;
    memcpy(&cnt[i], p, 4);
    p += 4;
    if (cnt[i] > size) return GMX_ERR_FORMAT;
    dense[i] = match_is_dense(cnt[i], size) ? 1 : 0;
    out->moff[i] = (uint64_t)(p - lb);
    if (!dense[i]) {
      if ((uint64_t)(end - p) < 9ull * cnt[i]) return GMX_ERR_FORMAT;
      uint32_t prev = 0;
      for (uint32_t c = 0; c < cnt[i]; ++c, p += 9) {
        uint32_t key, ptr;
        memcpy(&key, p, 4);
        memcpy(&ptr, p + 4, 4);
        if (key >= size || (c > 0 && key <= prev)) return GMX_ERR_FORMAT;  // ascending, below the table size
        if (p[8] != 0 || ptr == 0 || ptr >= hs) return GMX_ERR_FORMAT;     // a valid pointer into the history
        prev = key;
      }
    } else {
      if ((uint64_t)(end - p) < 5ull * size) return GMX_ERR_FORMAT;
      uint32_t valid = 0;
      for (uint32_t e = 0; e < size; ++e, p += 5) {
        uint32_t ptr;
        memcpy(&ptr, p, 4);
        if (p[4] != 0 || (ptr != 0 && ptr >= hs)) return GMX_ERR_FORMAT;
        valid += ptr != 0;
      }
      if (valid != cnt[i]) return GMX_ERR_FORMAT;  // the branch follows from the count
    }
    if (end - p < 2048) return GMX_ERR_FORMAT;
    out->tail[i] = p;
    p += 2048;
  }
  if (p != end) return GMX_ERR_FORMAT;
  for (int i = 0; i < K; ++i, sb += 11) {
    memcpy(&out->cms[i], sb, 8);
    const uint8_t bp = sb[9];
    if ((bp & (bp - 1)) != 0) return GMX_ERR_FORMAT;                    // bit_pos_: 0 or a power of two
    if (out->cms[i] != 0 && out->cms[i] >= hs) return GMX_ERR_FORMAT;   // cur_match_ inside the history
  }
  return GMX_OK;
}

extern "C" int gmx_match_import(gmx_match* mb, int stream, const void* long_buf, size_t long_bytes,
                                const void* short_buf, size_t short_bytes) {
  if (!mb || stream < 0 || stream >= mb->S || !long_buf || !short_buf) return GMX_ERR_INVALID;
  const GmxMatchDev& d = mb->dev;
  const int K = d.k;
  // ---- validate everything before the bank is touched
  const uint8_t* const lb = (const uint8_t*)long_buf;
  GmxMatchSection sec;
  {
    int rcv = match_validate_section(d, lb, long_bytes, (const uint8_t*)short_buf, short_bytes, &sec);
    if (rcv) return rcv;
  }
  const uint64_t hs = sec.hs;
  const uint8_t* const hist_src = sec.hist_src;
  const uint32_t* const cnt = sec.cnt;
  const uint8_t* const dense = sec.dense;
  const uint64_t* const moff = sec.moff;
  const uint8_t* const* const tail = sec.tail;
  const uint64_t* const cms = sec.cms;
  GmxMatchModelState ms[GMX_MATCH_MAX_MODELS];
  GmxMatchStreamState ss;
  // ---- the bank
  int rc = match_read_states(mb, stream, ms, &ss);  // (drains the bank's stream; keeps slot values and new_bit)
  if (rc) return rc;
  rc = match_ckpt_ready(mb);
  if (rc) return rc;
  const uint8_t* sp = (const uint8_t*)short_buf;
  for (int i = 0; i < K; ++i, sp += 11) {
    ms[i].cur_match = (uint32_t)cms[i];
    ms[i].cur_byte = sp[8];
    ms[i].bit_pos = sp[9];
    ms[i].match_length = sp[10];
  }
  ss.hist_size = (uint32_t)hs;
  uint8_t* const bank = mb->banks + (size_t)stream * d.bank_bytes;
  uint8_t* staged = nullptr;
  {
    hipError_t e = hipMalloc((void**)&staged, long_bytes);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? GMX_ERR_NOMEM : hip_fail(e, "hipMalloc(section)");
  }
  int ret = GMX_OK;
#define XCHK(call)                        \
  do {                                    \
    hipError_t e_ = (call);               \
    if (e_ != hipSuccess) {               \
      ret = hip_fail(e_, #call);          \
      goto out;                           \
    }                                     \
  } while (0)
  {
    GmxMatchCkptArgs a;
    memset(&a, 0, sizeof a);
    a.bank = bank;
    a.dev = mb->dev_d;
    a.model_cnt = mb->model_cnt_d;
    a.model_dense = mb->model_dense_d;
    a.model_off = mb->model_off_d;
    a.buf = staged;
    XCHK(hipMemcpyAsync(staged, lb, long_bytes, hipMemcpyHostToDevice, mb->stream));
    XCHK(hipMemcpyAsync(mb->model_cnt_d, cnt, sizeof sec.cnt, hipMemcpyHostToDevice, mb->stream));
    XCHK(hipMemcpyAsync(mb->model_dense_d, dense, sizeof sec.dense, hipMemcpyHostToDevice, mb->stream));
    XCHK(hipMemcpyAsync(mb->model_off_d, moff, sizeof sec.moff, hipMemcpyHostToDevice, mb->stream));
    XCHK(hipMemsetAsync(bank, 0, (size_t)d.tab_bytes, mb->stream));
    XCHK(gmx_launch_match_ckpt_scatter(&a, K, 256, mb->stream));
    if (hs)
      XCHK(hipMemcpyAsync(mb->hist + (size_t)stream * d.hist_cap, hist_src, (size_t)hs, hipMemcpyHostToDevice,
                          mb->stream));
    for (int i = 0; i < K; ++i) {
      XCHK(hipMemcpyAsync(bank + d.pred_off + 1024ull * i, tail[i], 1024, hipMemcpyHostToDevice, mb->stream));
      XCHK(hipMemcpyAsync(bank + d.cnt_off + 1024ull * i, tail[i] + 1024, 1024, hipMemcpyHostToDevice, mb->stream));
    }
    XCHK(hipStreamSynchronize(mb->stream));
  }
out:
#undef XCHK
  (void)hipFree(staged);
  if (ret) return ret;
  rc = match_write_states(mb, stream, ms, &ss);
  if (rc) return rc;
  mb->hist_bound[stream] = hs;
  mb->fwd_done[stream] = 0;
  return GMX_OK;
}

// Match::Copy x K (match.cpp:125-131) and LongTermMemory::Copy's history and match_memory; the slot values and
// new_bit travel too (ShortTermMemory::Copy copies them in the reference).
extern "C" int gmx_match_copy(gmx_match* dst, int dst_stream, gmx_match* src, int src_stream) {
  if (!dst || !src || dst_stream < 0 || dst_stream >= dst->S || src_stream < 0 || src_stream >= src->S)
    return GMX_ERR_INVALID;
  // the same models on the same device (Predictor::Copy copies between two Predictors of one program)
  if (dst->device != src->device || dst->dev.k != src->dev.k || dst->dev.bank_bytes != src->dev.bank_bytes)
    return GMX_ERR_INVALID;
  for (int i = 0; i < dst->dev.k; ++i)
    if (dst->dev.m[i].table_size != src->dev.m[i].table_size || dst->dev.m[i].limit != src->dev.m[i].limit ||
        dst->dev.m[i].slot != src->dev.m[i].slot)
      return GMX_ERR_INVALID;
  if (dst == src && dst_stream == src_stream) return GMX_OK;
  HIPCHK(hipSetDevice(src->device));
  {
    int rcs = match_settle(src);
    if (!rcs && dst != src) rcs = match_settle(dst);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(src->stream));
  GmxMatchStreamState ss;
  HIPCHK(hipMemcpy(&ss, src->banks + (size_t)src_stream * src->dev.bank_bytes + src->dev.sstate_off, sizeof ss,
                   hipMemcpyDeviceToHost));
  if (ss.hist_size > dst->dev.hist_cap) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(dst->device));
  HIPCHK(hipStreamSynchronize(dst->stream));
  HIPCHK(hipMemcpy(dst->banks + (size_t)dst_stream * dst->dev.bank_bytes,
                   src->banks + (size_t)src_stream * src->dev.bank_bytes, dst->dev.bank_bytes,
                   hipMemcpyDeviceToDevice));
  if (ss.hist_size)
    HIPCHK(hipMemcpy(dst->hist + (size_t)dst_stream * dst->dev.hist_cap,
                     src->hist + (size_t)src_stream * src->dev.hist_cap, ss.hist_size, hipMemcpyDeviceToDevice));
  dst->hist_bound[dst_stream] = ss.hist_size;
  dst->fwd_done[dst_stream] = 0;
  return GMX_OK;
}

// Match::GetMemoryUsage (match.cpp:133-141): a constant of the table size.
extern "C" int gmx_match_memory_usage(gmx_match* mb, int model, uint64_t* bytes) {
  if (!mb || model < 0 || model >= mb->dev.k || !bytes) return GMX_ERR_INVALID;
  *bytes = 27ull + 256 * 4 * 2 + 5ull * mb->dev.m[model].table_size;
  return GMX_OK;
}
