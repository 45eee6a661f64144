// gmx_ctx.inc -- host side of the context banks (included by gmx_capi.cpp).
//
// Replaces, for S independent streams, what the reference computes per bit on the host between the coder and the
// models: the context fields of BasicContexts (basic-contexts.cpp:5-40), the nine IntervalContext, nineteen SkipContext
// and nine IndirectHash objects of predictor.cpp:54-76, :78-185, :210-249.  Compute is gmx_ctx.hip; nothing here falls
// back to the CPU.

struct gmx_ctx_batch : GmxBatchCore {
  gmx_ctx* cb = nullptr;
  uint64_t& max_bits = max_rows;
  uint64_t max_fires = 0;
  unsigned flags = 0;
  uint8_t* d_bits = nullptr;
  uint32_t* d_values = nullptr;   // only with GMX_CTX_BATCH_VALUES
  uint32_t* d_scratch = nullptr;  // [S][max_fires][H]
  uint8_t* h_bits = nullptr;
  uint32_t* h_values = nullptr;
};

struct gmx_ctx {
  int device = 0, S = 0;
  GmxCtxDev dev;                 // host copy
  GmxCtxDev* dev_d = nullptr;
  uint8_t* banks = nullptr;      // [S][bank_bytes]
  hipStream_t stream = nullptr;  // kernels AND the batches' transfers, as for the Match banks: the fourth stream of
                                 // the mixers' priority level (the group's own and its two transfer streams, §4.10)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_mark[2] = {};    // a timed run: behind the chain kernel, behind the expand kernel
  float last_ms[3] = {};         // ... and what its three kernels took (gmx_ctx_last_kernel_ms)
  GmxBatchBank bb;               // its batches
  GmxCountList counts;
  // checkpoint: the chunk list (the same for every stream) and its device arrays, lazily
  std::vector<GmxCtxCkptChunk> chunks;
  GmxCtxCkptChunk* chunks_d = nullptr;
  uint32_t* chunk_cnt_d = nullptr;
  uint32_t* chunk_base_d = nullptr;
  uint8_t* hash_dense_d = nullptr;
  uint32_t* hash_cnt_d = nullptr;
  uint64_t* hash_off_d = nullptr;
  // gmx_chainstep_attach_ctx: the lock-step object whose steps run this bank (the two register with each other, like a
  // Match bank and its lock-step objects), and per stream "a Predict of a step waits for its Learn": until then the
  // board's new_bit means nothing, and neither a run nor a reader of the board may take it for a coded bit
  gmx_chainstep* chainstep = nullptr;
  bool moved = false;  // a gmx_ctx_* call may have moved a stream within its byte: the object reads the boards again
  std::vector<uint8_t> outstanding;
  struct GmxCtxGckState* gck = nullptr;  // the group checkpoint's staging, lazily (gmx_ctx_ckpt.inc)
  int gck_ops = 0;                       // round trips of the newest group call (gmx_debug_ctx_group_ops)
  // The per-bit surface (gmx_ctx_forward / gmx_ctx_learn).  A learn is only noted (1 + bit) and travels with the
  // stream's next forward -- a launch, or a command of the session wave the stream rides in; `outstanding` above is
  // "a forward waits for its learn" here as well.
  std::vector<uint8_t> noted;
  int n_noted = 0;
  GmxCtxBitReply* bit_reply = nullptr;   // pinned, lazily
  int bit_launches = 0;                  // launches of gmx_ctx_bit_kernel so far (gmx_debug_ctx_bit_launches)
  // gmx_indirect_attach_ctx: the streams step at the head of a chained forward in the session waves of `host`.
  // wave_fresh[s]: the register copy of stream s's wave, if one runs, is what the board holds -- nothing but that
  // wave has moved the stream since; otherwise its next command says GMX_CTX_WAVE_RELOAD.
  gmx_indirect* host = nullptr;
  int32_t* routes_d = nullptr;
  int32_t routes[GMX_CTX_WAVE_ROUTE_WORDS] = {};
  bool own_ind = false, own_match = false;  // a column of the Indirect / Match records is the caller's (routed -1)
  std::vector<uint8_t> wave_fresh;
};
static void ctx_gck_free(gmx_ctx* cb);  // gmx_ctx_ckpt.inc
static void chainstep_ctx_gone(gmx_chainstep* cs);  // gmx_chainstep.inc
static int chainstep_settle(gmx_chainstep* cs);     // ... no step of it is in flight any more
static int ctx_flush_noted(gmx_ctx* cb, int s);

// Before a gmx_ctx_* call reads or writes the bank through anything but the per-bit surface: the steps of a lock-step
// object it is attached to run on the group's stream; the session waves it rides in stop (they keep nothing of a
// stream's state, so there is nothing to write back), and every noted learn is run.
static int ctx_settle(gmx_ctx* cb) {
  int first = cb->chainstep ? chainstep_settle(cb->chainstep) : GMX_OK;
  if (cb->host) {
    const int rc = ind_sessions_close(cb->host);
    if (rc && !first) first = rc;
    std::fill(cb->wave_fresh.begin(), cb->wave_fresh.end(), 0);
  }
  for (int s = 0; s < cb->S && cb->n_noted > 0; ++s) {
    const int rc = ctx_flush_noted(cb, s);
    if (rc && !first) first = rc;
  }
  return first;
}

// Before stream s's board is moved by anything but a command of the wave the stream rides in (s < 0: every stream): see
// ind_ctx_board_moves.  An Indirect forward that took its indices from the board is learned now if its learn is noted,
// and void otherwise.
static int ctx_board_moves(gmx_ctx* cb, int s) { return cb->host ? ind_ctx_board_moves(cb->host, s) : GMX_OK; }

extern "C" {
hipError_t gmx_launch_ctx_bit(const GmxCtxDev* dv, const GmxCtxBitArgs* args, hipStream_t stream);
hipError_t gmx_launch_ctx_run(const GmxCtxDev* dv, int n_hash, const GmxCtxRunArgs* args, hipStream_t stream,
                              hipEvent_t* marks);
hipError_t gmx_launch_ctx_init(const GmxCtxDev* dv, uint8_t* banks, int n_streams, hipStream_t stream);
hipError_t gmx_launch_ctx_heads(const GmxCtxDev* dv, const uint8_t* banks, int n_streams, uint32_t* out,
                                 hipStream_t stream);
hipError_t gmx_launch_ctx_step(const GmxCtxDev* dv, const GmxCtxStepArgs* args, hipStream_t stream);
hipError_t gmx_launch_ctx_ckpt_count(const GmxCtxCkptArgs* a, hipStream_t stream);
hipError_t gmx_launch_ctx_ckpt_pack(const GmxCtxCkptArgs* a, hipStream_t stream);
hipError_t gmx_launch_ctx_ckpt_scatter(const GmxCtxCkptArgs* a, int n_hash, hipStream_t stream);
}

static void ctx_batch_free(gmx_ctx_batch* b) {
  if (!b) return;
  batch_core_free(*b);
  delete b;
}

extern "C" void gmx_ctx_destroy(gmx_ctx* cb) {
  if (!cb) return;
  (void)hipSetDevice(cb->device);
  if (cb->chainstep) chainstep_ctx_gone(cb->chainstep);  // (its later steps fail; none is in flight any more)
  cb->chainstep = nullptr;
  if (cb->host) (void)ctx_host_detach(cb);  // (the waves stop: none of them holds this bank any more)
  if (cb->stream) (void)hipStreamSynchronize(cb->stream);
  if (cb->routes_d) (void)hipFree(cb->routes_d);
  if (cb->bit_reply) (void)hipHostFree(cb->bit_reply);
  batch_bank_detach_all(cb->bb);  // shells, as for gmx_batch
  void* dv[] = {cb->banks, cb->dev_d, cb->chunks_d, cb->chunk_cnt_d, cb->chunk_base_d, cb->hash_dense_d,
                cb->hash_cnt_d, cb->hash_off_d};
  for (void* p : dv)
    if (p) (void)hipFree(p);
  if (cb->ev0) (void)hipEventDestroy(cb->ev0);
  if (cb->ev1) (void)hipEventDestroy(cb->ev1);
  for (hipEvent_t e : cb->ev_mark)
    if (e) (void)hipEventDestroy(e);
  count_list_free(cb->counts);
  ctx_gck_free(cb);
  if (cb->stream) (void)hipStreamDestroy(cb->stream);
  delete cb;
}

extern "C" int gmx_ctx_reset(gmx_ctx* cb) {
  if (!cb) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(cb->device));
  {
    int rcs = ctx_board_moves(cb, -1);
    if (!rcs) rcs = ctx_settle(cb);
    if (rcs) return rcs;
  }
  std::fill(cb->outstanding.begin(), cb->outstanding.end(), 0);
  std::fill(cb->noted.begin(), cb->noted.end(), 0);
  cb->n_noted = 0;
  cb->moved = true;
  HIPCHK(hipMemsetAsync(cb->banks, 0, (size_t)cb->S * cb->dev.bank_bytes, cb->stream));
  HIPCHK(gmx_launch_ctx_init(cb->dev_d, cb->banks, cb->S, cb->stream));
  HIPCHK(hipStreamSynchronize(cb->stream));
  return GMX_OK;
}

// The descriptor list -> the device description; GMX_ERR_INVALID for anything outside the documented ranges.
static int ctx_describe(const gmx_ctx_desc* descs, int n_vars, GmxCtxDev* out) {
  GmxCtxDev& d = *out;
  memset(&d, 0, sizeof d);
  d.v = n_vars;
  uint64_t off = 0;
  int n_maps = 0;
  for (int i = 0; i < n_vars; ++i) {
    const gmx_ctx_desc& c = descs[i];
    GmxCtxVarDev& v = d.var[i];
    v.kind = c.kind;
    switch (c.kind) {
      case GMX_CTX_ZERO:
      case GMX_CTX_BIT_CONTEXT:
        break;
      case GMX_CTX_RECENT_BYTE:
      case GMX_CTX_BYTE_PLUS_RECENT:
        if (c.index < 0 || c.index > 9) return GMX_ERR_INVALID;
        v.index = c.index;
        break;
      case GMX_CTX_INTERVAL: {
        if (c.num_bits < 1 || c.num_bits > 31) return GMX_ERR_INVALID;
        int max_value = 0;
        for (int k = 0; k < 256; ++k) max_value = std::max(max_value, (int)c.map[k]);
        int shift = 1;
        while ((1 << shift) <= max_value) ++shift;  // interval-context.cpp:12-13
        v.num_bits = c.num_bits;
        v.shift = shift;
        v.index = n_maps;
        memcpy(d.maps[n_maps++], c.map, 256);
        break;
      }
      case GMX_CTX_SKIP:
        if (c.n_bytes < 1 || c.n_bytes > 8) return GMX_ERR_INVALID;
        for (int k = 0; k < c.n_bytes; ++k) {
          if (c.bytes_to_use[k] > 15) return GMX_ERR_INVALID;
          v.bytes_to_use[k] = c.bytes_to_use[k];
        }
        v.n_bytes = c.n_bytes;
        break;
      case GMX_CTX_INDIRECT_HASH: {
        if (c.outer_order < 1 || c.outer_order > 4 || c.inner_order < 1 || c.inner_order > 4 || c.table_size == 0 ||
            d.h >= GMX_CTX_MAX_HASH)
          return GMX_ERR_INVALID;
        GmxCtxHashDev& h = d.hash[d.h];
        h.tab_off = off;
        h.table_size = c.table_size;
        h.outer_mask = (1u << (8 * (c.outer_order - 1))) - 1u;
        h.inner_mask = (1u << (8 * (c.inner_order - 1))) - 1u;
        h.var = i;
        v.index = d.h++;
        off += round_up64(4ull * c.table_size, 256);
        break;
      }
      default:
        return GMX_ERR_INVALID;
    }
  }
  d.tab_bytes = off;
  d.hstate_off = off;
  off += GMX_CTX_MAX_HASH * sizeof(GmxCtxHashState);
  d.board_off = off;
  off += sizeof(GmxCtxBoard);
  d.bank_bytes = round_up64(off, 256);
  return GMX_OK;
}

extern "C" int gmx_ctx_create(gmx_ctx** out, const gmx_ctx_desc* descs, int n_vars, int n_streams, int device) {
  if (!out) return GMX_ERR_INVALID;
  *out = nullptr;
  if (!descs || n_vars < 1 || n_vars > GMX_CTX_MAX_VARS || n_streams < 1) return GMX_ERR_INVALID;
  gmx_ctx* cb = new (std::nothrow) gmx_ctx();
  if (!cb) return GMX_ERR_NOMEM;
  int rc = ctx_describe(descs, n_vars, &cb->dev);
  if (rc) {
    delete cb;
    return rc;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    delete cb;
    return GMX_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) {
    delete cb;
    return GMX_ERR_INVALID;
  }
  cb->device = device;
  batch_bank_init(cb->bb, cb, device, &cb->stream);  // (no transfer streams: see the comment at gmx_ctx::stream)
  cb->S = n_streams;
  cb->outstanding.assign((size_t)n_streams, 0);
  cb->noted.assign((size_t)n_streams, 0);
  cb->wave_fresh.assign((size_t)n_streams, 0);
  const GmxCtxDev& d = cb->dev;
  for (int i = 0; i < d.h; ++i)
    for (uint32_t e = 0; e < d.hash[i].table_size; e += GMX_CTX_CKPT_CHUNK) {
      cb->chunks.push_back(GmxCtxCkptChunk{(uint32_t)i, e});
      if (d.hash[i].table_size - e <= (uint32_t)GMX_CTX_CKPT_CHUNK) break;  // (no wrap for sizes near 2^32)
    }
  {
    hipError_t e0 = hipSetDevice(device);
    if (e0 != hipSuccess) {
      delete cb;
      return hip_fail(e0, "hipSetDevice");
    }
  }
#define CCHK(call)                                           \
  do {                                                       \
    hipError_t e_ = (call);                                  \
    if (e_ != hipSuccess) {                                  \
      int r_ = hip_fail(e_, #call);                          \
      gmx_ctx_destroy(cb);                                   \
      return e_ == hipErrorOutOfMemory ? GMX_ERR_NOMEM : r_; \
    }                                                        \
  } while (0)
  CCHK(bank_stream_create(&cb->stream, 0));
  CCHK(hipEventCreate(&cb->ev0));
  CCHK(hipEventCreate(&cb->ev1));
  CCHK(hipEventCreate(&cb->ev_mark[0]));
  CCHK(hipEventCreate(&cb->ev_mark[1]));
  CCHK(hipMalloc((void**)&cb->dev_d, sizeof(GmxCtxDev)));
  CCHK(hipMemcpy(cb->dev_d, &cb->dev, sizeof(GmxCtxDev), hipMemcpyHostToDevice));
  CCHK(hipMalloc((void**)&cb->banks, (size_t)n_streams * d.bank_bytes));
#undef CCHK
  rc = gmx_ctx_reset(cb);
  if (rc) {
    gmx_ctx_destroy(cb);
    return rc;
  }
  *out = cb;
  return GMX_OK;
}

extern "C" int gmx_ctx_n_streams(const gmx_ctx* cb) { return cb ? cb->S : GMX_ERR_INVALID; }
extern "C" int gmx_ctx_n_vars(const gmx_ctx* cb) { return cb ? cb->dev.v : GMX_ERR_INVALID; }
extern "C" uint64_t gmx_ctx_bank_bytes(const gmx_ctx* cb) { return cb ? cb->dev.bank_bytes : 0; }
extern "C" int gmx_ctx_sync(gmx_ctx* cb) {
  if (!cb) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(cb->device));
  HIPCHK(hipStreamSynchronize(cb->stream));
  return GMX_OK;
}
extern "C" int gmx_ctx_set_cu_mask(gmx_ctx* cb, const uint32_t* mask, int n_words) {
  if (!cb || n_words < 0 || (n_words > 0 && !mask)) return GMX_ERR_INVALID;
  if (cb->chainstep) return GMX_ERR_STATE;  // (its captured steps order themselves against the stream there is)
  HIPCHK(hipSetDevice(cb->device));
  return stream_with_cu_mask(&cb->stream, mask, n_words);
}

// ---- batches -----------------------------------------------------------------------------------
static int ctx_batch_alloc(gmx_ctx_batch* b, gmx_ctx* cb, uint64_t max_bits) {
  int rc = batch_core_alloc(*b, &cb->bb, cb->S, max_bits, true);  // (the pinned arrays too: the accessors never allocate)
  if (rc) return rc;
  if (cb->dev.h) BCHK(hipMalloc((void**)&b->d_scratch, (size_t)cb->S * b->max_fires * (size_t)cb->dev.h * 4));
  return GMX_OK;
}
extern "C" int gmx_ctx_batch_create(gmx_ctx_batch** out, gmx_ctx* cb, uint64_t max_bits, unsigned flags) {
  if (!out) return GMX_ERR_INVALID;
  *out = nullptr;
  if (!cb || max_bits == 0 || max_bits > (1ull << 30) || (flags & ~GMX_CTX_BATCH_VALUES)) return GMX_ERR_INVALID;
  gmx_ctx_batch* b = new (std::nothrow) gmx_ctx_batch();
  if (!b) return GMX_ERR_NOMEM;
  b->back = (void**)&b->cb;
  b->max_fires = max_bits / 8 + 2;  // byte openings of a run: at most (8 + n - 1) / 8 + 1
  b->flags = flags;
  gmx_ctx_batch_cols(b->cols, b, cb->dev.v, flags);
  int rc = ctx_batch_alloc(b, cb, max_bits);
  if (rc) {
    ctx_batch_free(b);
    return rc;
  }
  *out = b;
  return GMX_OK;
}
extern "C" void gmx_ctx_batch_destroy(gmx_ctx_batch* b) { ctx_batch_free(b); }
extern "C" uint64_t gmx_ctx_batch_max_bits(const gmx_ctx_batch* b) { return b ? b->max_bits : 0; }
extern "C" uint8_t* gmx_ctx_batch_bits(gmx_ctx_batch* b) { return (b && b->cb) ? b->h_bits : nullptr; }
extern "C" const uint32_t* gmx_ctx_batch_values(gmx_ctx_batch* b) { return (b && b->cb) ? b->h_values : nullptr; }

// (on the bank's own stream, as for the Match banks)
extern "C" int gmx_ctx_batch_upload(gmx_ctx_batch* b, uint64_t n_bits) { return batch_core_transfer(b, n_bits, GMX_COL_UP); }
extern "C" int gmx_ctx_batch_download(gmx_ctx_batch* b, uint64_t n_bits) {
  if (b && !(b->flags & GMX_CTX_BATCH_VALUES)) return GMX_ERR_INVALID;  // (there is nothing to fetch)
  return batch_core_transfer(b, n_bits, GMX_COL_DOWN);
}
extern "C" int gmx_ctx_batch_wait(gmx_ctx_batch* b) { return batch_core_wait(b); }

// ---- compute -----------------------------------------------------------------------------------
static int ctx_route_ok(const gmx_ctx* cb, const int32_t* route, int n, int want) {
  if (!route || n != want || n < 1 || n > GMX_CTX_MAX_ROUTE) return GMX_ERR_INVALID;
  for (int i = 0; i < n; ++i)
    if (route[i] < -1 || route[i] >= cb->dev.v) return GMX_ERR_INVALID;
  return GMX_OK;
}
// Everything a run demands of its targets, for the largest bit count of the launch.
static int ctx_targets_ok(const gmx_ctx* cb, const gmx_ctx_targets* t, uint64_t n_bits) {
  if (!t) return GMX_OK;
  if (t->mixers) {
    const gmx_batch* m = t->mixers;
    if (!m->g || m->S != cb->S || m->g->device != cb->device || n_bits > m->max_bits) return GMX_ERR_INVALID;
    if (ctx_route_ok(cb, t->mixer_route, t->n_mixer_route, m->g->topo.m)) return GMX_ERR_INVALID;
  }
  if (t->indirect) {
    const gmx_ind_batch* ib = t->indirect;
    if (!ib->ib || ib->S != cb->S || ib->ib->device != cb->device || n_bits > ib->max_bits) return GMX_ERR_INVALID;
    if (ctx_route_ok(cb, t->ind_route, t->n_ind_route, ib->ib->dev.k)) return GMX_ERR_INVALID;
  }
  if (t->match) {
    const gmx_match_batch* mb = t->match;
    if (!mb->mb || mb->S != cb->S || mb->mb->device != cb->device || n_bits > mb->max_bits) return GMX_ERR_INVALID;
    if (ctx_route_ok(cb, t->match_route, t->n_match_route, mb->mb->dev.k)) return GMX_ERR_INVALID;
  }
  return GMX_OK;
}

static int ctx_launch(gmx_ctx* cb, gmx_ctx_batch* b, uint64_t T, const uint64_t* n_list,
                      const gmx_ctx_targets* t, float* kernel_ms) {
  if (T == 0) return GMX_OK;
  GmxCtxRunArgs a;
  memset(&a, 0, sizeof a);
  a.banks = cb->banks;
  a.bits = b->d_bits;
  a.values = b->d_values;
  a.scratch = b->d_scratch;
  a.rec_stride = b->max_bits;
  a.max_fires = b->max_fires;
  a.T = T;
  a.n_streams = cb->S;
  if (n_list) {
    int rcl = count_list_stage(cb->counts, n_list, cb->S, cb->stream, &a.T_list);
    if (rcl) return rcl;
  }
  hipStream_t st = cb->stream;
  if (t && t->mixers) {
    gmx_batch* m = t->mixers;
    a.tg[0].ctx = m->d_ctx;
    a.tg[0].stride = m->max_bits;
    a.tg[0].n_cols = t->n_mixer_route;
    memcpy(a.tg[0].route, t->mixer_route, 4 * (size_t)t->n_mixer_route);
    int rcw = xfer_writer_waits(m->x, st);
    if (rcw) return rcw;
  }
  if (t && t->indirect) {
    gmx_ind_batch* ib = t->indirect;
    a.tg[1].ctx = ib->d_ctx;
    a.tg[1].bc = ib->d_bc;
    a.tg[1].bits = ib->d_bits;
    a.tg[1].stride = ib->max_bits;
    a.tg[1].n_cols = t->n_ind_route;
    memcpy(a.tg[1].route, t->ind_route, 4 * (size_t)t->n_ind_route);
    int rcw = xfer_writer_waits(ib->x, st);
    if (rcw) return rcw;
  }
  if (t && t->match) {
    // A Match batch's transfers and kernels share the Match bank's stream (gmx_match_batch_upload): its upload mark
    // and its last device-side use are events of that stream, and the marks below make that stream wait for this
    // writer -- the same hand-shake as for the two other targets, and nothing of what the Match calls do changes
    gmx_match_batch* mb = t->match;
    a.tg[2].ctx = mb->d_ctx;
    a.tg[2].bc = mb->d_bc;
    a.tg[2].bits = mb->d_bits;
    a.tg[2].stride = mb->max_bits;
    a.tg[2].n_cols = t->n_match_route;
    memcpy(a.tg[2].route, t->match_route, 4 * (size_t)t->n_match_route);
    int rcw = xfer_writer_waits(mb->x, st);
    if (rcw) return rcw;
  }
  {
    int rcx = xfer_before_run(b->x, st);
    if (rcx) return rcx;
  }
  if (kernel_ms) HIPCHK(hipEventRecord(cb->ev0, st));
  HIPCHK(gmx_launch_ctx_run(cb->dev_d, cb->dev.h, &a, st, kernel_ms ? cb->ev_mark : nullptr));
  if (n_list) {
    int rcl = count_list_used(cb->counts, st);
    if (rcl) return rcl;
  }
  {
    int rcx = xfer_note_device_use(b->x, st);
    if (rcx) return rcx;
  }
  if (kernel_ms) {
    HIPCHK(hipEventRecord(cb->ev1, st));
    HIPCHK(hipEventSynchronize(cb->ev1));
    HIPCHK(hipEventElapsedTime(kernel_ms, cb->ev0, cb->ev1));
    HIPCHK(hipEventElapsedTime(&cb->last_ms[0], cb->ev0, cb->ev_mark[0]));
    HIPCHK(hipEventElapsedTime(&cb->last_ms[1], cb->ev_mark[0], cb->ev_mark[1]));
    HIPCHK(hipEventElapsedTime(&cb->last_ms[2], cb->ev_mark[1], cb->ev1));
  }
  if (t && t->mixers) {
    int rcn = xfer_writer_done(t->mixers->x, st, t->mixers->g->stream);
    if (rcn) return rcn;
  }
  if (t && t->indirect) {
    int rcn = xfer_writer_done(t->indirect->x, st, t->indirect->ib->stream);
    if (rcn) return rcn;
  }
  if (t && t->match) {
    int rcn = xfer_writer_done(t->match->x, st, t->match->mb->stream);
    if (rcn) return rcn;
  }
  return GMX_OK;
}

extern "C" int gmx_ctx_run(gmx_ctx* cb, gmx_ctx_batch* b, uint64_t n_bits, const gmx_ctx_targets* targets,
                           float* kernel_ms) {
  if (!cb || !b || b->cb != cb || n_bits > b->max_bits) return GMX_ERR_INVALID;
  int rc = ctx_targets_ok(cb, targets, n_bits);
  if (rc) return rc;
  if (n_bits)
    for (int s = 0; s < cb->S; ++s)
      if (cb->outstanding[s]) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(cb->device));
  rc = n_bits ? ctx_board_moves(cb, -1) : GMX_OK;
  if (!rc) rc = ctx_settle(cb);
  if (rc) return rc;
  if (kernel_ms) *kernel_ms = 0.0f;
  cb->moved = true;
  return ctx_launch(cb, b, n_bits, nullptr, targets, kernel_ms);
}

extern "C" int gmx_ctx_last_kernel_ms(const gmx_ctx* cb, float* ms) {
  if (!cb || !ms) return GMX_ERR_INVALID;
  memcpy(ms, cb->last_ms, sizeof cb->last_ms);
  return GMX_OK;
}

extern "C" int gmx_ctx_run_ragged(gmx_ctx* cb, gmx_ctx_batch* b, const uint64_t* n_bits,
                                  const gmx_ctx_targets* targets) {
  if (!cb || !b || b->cb != cb || !n_bits) return GMX_ERR_INVALID;
  uint64_t maxn = 0;
  bool same = true;
  for (int s = 0; s < cb->S; ++s) {
    if (n_bits[s] > b->max_bits) return GMX_ERR_INVALID;
    if (n_bits[s] && cb->outstanding[s]) return GMX_ERR_STATE;
    maxn = std::max(maxn, n_bits[s]);
    same = same && n_bits[s] == n_bits[0];
  }
  int rc = ctx_targets_ok(cb, targets, maxn);
  if (rc) return rc;
  HIPCHK(hipSetDevice(cb->device));
  for (int s = 0; s < cb->S && !rc; ++s)
    if (n_bits[s]) rc = ctx_board_moves(cb, s);
  if (!rc) rc = ctx_settle(cb);
  if (rc) return rc;
  cb->moved = true;
  return ctx_launch(cb, b, maxn, same ? nullptr : n_bits, targets, nullptr);
}

// ---- the per-bit surface: one record of gmx_ctx_run for one stream -----------------------------------------
// One launch of gmx_ctx_bit_kernel on the bank's stream, waited for when it predicts.  The stream's wave, if one runs
// (gmx_indirect_attach_ctx), does not touch the context bank unless a command tells it to, and every store of its
// last command was in memory before the host saw the answer: it need not stop, but it reads its copy again.
static int ctx_bit_launch(gmx_ctx* cb, int stream, uint32_t what, uint32_t bit, uint32_t* values, uint32_t* bit_context) {
  if (!cb->bit_reply) {
    HIPCHK(hipHostMalloc((void**)&cb->bit_reply, sizeof(GmxCtxBitReply), hipHostMallocDefault));
    memset(cb->bit_reply, 0, sizeof(GmxCtxBitReply));
  }
  GmxCtxBitArgs a;
  memset(&a, 0, sizeof a);
  a.banks = cb->banks;
  a.reply = cb->bit_reply;
  a.stream = stream;
  a.what = what;
  a.bit = bit;
  HIPCHK(gmx_launch_ctx_bit(cb->dev_d, &a, cb->stream));
  cb->bit_launches += 1;
  if (cb->host) cb->wave_fresh[stream] = 0;
  cb->moved = true;
  if (!(what & GMX_STEP_PREDICT)) return GMX_OK;  // (a learn is not waited for: whatever reads the bank next is behind it)
  HIPCHK(hipStreamSynchronize(cb->stream));
  if (values) memcpy(values, cb->bit_reply->values, 4 * (size_t)cb->dev.v);
  if (bit_context) *bit_context = cb->bit_reply->bit_context;
  return GMX_OK;
}

// A learn gmx_ctx_learn noted for stream s: on its own through the launch path now.
static int ctx_flush_noted(gmx_ctx* cb, int s) {
  if (!cb->noted[s]) return GMX_OK;
  const int rc = ctx_bit_launch(cb, s, GMX_STEP_LEARN, (uint32_t)(cb->noted[s] - 1), nullptr, nullptr);
  if (rc) return rc;
  cb->noted[s] = 0;
  cb->n_noted -= 1;
  return GMX_OK;
}

// The forward on the launch path; a noted learn of the stream travels in the same launch.
static int ctx_forward_launch(gmx_ctx* cb, int stream, uint32_t* values, uint32_t* bit_context) {
  {
    // (the Indirect learn of the stream's last chained forward first, where it is only noted: a wave restarted for it
    // later would recompute that forward from the board this launch moves)
    const int rcm = ctx_board_moves(cb, stream);
    if (rcm) return rcm;
  }
  uint32_t what = GMX_STEP_PREDICT, bit = 0;
  if (cb->noted[stream]) {
    what |= GMX_STEP_LEARN;
    bit = (uint32_t)(cb->noted[stream] - 1);
  }
  const int rc = ctx_bit_launch(cb, stream, what, bit, values, bit_context);
  if (rc) return rc;
  if (cb->noted[stream]) {
    cb->noted[stream] = 0;
    cb->n_noted -= 1;
  }
  cb->outstanding[stream] = 1;
  return GMX_OK;
}

// Tests: launches of gmx_ctx_bit_kernel on this bank so far -- forwards and learns of the launch path; a bit that went
// through the session wave adds none.
extern "C" int gmx_debug_ctx_bit_launches(const gmx_ctx* cb) { return cb ? cb->bit_launches : GMX_ERR_INVALID; }

extern "C" int gmx_ctx_forward(gmx_ctx* cb, int stream, uint32_t* values, uint32_t* bit_context) {
  if (!cb || stream < 0 || stream >= cb->S) return GMX_ERR_INVALID;
  if (cb->chainstep) return GMX_ERR_STATE;            // the lock-step object steps this bank
  if (cb->outstanding[stream]) return GMX_ERR_STATE;  // a Predict moves state: one per bit
  HIPCHK(hipSetDevice(cb->device));
  if (cb->host) {  // the waves stop; the stream's own noted learn still travels with this forward
    const int rc = ind_sessions_close(cb->host);
    if (rc) return rc;
    std::fill(cb->wave_fresh.begin(), cb->wave_fresh.end(), 0);
  }
  return ctx_forward_launch(cb, stream, values, bit_context);
}

// ShortTermMemory::new_bit of the stream: what Predictor::Learn and Predictor::Perceive both leave for the next
// BasicContexts::Predict, so a generated bit is perceived through this call too.
extern "C" int gmx_ctx_learn(gmx_ctx* cb, int stream, int bit) {
  if (!cb || stream < 0 || stream >= cb->S || (bit != 0 && bit != 1)) return GMX_ERR_INVALID;
  if (cb->chainstep) return GMX_ERR_STATE;
  if (!cb->noted[stream]) cb->n_noted += 1;
  cb->noted[stream] = (uint8_t)(1 + bit);
  cb->outstanding[stream] = 0;
  return GMX_OK;
}

// ---- the blackboard --------------------------------------------------------------------------------
static uint8_t* ctx_bank(gmx_ctx* cb, int stream) { return cb->banks + (size_t)stream * cb->dev.bank_bytes; }

extern "C" int gmx_ctx_blackboard_get(gmx_ctx* cb, int stream, gmx_ctx_blackboard* out) {
  if (!cb || stream < 0 || stream >= cb->S || !out) return GMX_ERR_INVALID;
  if (cb->outstanding[stream]) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(cb->device));
  {
    int rcs = ctx_settle(cb);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(cb->stream));
  GmxCtxBoard bd;
  HIPCHK(hipMemcpy(&bd, ctx_bank(cb, stream) + cb->dev.board_off, sizeof bd, hipMemcpyDeviceToHost));
  memset(out, 0, sizeof *out);
  out->recent_bits = (int32_t)bd.recent_bits;
  out->new_bit = (int32_t)bd.new_bit;
  out->first_prediction = (int32_t)bd.first_prediction;
  out->rotating_history_pos = bd.pos;
  memcpy(out->rotating_history, bd.ring, GMX_CTX_RING);
  for (int i = 0; i < 10; ++i) out->recent_bytes[i] = bd.ring[(bd.pos + GMX_CTX_RING - i) % GMX_CTX_RING];
  out->last_byte = out->recent_bytes[0];
  memcpy(out->values, bd.values, 4 * (size_t)cb->dev.v);
  return GMX_OK;
}

extern "C" int gmx_ctx_blackboard_set(gmx_ctx* cb, int stream, const gmx_ctx_blackboard* in) {
  if (!cb || stream < 0 || stream >= cb->S || !in) return GMX_ERR_INVALID;
  if (in->recent_bits < 1 || in->recent_bits > 255 || (in->new_bit != 0 && in->new_bit != 1) ||
      in->rotating_history_pos >= GMX_CTX_RING || (in->first_prediction && in->recent_bits != 1))
    return GMX_ERR_INVALID;
  for (int i = 0; i < 10; ++i)  // last_byte and recent_bytes are views of the ring here
    if (in->recent_bytes[i] != in->rotating_history[(in->rotating_history_pos + GMX_CTX_RING - i) % GMX_CTX_RING])
      return GMX_ERR_INVALID;
  if (in->last_byte != in->recent_bytes[0]) return GMX_ERR_INVALID;
  GmxCtxBoard bd;
  memset(&bd, 0, sizeof bd);
  bd.recent_bits = (uint32_t)in->recent_bits;
  bd.new_bit = (uint32_t)in->new_bit;
  bd.first_prediction = in->first_prediction ? 1u : 0u;
  bd.pos = in->rotating_history_pos;
  memcpy(bd.ring, in->rotating_history, GMX_CTX_RING);
  memcpy(bd.values, in->values, 4 * (size_t)cb->dev.v);
  HIPCHK(hipSetDevice(cb->device));
  {
    int rcs = ctx_board_moves(cb, stream);
    if (!rcs) rcs = ctx_settle(cb);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(cb->stream));
  HIPCHK(hipMemcpy(ctx_bank(cb, stream) + cb->dev.board_off, &bd, sizeof bd, hipMemcpyHostToDevice));
  cb->outstanding[stream] = 0;
  cb->moved = true;
  return GMX_OK;
}

// ---- persistence: IndirectHash::WriteToDisk / ReadFromDisk x H (indirect-hash.cpp:33-74) ---------------
static int ctx_ckpt_ready(gmx_ctx* cb) {
  if (cb->chunks_d || cb->chunks.empty()) return GMX_OK;
  const size_t n = cb->chunks.size();
  HIPCHK(hipMalloc((void**)&cb->chunks_d, n * sizeof(GmxCtxCkptChunk)));
  HIPCHK(hipMemcpy(cb->chunks_d, cb->chunks.data(), n * sizeof(GmxCtxCkptChunk), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc((void**)&cb->chunk_cnt_d, n * 4));
  HIPCHK(hipMalloc((void**)&cb->chunk_base_d, n * 4));
  HIPCHK(hipMalloc((void**)&cb->hash_dense_d, GMX_CTX_MAX_HASH));
  HIPCHK(hipMalloc((void**)&cb->hash_cnt_d, GMX_CTX_MAX_HASH * 4));
  HIPCHK(hipMalloc((void**)&cb->hash_off_d, GMX_CTX_MAX_HASH * 8));
  return GMX_OK;
}
static bool ctx_is_dense(uint32_t cnt, uint32_t size) { return !(cnt < size / 2); }  // indirect-hash.cpp:42

extern "C" int gmx_ctx_export(gmx_ctx* cb, int stream, void* buf, size_t* bytes, size_t* offsets) {
  if (!cb || stream < 0 || stream >= cb->S || !bytes) return GMX_ERR_INVALID;
  const GmxCtxDev& d = cb->dev;
  const int H = d.h;
  HIPCHK(hipSetDevice(cb->device));
  {
    int rcs = ctx_settle(cb);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(cb->stream));
  if (H == 0) {
    if (offsets) offsets[0] = 0;
    *bytes = 0;
    return GMX_OK;
  }
  int rc = ctx_ckpt_ready(cb);
  if (rc) return rc;
  uint8_t* const bank = ctx_bank(cb, stream);
  const size_t n_chunks = cb->chunks.size();
  GmxCtxCkptArgs a;
  memset(&a, 0, sizeof a);
  a.bank = bank;
  a.dev = cb->dev_d;
  a.chunks = cb->chunks_d;
  a.n_chunks = (uint32_t)n_chunks;
  a.chunk_cnt = cb->chunk_cnt_d;
  a.chunk_base = cb->chunk_base_d;
  a.hash_dense = cb->hash_dense_d;
  a.hash_cnt = cb->hash_cnt_d;
  a.hash_off = cb->hash_off_d;
  // count on the device, scan on the host
  HIPCHK(gmx_launch_ctx_ckpt_count(&a, cb->stream));
  std::vector<uint32_t> cc(n_chunks), base(n_chunks);
  HIPCHK(hipMemcpyAsync(cc.data(), cb->chunk_cnt_d, n_chunks * 4, hipMemcpyDeviceToHost, cb->stream));
  HIPCHK(hipStreamSynchronize(cb->stream));
  uint32_t cnt[GMX_CTX_MAX_HASH] = {};
  uint8_t dense[GMX_CTX_MAX_HASH] = {};
  uint64_t poff[GMX_CTX_MAX_HASH] = {}, body[GMX_CTX_MAX_HASH] = {};
  for (size_t c = 0; c < n_chunks; ++c) {
    base[c] = cnt[cb->chunks[c].hash];
    cnt[cb->chunks[c].hash] += cc[c];
  }
  uint64_t pairs = 0;
  size_t need = 0;
  for (int i = 0; i < H; ++i) {
    dense[i] = ctx_is_dense(cnt[i], d.hash[i].table_size) ? 1 : 0;
    body[i] = dense[i] ? 4ull * d.hash[i].table_size : 8ull * cnt[i];
    poff[i] = 2 * pairs;
    if (!dense[i]) pairs += cnt[i];
    if (offsets) offsets[i] = need;
    need += 4 + body[i] + 12;
  }
  if (offsets) offsets[H] = need;
  const bool fits = !buf || *bytes >= need;
  *bytes = need;
  if (!buf) return GMX_OK;
  if (!fits) return GMX_ERR_INVALID;
  GmxCtxHashState hs[GMX_CTX_MAX_HASH];
  HIPCHK(hipMemcpy(hs, bank + d.hstate_off, sizeof hs, hipMemcpyDeviceToHost));
  // pack on the device: the host reads only what it writes out
  uint32_t* pk = nullptr;
  if (pairs) {
    hipError_t e = hipMalloc((void**)&pk, pairs * 8);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? GMX_ERR_NOMEM : hip_fail(e, "hipMalloc(pairs)");
  }
  a.buf = pk;
  int ret = GMX_OK;
#define XCHK(call)               \
  do {                           \
    hipError_t e_ = (call);      \
    if (e_ != hipSuccess) {      \
      ret = hip_fail(e_, #call); \
      goto out;                  \
    }                            \
  } while (0)
  {
    if (pairs) {
      XCHK(hipMemcpyAsync(cb->chunk_base_d, base.data(), n_chunks * 4, hipMemcpyHostToDevice, cb->stream));
      XCHK(hipMemcpyAsync(cb->hash_dense_d, dense, sizeof dense, hipMemcpyHostToDevice, cb->stream));
      XCHK(hipMemcpyAsync(cb->hash_off_d, poff, sizeof poff, hipMemcpyHostToDevice, cb->stream));
      XCHK(gmx_launch_ctx_ckpt_pack(&a, cb->stream));
      XCHK(hipStreamSynchronize(cb->stream));
    }
    uint8_t* o = (uint8_t*)buf;
    for (int i = 0; i < H; ++i) {
      memcpy(o, &cnt[i], 4);
      o += 4;
      if (body[i]) {
        if (dense[i]) XCHK(hipMemcpy(o, bank + d.hash[i].tab_off, (size_t)body[i], hipMemcpyDeviceToHost));
        else XCHK(hipMemcpy(o, pk + poff[i], (size_t)body[i], hipMemcpyDeviceToHost));
      }
      o += body[i];
      memcpy(o, &hs[i].outer_context, 8);
      memcpy(o + 8, &hs[i].outer_hash, 4);
      o += 12;
    }
  }
out:
#undef XCHK
  if (pk) (void)hipFree(pk);
  return ret;
}

// gmx_ctx_import's rules over one stream's H sections -- lengths, the branch against the count, strictly ascending
// keys below the table size, no zero value in a sparse record, the count of a dense table -- for both imports
// (gmx_ctx_ckpt.inc).  Touches no bank.
struct GmxCtxSection {
  uint32_t cnt[GMX_CTX_MAX_HASH];
  uint8_t dense[GMX_CTX_MAX_HASH];
  uint64_t poff[GMX_CTX_MAX_HASH];       // u32 offset of a sparse table's pairs among the section's pairs
  const uint8_t* body[GMX_CTX_MAX_HASH];  // behind the table's u32 count
  GmxCtxHashState hs[GMX_CTX_MAX_HASH];
  uint64_t pairs;
};
static int ctx_validate_section(const GmxCtxDev& d, const uint8_t* lb, size_t bytes, GmxCtxSection* sec) {
  const int H = d.h;
  const uint8_t* p = lb;
  const uint8_t* const end = lb + bytes;
  memset(sec, 0, sizeof *sec);
  uint32_t* const cnt = sec->cnt;
  uint8_t* const dense = sec->dense;
  uint64_t* const poff = sec->poff;
  const uint8_t** const body = sec->body;
  GmxCtxHashState* const hs = sec->hs;
  uint64_t pairs = 0;
  for (int i = 0; i < H; ++i) {
    const uint32_t size = d.hash[i].table_size;
    if (end - p < 4) return GMX_ERR_FORMAT;
    memcpy(&cnt[i], p, 4);
    p += 4;
    if (cnt[i] > size) return GMX_ERR_FORMAT;
    dense[i] = ctx_is_dense(cnt[i], size) ? 1 : 0;
    body[i] = p;
    if (!dense[i]) {
      if ((uint64_t)(end - p) < 8ull * cnt[i]) return GMX_ERR_FORMAT;
      uint32_t prev = 0;
      for (uint32_t c = 0; c < cnt[i]; ++c, p += 8) {
        uint32_t key, val;
        memcpy(&key, p, 4);
        memcpy(&val, p + 4, 4);
        if (key >= size || (c > 0 && key <= prev) || val == 0) return GMX_ERR_FORMAT;
        prev = key;
      }
      poff[i] = 2 * pairs;
      pairs += cnt[i];
    } else {
      if ((uint64_t)(end - p) < 4ull * size) return GMX_ERR_FORMAT;
      uint32_t nz = 0;
      for (uint32_t e = 0; e < size; ++e, p += 4) {
        uint32_t val;
        memcpy(&val, p, 4);
        nz += val != 0;
      }
      if (nz != cnt[i]) return GMX_ERR_FORMAT;  // the branch follows from the count
    }
    if (end - p < 12) return GMX_ERR_FORMAT;
    memcpy(&hs[i].outer_context, p, 8);
    memcpy(&hs[i].outer_hash, p + 8, 4);
    p += 12;
  }
  if (p != end) return GMX_ERR_FORMAT;
  sec->pairs = pairs;
  return GMX_OK;
}

extern "C" int gmx_ctx_import(gmx_ctx* cb, int stream, const void* buf, size_t bytes) {
  if (!cb || stream < 0 || stream >= cb->S || (!buf && bytes)) return GMX_ERR_INVALID;
  const GmxCtxDev& d = cb->dev;
  const int H = d.h;
  // ---- validate everything before the bank is touched
  GmxCtxSection sec;
  {
    int rcv = ctx_validate_section(d, (const uint8_t*)buf, bytes, &sec);
    if (rcv) return rcv;
  }
  const uint32_t* const cnt = sec.cnt;
  const uint8_t* const dense = sec.dense;
  const uint64_t* const poff = sec.poff;
  const uint8_t* const* const body = sec.body;
  const GmxCtxHashState* const hs = sec.hs;
  const uint64_t pairs = sec.pairs;
  if (H == 0) return GMX_OK;
  // ---- the bank
  HIPCHK(hipSetDevice(cb->device));
  {
    int rcs = ctx_settle(cb);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(cb->stream));
  int rc = ctx_ckpt_ready(cb);
  if (rc) return rc;
  uint8_t* const bank = ctx_bank(cb, stream);
  uint32_t* staged = nullptr;
  if (pairs) {
    hipError_t e = hipMalloc((void**)&staged, pairs * 8);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? GMX_ERR_NOMEM : hip_fail(e, "hipMalloc(pairs)");
  }
  int ret = GMX_OK;
#define XCHK(call)               \
  do {                           \
    hipError_t e_ = (call);      \
    if (e_ != hipSuccess) {      \
      ret = hip_fail(e_, #call); \
      goto out;                  \
    }                            \
  } while (0)
  {
    GmxCtxCkptArgs a;
    memset(&a, 0, sizeof a);
    a.bank = bank;
    a.dev = cb->dev_d;
    a.hash_dense = cb->hash_dense_d;
    a.hash_cnt = cb->hash_cnt_d;
    a.hash_off = cb->hash_off_d;
    a.buf = staged;
    XCHK(hipMemsetAsync(bank, 0, (size_t)d.tab_bytes, cb->stream));
    for (int i = 0; i < H; ++i) {
      if (dense[i]) XCHK(hipMemcpyAsync(bank + d.hash[i].tab_off, body[i], 4ull * d.hash[i].table_size,
                                        hipMemcpyHostToDevice, cb->stream));
      else if (cnt[i]) XCHK(hipMemcpyAsync(staged + poff[i], body[i], 8ull * cnt[i], hipMemcpyHostToDevice, cb->stream));
    }
    if (pairs) {
      XCHK(hipMemcpyAsync(cb->hash_dense_d, dense, sizeof sec.dense, hipMemcpyHostToDevice, cb->stream));
      XCHK(hipMemcpyAsync(cb->hash_cnt_d, cnt, sizeof sec.cnt, hipMemcpyHostToDevice, cb->stream));
      XCHK(hipMemcpyAsync(cb->hash_off_d, poff, sizeof sec.poff, hipMemcpyHostToDevice, cb->stream));
      XCHK(gmx_launch_ctx_ckpt_scatter(&a, H, cb->stream));
    }
    XCHK(hipMemcpyAsync(bank + d.hstate_off, hs, sizeof sec.hs, hipMemcpyHostToDevice, cb->stream));
    XCHK(hipStreamSynchronize(cb->stream));  // (the sources are the caller's and this frame's)
  }
out:
#undef XCHK
  if (staged) (void)hipFree(staged);
  return ret;
}

// IndirectHash::Copy x H (indirect-hash.cpp:76-81) and ShortTermMemory::Copy's share of the blackboard.
extern "C" int gmx_ctx_copy(gmx_ctx* dst, int dst_stream, gmx_ctx* src, int src_stream) {
  if (!dst || !src || dst_stream < 0 || dst_stream >= dst->S || src_stream < 0 || src_stream >= src->S)
    return GMX_ERR_INVALID;
  if (dst->device != src->device || dst->dev.v != src->dev.v || dst->dev.h != src->dev.h ||
      dst->dev.bank_bytes != src->dev.bank_bytes ||
      memcmp(dst->dev.var, src->dev.var, sizeof dst->dev.var) != 0 ||
      memcmp(dst->dev.hash, src->dev.hash, sizeof dst->dev.hash) != 0 ||
      memcmp(dst->dev.maps, src->dev.maps, sizeof dst->dev.maps) != 0)
    return GMX_ERR_INVALID;
  if (src->outstanding[src_stream]) return GMX_ERR_STATE;
  if (dst == src && dst_stream == src_stream) return GMX_OK;
  HIPCHK(hipSetDevice(src->device));
  {
    int rcs = ctx_board_moves(dst, dst_stream);
    if (!rcs) rcs = ctx_settle(src);
    if (!rcs && dst != src) rcs = ctx_settle(dst);
    if (rcs) return rcs;
  }
  HIPCHK(hipStreamSynchronize(src->stream));
  if (dst != src) HIPCHK(hipStreamSynchronize(dst->stream));
  HIPCHK(hipMemcpy(ctx_bank(dst, dst_stream), ctx_bank(src, src_stream), dst->dev.bank_bytes,
                   hipMemcpyDeviceToDevice));
  dst->outstanding[dst_stream] = 0;
  dst->moved = true;
  return GMX_OK;
}

extern "C" int gmx_ctx_memory_usage(gmx_ctx* cb, int var, uint64_t* bytes) {
  if (!cb || var < 0 || var >= cb->dev.v || !bytes) return GMX_ERR_INVALID;
  const GmxCtxVarDev& v = cb->dev.var[var];
  // GetMemoryUsage of the variable's object (indirect-hash.cpp:83-89, interval-context.h, skip-context.h); the fields
  // of BasicContexts have no object of their own
  *bytes = v.kind == GMX_CTX_INDIRECT_HASH ? 36ull + 4ull * cb->dev.hash[v.index].table_size
           : v.kind == GMX_CTX_INTERVAL    ? 256ull * 4 + 8 + 4
           : v.kind == GMX_CTX_SKIP        ? 4ull * (uint64_t)v.n_bytes + 4
                                           : 0;
  return GMX_OK;
}

// ---- in the per-bit sessions: the bank's streams step in the session waves of an Indirect bank -----------------------
// Either object goes, or the attachment is given up: the waves stop (nothing of a stream's context state lives in
// them), a noted learn stays noted and takes the launch path with the stream's next forward.
static int ctx_host_detach(gmx_ctx* cb) {
  if (!cb || !cb->host) return GMX_OK;
  gmx_indirect* ib = cb->host;
  (void)hipSetDevice(ib->device);
  const int rc = ind_sessions_close(ib);
  ib->ctx = nullptr;
  ib->ctx_dev_d = nullptr;
  ib->ctx_banks = nullptr;
  ib->ctx_routes_d = nullptr;
  ib->ctx_bank_bytes = 0;
  ib->ctx_v = ib->ctx_n_mixer_cols = 0;
  cb->host = nullptr;
  std::fill(cb->wave_fresh.begin(), cb->wave_fresh.end(), 0);
  return rc;
}

extern "C" int gmx_indirect_attach_ctx(gmx_indirect* ib, gmx_ctx* cb, const gmx_ctx_step_routes* routes) {
  if (!ib) return GMX_ERR_INVALID;
  if (!cb) {  // detach
    HIPCHK(hipSetDevice(ib->device));
    return ib->ctx ? ctx_host_detach(ib->ctx) : GMX_OK;
  }
  if (!routes || cb->S != ib->S || cb->device != ib->device) return GMX_ERR_INVALID;
  const int K = ib->dev.k, KM = ib->match ? ib->match_k : 0;
  // (the mixer route's length is checked against the group's M by the forward, which knows the group)
  if (routes->n_mixer_route > GMX_MAX_MIXERS ||
      ctx_route_ok(cb, routes->mixer_route, routes->n_mixer_route, routes->n_mixer_route))
    return GMX_ERR_INVALID;
  if (ctx_route_ok(cb, routes->ind_route, routes->n_ind_route, K)) return GMX_ERR_INVALID;
  const bool has_match = routes->match_route || routes->n_match_route;
  if (has_match != (KM > 0)) return GMX_ERR_INVALID;  // NULL / 0 iff no Match bank is attached to ib
  if (has_match && ctx_route_ok(cb, routes->match_route, routes->n_match_route, KM)) return GMX_ERR_INVALID;
  for (int c = 0; c < ib->match_n_cols; ++c)  // a column has one writer on the device
    if (KM > 0 && ib->match_cols[c] < routes->n_mixer_route && routes->mixer_route[ib->match_cols[c]] >= 0)
      return GMX_ERR_INVALID;
  if (cb->chainstep) return GMX_ERR_STATE;  // one host of its per-bit state at a time
  if (cb->host && cb->host != ib) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(ib->device));
  int rc = ib->ctx ? ctx_host_detach(ib->ctx) : GMX_OK;  // (another bank, or this one with other routes)
  if (rc) return rc;
  rc = ind_sessions_close(ib);  // the waves that run are a build without the context phase
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(cb->stream));
  if (!cb->routes_d) HIPCHK(hipMalloc((void**)&cb->routes_d, sizeof cb->routes));
  for (int32_t& r : cb->routes) r = -1;
  memcpy(cb->routes + GMX_CTX_WAVE_ROUTE_IND, routes->ind_route, 4 * (size_t)K);
  if (has_match) memcpy(cb->routes + GMX_CTX_WAVE_ROUTE_MATCH, routes->match_route, 4 * (size_t)KM);
  memcpy(cb->routes + GMX_CTX_WAVE_ROUTE_MIXER, routes->mixer_route, 4 * (size_t)routes->n_mixer_route);
  HIPCHK(hipMemcpy(cb->routes_d, cb->routes, sizeof cb->routes, hipMemcpyHostToDevice));
  cb->own_ind = cb->own_match = false;
  for (int c = 0; c < K; ++c) cb->own_ind = cb->own_ind || routes->ind_route[c] < 0;
  for (int c = 0; c < KM; ++c) cb->own_match = cb->own_match || routes->match_route[c] < 0;
  std::fill(cb->wave_fresh.begin(), cb->wave_fresh.end(), 0);
  ib->ctx = cb;
  ib->ctx_dev_d = cb->dev_d;
  ib->ctx_banks = cb->banks;
  ib->ctx_bank_bytes = cb->dev.bank_bytes;
  ib->ctx_routes_d = cb->routes_d;
  ib->ctx_v = cb->dev.v;
  ib->ctx_n_mixer_cols = routes->n_mixer_route;
  cb->host = ib;
  return GMX_OK;
}
