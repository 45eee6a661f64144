// gmx_lockstep.inc -- many streams advancing one bit at a time, all together (included by
// gmx_capi.cpp).
//
// A decoder learns its bit from Predict's own result (coder/decoder.cpp:19-39), so S files being
// decoded on one GPU advance in lock step: Predict for all S, S arithmetic decoders on the host,
// Learn for all S.  Through the batched surface that is four memcpys, a launch and a
// synchronisation for the first half and three more calls for the second, per BIT -- launch-bound
// (82 us per step at S = 1).  Here each half is ONE hipGraph, captured once: the record uploads,
// the kernel (T = 1; forward with its outputs latched, or learn from the latch) and the download
// of the S probabilities.  What changes from step to step travels through fixed buffers: the
// records in the batch's pinned host arrays, the decay factors in a pinned array of S floats the
// host refills with libm before every learn (the bits likewise go through a private pinned copy: the
// learn graph runs asynchronously, the caller's array is free again when the call returns).

static hipError_t lockstep_launch_kernel(gmx_group* g, const GmxRunArgs& a, hipStream_t on = nullptr) {
  const bool stock = g->topo.n == 90 && g->topo.l0 == 24 && g->topo.l1 == 8 && g->topo.n_skip == 1 &&
                     g->topo.has_final && g->topo.mx[23].stride == 128 && !g->force_general;
  hipStream_t st = on ? on : g->stream;
  if (stock)
    return gmx_launch_stock_kernel(g->topo_dev, &a, g->S, GMX_STK_LDS_BYTES(g->topo.lds_misc), a.mask != nullptr, g->stock_staged,
                                   topo_tables_pow2(g->topo), st);
  return gmx_launch_bank_kernel(g->topo_dev, &a, g->S, g->lds_bytes, a.mask != nullptr, g->topo.l0, g->topo.l1,
                                g->topo.n_skip, g->topo.has_final, g->topo.mx[g->topo.l0 - 1].stride, st);
}


// ---- GMX_LOCKSTEP_PERSISTENT: S persistent waves behind one doorbell (gmx_stock_lockstep_kernel) --------
extern "C" hipError_t gmx_launch_stock_lockstep(const GmxTopoDev* tp_dev, const GmxLsArgs* args, unsigned lds_bytes,
                                                hipStream_t stream);
extern "C" int gmx_stock_lockstep_capacity(unsigned lds_bytes, int device);

// The decay factor of every stream's next learn (+ `ahead` learns from now): one libm call per distinct bit
// count, and streams in lock step mostly stand at the same one.
static void ls_fill_decay(gmx_lockstep* ls, uint64_t ahead) {
  gmx_group* g = ls->g;
  uint64_t at = ~0ull;
  float v = 0.0f;
  for (int s = 0; s < g->S; ++s) {
    if (g->steps[s] + ahead != at) {
      at = g->steps[s] + ahead;
      v = decay_base(at);
    }
    ls->dec_host[s] = v;
  }
}

// Every wave fetches its own record across the link: 9 us per step + 0.1-0.2 us per stream (the link does about 100 M
// small reads a second), against 41 us + 0.025 us per stream for a graph with its bulk copies: 9 / 23 / 54 us at
// 1 / 64 / 256 streams against 41 / 41 / 47 -- beyond this many streams the flag is ignored.  (Bulk copies into
// the device while the waves spin were tried twice: slower at 64 streams, and from 256 streams on they only
// complete when the waves leave on their idle timers.)
static const int kLsPersistentMaxStreams = 128;

static int ls_persist_launch(gmx_lockstep* ls) {
  gmx_group* g = ls->g;
  gmx_batch* b = ls->b;
  if (ls->ps_running) HIPCHK(hipStreamSynchronize(ls->ps_stream));  // (only ever called when the blocks have left)
  GmxLsArgs a;
  memset(&a, 0, sizeof a);
  a.banks = g->banks;
  a.door = ls->door;
  a.done = ls->done;
  a.pred = b->h_pred;
  a.mask = b->h_mask;
  a.ctx = b->h_ctx;
  a.bits = ls->bits_host;
  a.dec = ls->dec_host;
  a.p = b->h_p;
  a.outs = (b->flags & GMX_BATCH_OUTPUTS) ? b->h_out : nullptr;
  a.blk_seen = ls->blk_seen;
  a.blk_replay = ls->blk_replay;
  a.relay = ls->relay;
  a.live = ls->live;
  a.idle_ticks = kIdleTicks;
  a.n_streams = g->S;
  a.exact = g->stock_exact ? 1 : 0;
  if (!ls->ps_counted) {
    g_open_sessions.fetch_add(1);
    ls->ps_counted = true;
  }
  ls->ps_running = true;
  HIPCHK(gmx_launch_stock_lockstep(g->topo_dev, &a, GMX_STK_LDS_BYTES(g->topo.lds_misc), ls->ps_stream));
  return GMX_OK;
}

static int ls_publish(gmx_lockstep* ls, uint32_t cmd) {
  ls->seq += 1;
  ls->word = (ls->seq << GMX_MB_SEQ_SHIFT) | cmd;
  mb_store_fence();  // the records in the host arrays are out before the doorbell rings
  __atomic_store_n(&ls->door->cmd_seq, ls->word, __ATOMIC_RELEASE);
  mb_store_fence();
  return GMX_OK;
}

// Until every block has answered the newest command.  Blocks that left on their idle timers before they saw
// it come back with the next launch (each knows what it has done, blk_seen); bounded.
static int ls_wait(gmx_lockstep* ls) {
  if (ls->ps_dead) {
    g_last_error = "persistent lock-step waves do not answer";
    return GMX_ERR_HIP;
  }
  uint64_t spins = 0;
  timespec t_start = {0, 0};
  while (mb_load(ls->done) != ls->word) {
    if ((++spins & 0xff) == 0) {
      if (hipStreamQuery(ls->ps_stream) == hipSuccess && mb_load(ls->done) != ls->word) {
        int rc = ls_persist_launch(ls);  // all blocks have left, some without having seen the command
        if (rc) return rc;
      }
      (void)hipGetLastError();
      timespec now;
      clock_gettime(CLOCK_MONOTONIC, &now);
      if (spins == 0x100) t_start = now;
      if (now.tv_sec - t_start.tv_sec > 10) {
        g_last_error = "persistent lock-step waves do not answer";
        (void)ls_publish(ls, GMX_MB_STOP);
        ls->ps_dead = true;
        if (ls->ps_counted) {  // the slot count is given back, the buffers are not (the waves may still be there)
          g_open_sessions.fetch_sub(1);
          ls->ps_counted = false;
        }
        return GMX_ERR_HIP;
      }
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  ls->completed = ls->word;
  ls->learn_inflight = false;
  return GMX_OK;
}

// The waves hand the banks back (rows and counters written to HBM).  What a Predict latched is gone with them --
// unless the caller only reads the banks (keep_forward: a checkpoint or a usage query between Predict and Learn):
// then every block keeps the forward it has not learned from and the next instance redoes it, as after an idle exit,
// so that the Learn that follows finds its Predict like on the graph path (whose latch survives such calls).
static int ls_persist_stop(gmx_lockstep* ls, bool keep_forward = false) {
  if (!ls->persistent || !ls->ps_running) return GMX_OK;
  if (ls->ps_dead) {
    g_last_error = "persistent lock-step waves do not answer";
    return GMX_ERR_HIP;
  }
  if (ls->seq != 0 && ls->completed != ls->word) {
    int rc = ls_wait(ls);
    if (rc) return rc;
  }
  const bool keep = keep_forward && ls->predicted;
  (void)ls_publish(ls, keep ? GMX_MB_STOP_KEEP : GMX_MB_STOP);
  HIPCHK(hipStreamSynchronize(ls->ps_stream));
  // the doorbell shows the last command everybody completed again: the next instance waits for a new one
  __atomic_store_n(&ls->door->cmd_seq, ls->completed, __ATOMIC_RELEASE);
  mb_store_fence();
  {
    uint32_t img[64];
    memset(img, 0, sizeof img);
    img[0] = ls->completed;
    HIPCHK(hipMemcpy(ls->relay, img, sizeof img, hipMemcpyHostToDevice));
  }
  ls->word = ls->completed;
  ls->ps_running = false;
  if (ls->ps_counted) {
    g_open_sessions.fetch_sub(1);
    ls->ps_counted = false;
  }
  if (!keep) ls->predicted = false;
  return GMX_OK;
}

static int locksteps_stop(gmx_group* g, gmx_lockstep* except, bool keep_forward) {
  int first = GMX_OK;
  for (gmx_lockstep* ls : g->locksteps) {
    if (ls == except) continue;
    int rc = ls_persist_stop(ls, keep_forward);
    if (rc && !first) first = rc;
  }
  return first;
}

// Before a persistent step: nobody else holds rows, the waves run, the previous (asynchronous) learn is done.
static int ls_persist_ready(gmx_lockstep* ls) {
  gmx_group* g = ls->g;
  int rc = sessions_close_perbit(g, false);
  if (rc) return rc;
  rc = locksteps_stop(g, ls, false);
  if (rc) return rc;
  if (ls->ps_dead) {
    g_last_error = "persistent lock-step waves do not answer";
    return GMX_ERR_HIP;
  }
  if (!ls->ps_running || hipStreamQuery(ls->ps_stream) == hipSuccess) {
    (void)hipGetLastError();
    HIPCHK(hipStreamSynchronize(g->stream));  // batched work on the banks is finished
    rc = ls_persist_launch(ls);
    if (rc) return rc;
  }
  (void)hipGetLastError();
  if (ls->seq != 0 && ls->completed != ls->word) return ls_wait(ls);
  return GMX_OK;
}
extern "C" void gmx_lockstep_destroy(gmx_lockstep* ls) {
  if (!ls) return;
  if (ls->g) {
    (void)hipSetDevice(ls->g->device);
    (void)ls_persist_stop(ls);
    if (ls->g->stream) (void)hipStreamSynchronize(ls->g->stream);
    auto& v = ls->g->locksteps;
    v.erase(std::remove(v.begin(), v.end(), ls), v.end());
  }
  // Persistent waves that stopped answering may still be polling: wait a bounded time for them, and if they are
  // still there free NOTHING they can touch -- their argument block points at dec_host, bits_host, the batch's pinned
  // arrays, the doorbell and the group's banks (leaked rather than freed under a running kernel; hipFree could
  // block on it, too).
  if (ls->ps_stream) {
    bool gone = true;
    if (ls->ps_dead) {
      gone = false;
      for (int i = 0; i < 1000 && !gone; ++i) {
        gone = hipStreamQuery(ls->ps_stream) == hipSuccess;
        if (!gone) {
          timespec ts = {0, 1000000};
          nanosleep(&ts, nullptr);
        }
      }
      (void)hipGetLastError();
    } else {
      (void)hipStreamSynchronize(ls->ps_stream);
    }
    if (!gone) {
      if (ls->g) ls->g->banks_in_use_by_dead_kernel = true;
      if (ls->b) batch_core_detach(*ls->b);  // the batch stays alive, out of the group's list
      ls->b = nullptr;
      delete ls;
      return;
    }
    (void)hipStreamDestroy(ls->ps_stream);
  }
  if (ls->x_predict) (void)hipGraphExecDestroy(ls->x_predict);
  if (ls->x_learn) (void)hipGraphExecDestroy(ls->x_learn);
  if (ls->x_step) (void)hipGraphExecDestroy(ls->x_step);
  if (ls->g_step) (void)hipGraphDestroy(ls->g_step);
  if (ls->g_predict) (void)hipGraphDestroy(ls->g_predict);
  if (ls->g_learn) (void)hipGraphDestroy(ls->g_learn);
  if (ls->dec_host) (void)hipHostFree(ls->dec_host);
  if (ls->bits_host) (void)hipHostFree(ls->bits_host);
  if (ls->dec_dev) (void)hipFree(ls->dec_dev);
  if (ls->idx_dev) (void)hipFree(ls->idx_dev);
  if (ls->door) (void)hipFree(ls->door);
  if (ls->done) (void)hipHostFree(ls->done);
  if (ls->blk_seen) (void)hipFree(ls->blk_seen);
  if (ls->blk_replay) (void)hipFree(ls->blk_replay);
  if (ls->relay) (void)hipFree(ls->relay);
  if (ls->live) (void)hipFree(ls->live);
  if (ls->b) batch_free(ls->b);
  delete ls;
}

extern "C" int gmx_lockstep_create(gmx_lockstep** out, gmx_group* g, unsigned flags) {
  if (!out || !g) return GMX_ERR_INVALID;
  *out = nullptr;
  HIPCHK(hipSetDevice(g->device));
  int rc = sessions_close(g, false);
  if (rc) return rc;
  gmx_lockstep* ls = new (std::nothrow) gmx_lockstep();
  if (!ls) return GMX_ERR_NOMEM;
  ls->g = g;
  g->locksteps.push_back(ls);
#define LCHK(call)                                 \
  do {                                             \
    hipError_t e_ = (call);                        \
    if (e_ != hipSuccess) {                        \
      int r_ = hip_fail(e_, #call);                \
      gmx_lockstep_destroy(ls);                    \
      return e_ == hipErrorOutOfMemory ? GMX_ERR_NOMEM : r_; \
    }                                              \
  } while (0)
  rc = batch_alloc(&ls->b, g, g->S, 1, GMX_BATCH_MASK | (flags & GMX_BATCH_OUTPUTS));
  if (rc) {
    gmx_lockstep_destroy(ls);
    return rc;
  }
  gmx_batch* b = ls->b;
  if (!gmx_batch_predictions(b) || !gmx_batch_active_mask(b) || !gmx_batch_contexts(b) || !gmx_batch_bits(b) ||
      !gmx_batch_p(b) || ((flags & GMX_BATCH_OUTPUTS) && !gmx_batch_outputs(b))) {
    gmx_lockstep_destroy(ls);
    return GMX_ERR_NOMEM;
  }
  const GmxTopoDev& t = g->topo;
  const size_t S = (size_t)g->S;
  memset(b->h_pred, 0, S * t.n_pad * sizeof(float));
  memset(b->h_mask, 0xff, S * t.mask_words * sizeof(uint32_t));
  memset(b->h_ctx, 0, S * t.m * sizeof(uint32_t));
  memset(b->h_bits, 0, S);
  LCHK(hipHostMalloc((void**)&ls->dec_host, S * sizeof(float), hipHostMallocDefault));
  LCHK(hipHostMalloc((void**)&ls->bits_host, S, hipHostMallocDefault));
  memset(ls->bits_host, 0, S);
  LCHK(hipMalloc((void**)&ls->dec_dev, S * sizeof(float)));
  LCHK(hipMalloc((void**)&ls->idx_dev, S * sizeof(uint32_t)));
  {
    std::vector<uint32_t> idn(S);
    for (size_t s = 0; s < S; ++s) idn[s] = (uint32_t)s;
    LCHK(hipMemcpy(ls->idx_dev, idn.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice));
    LCHK(hipMemset(ls->dec_dev, 0, S * sizeof(float)));
  }
  LCHK(hipStreamSynchronize(g->stream));
  GmxRunArgs a;
  memset(&a, 0, sizeof a);
  a.banks = g->banks;
  a.pred = b->d_pred;
  a.mask = b->d_mask;
  a.ctx = b->d_ctx;
  a.bits = b->d_bits;
  a.decay = ls->dec_dev;
  a.decay_idx = ls->idx_dev;
  a.p_out = b->d_p;
  a.out_all = (flags & GMX_BATCH_OUTPUTS) ? b->d_out : nullptr;
  a.latch_out = g->latch_out;
  a.rec_stride = 1;
  a.T = 1;
  a.stream_base = 0;
  a.rec_base = 0;
  a.n_streams = g->S;
  hipStream_t st = g->stream;
  // ---- Predict for every stream: records in, kernel, probabilities out -------------------------
  LCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  {
    hipError_t e = hipMemcpyAsync(b->d_pred, b->h_pred, S * t.n_pad * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_mask, b->h_mask, S * t.mask_words * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_ctx, b->h_ctx, S * t.m * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    a.mode = GMX_MODE_PREDICT | GMX_MODE_LATCH | (g->stock_exact ? GMX_MODE_EXACT : 0u);
    if (e == hipSuccess) e = lockstep_launch_kernel(g, a);
    if (e == hipSuccess) e = hipMemcpyAsync(b->h_p, b->d_p, S * sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && a.out_all) e = hipMemcpyAsync(b->h_out, b->d_out, S * t.m * sizeof(float), hipMemcpyDeviceToHost, st);
    hipError_t e2 = hipStreamEndCapture(st, &ls->g_predict);
    LCHK(e);
    LCHK(e2);
  }
  LCHK(hipGraphInstantiate(&ls->x_predict, ls->g_predict, nullptr, nullptr, 0));
  // ---- Learn for every stream: coded bits and decay factors in, kernel --------------------------
  LCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  {
    hipError_t e = hipMemcpyAsync(b->d_bits, ls->bits_host, S, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ls->dec_dev, ls->dec_host, S * sizeof(float), hipMemcpyHostToDevice, st);
    a.mode = GMX_MODE_LEARN | (g->stock_exact ? GMX_MODE_EXACT : 0u);
    if (e == hipSuccess) e = lockstep_launch_kernel(g, a);
    hipError_t e2 = hipStreamEndCapture(st, &ls->g_learn);
    LCHK(e);
    LCHK(e2);
  }
  LCHK(hipGraphInstantiate(&ls->x_learn, ls->g_learn, nullptr, nullptr, 0));
  // ---- both in one: Learn of the bits just coded, then Predict of the next records ---------------
  // (between Predictor::Learn of bit t and Predictor::Predict of bit t+1 nothing needs the host)
  LCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  {
    hipError_t e = hipMemcpyAsync(b->d_bits, ls->bits_host, S, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ls->dec_dev, ls->dec_host, S * sizeof(float), hipMemcpyHostToDevice, st);
    a.mode = GMX_MODE_LEARN | (g->stock_exact ? GMX_MODE_EXACT : 0u);
    if (e == hipSuccess) e = lockstep_launch_kernel(g, a);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_pred, b->h_pred, S * t.n_pad * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_mask, b->h_mask, S * t.mask_words * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_ctx, b->h_ctx, S * t.m * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    a.mode = GMX_MODE_PREDICT | GMX_MODE_LATCH | (g->stock_exact ? GMX_MODE_EXACT : 0u);
    if (e == hipSuccess) e = lockstep_launch_kernel(g, a);
    if (e == hipSuccess) e = hipMemcpyAsync(b->h_p, b->d_p, S * sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && a.out_all) e = hipMemcpyAsync(b->h_out, b->d_out, S * t.m * sizeof(float), hipMemcpyDeviceToHost, st);
    hipError_t e2 = hipStreamEndCapture(st, &ls->g_step);
    LCHK(e);
    LCHK(e2);
  }
  LCHK(hipGraphInstantiate(&ls->x_step, ls->g_step, nullptr, nullptr, 0));
  // ---- persistent waves instead of graphs, where they apply -------------------------------------
  if ((flags & GMX_LOCKSTEP_PERSISTENT) && group_is_stock(g) && !g->force_general) {
    int large_bar = 0;
    (void)hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, g->device);
    const int cap = gmx_stock_lockstep_capacity(GMX_STK_LDS_BYTES(g->topo.lds_misc), g->device);
    (void)hipGetLastError();
    void* q = nullptr;
    if (large_bar && g->S <= cap && g->S <= kLsPersistentMaxStreams &&
        hipExtMallocWithFlags(&q, sizeof(GmxLsDoor), hipDeviceMallocFinegrained) == hipSuccess) {
      ls->door = (GmxLsDoor*)q;
      LCHK(hipMemset(ls->door, 0, sizeof(GmxLsDoor)));
      LCHK(hipHostMalloc((void**)&ls->done, 64, hipHostMallocMapped | hipHostMallocCoherent));
      memset(ls->done, 0, 64);
      LCHK(hipMalloc((void**)&ls->blk_seen, S * sizeof(uint32_t)));
      LCHK(hipMalloc((void**)&ls->blk_replay, S * sizeof(uint32_t)));
      LCHK(hipMalloc((void**)&ls->relay, 64 * sizeof(uint32_t)));
      LCHK(hipMemset(ls->relay, 0, 64 * sizeof(uint32_t)));
      LCHK(hipMalloc((void**)&ls->live, S * GMX_LS_LIVE_FLOATS * sizeof(float)));
      LCHK(hipMemset(ls->blk_seen, 0, S * sizeof(uint32_t)));
      LCHK(hipMemset(ls->blk_replay, 0, S * sizeof(uint32_t)));
      LCHK(hipMemset(ls->live, 0, S * GMX_LS_LIVE_FLOATS * sizeof(float)));
      LCHK(persistent_stream_create(&ls->ps_stream));
      LCHK(hipDeviceSynchronize());
      ls->persistent = true;
    }
    (void)hipGetLastError();
  }
#undef LCHK
  *out = ls;
  return GMX_OK;
}

extern "C" gmx_batch* gmx_lockstep_batch(gmx_lockstep* ls) { return (ls && ls->g) ? ls->b : nullptr; }
extern "C" int gmx_lockstep_is_persistent(const gmx_lockstep* ls) { return (ls && ls->persistent) ? 1 : 0; }

// Mixer::Predict x M for all S streams with the records in the batch's host arrays; returns when
// the S probabilities (gmx_batch_p) are on the host.
extern "C" int gmx_lockstep_predict(gmx_lockstep* ls) {
  if (!ls || !ls->g) return GMX_ERR_INVALID;
  gmx_group* g = ls->g;
  HIPCHK(hipSetDevice(g->device));
  if (ls->persistent) {
    int rc = ls_persist_ready(ls);
    if (rc) return rc;
    ls_fill_decay(ls, 0);  // latched with the forward
    rc = ls_publish(ls, GMX_MB_FORWARD);
    if (rc) return rc;
    rc = ls_wait(ls);
    if (rc) return rc;
    std::fill(g->fwd_done.begin(), g->fwd_done.end(), 0);
    for (gmx_lockstep* o : g->locksteps) o->predicted = false;
    ls->predicted = true;
    return GMX_OK;
  }
  {
    int rc = sessions_close(g, false);
    if (rc) return rc;
  }
  HIPCHK(hipGraphLaunch(ls->x_predict, g->stream));
  ls->b->x.idle = false;  // (the graph works on the batch's arrays: a download is ordered behind it again)
  HIPCHK(hipStreamSynchronize(g->stream));
  std::fill(g->fwd_done.begin(), g->fwd_done.end(), 0);
  for (gmx_lockstep* o : g->locksteps) o->predicted = false;  // the group has ONE latch: it is this Predict's now
  ls->predicted = true;
  return GMX_OK;
}

// Mixer::Learn x M for all S streams with the coded bits in gmx_batch_bits; asynchronous.
extern "C" int gmx_lockstep_learn(gmx_lockstep* ls) {
  if (!ls || !ls->g) return GMX_ERR_INVALID;
  if (!ls->predicted) return GMX_ERR_STATE;
  gmx_group* g = ls->g;
  HIPCHK(hipSetDevice(g->device));
  for (int s = 0; s < g->S; ++s)
    if (ls->b->h_bits[s] > 1) return GMX_ERR_INVALID;
  if (ls->persistent) {
    int rc = ls_persist_ready(ls);  // (a wave that left since the Predict redoes it from its own copy of the record)
    if (rc) return rc;
    if (!ls->predicted) return GMX_ERR_STATE;  // something else took the banks in between
    for (int s = 0; s < g->S; ++s) ls->bits_host[s] = ls->b->h_bits[s];
    rc = ls_publish(ls, GMX_MB_LEARN0);  // not waited for: the next call on the group does
    if (rc) return rc;
    ls->learn_inflight = true;
    for (int s = 0; s < g->S; ++s) g->steps[s] += 1;
    ls->predicted = false;
    return GMX_OK;
  }
  {  // no per-bit session may hold rows in registers while the graph kernel runs
    int rc = sessions_close(g, false);
    if (rc) return rc;
  }
  // the graph runs later: it reads private copies, so the caller may reuse gmx_batch_bits at once
  for (int s = 0; s < g->S; ++s) ls->bits_host[s] = ls->b->h_bits[s];
  ls_fill_decay(ls, 0);
  HIPCHK(hipGraphLaunch(ls->x_learn, g->stream));
  ls->b->x.idle = false;  // (the graph works on the batch's arrays: a download is ordered behind it again)
  for (int s = 0; s < g->S; ++s) g->steps[s] += 1;
  ls->predicted = false;
  return GMX_OK;
}

// gmx_lockstep_learn with the bits in gmx_batch_bits, then gmx_lockstep_predict with the records in
// the batch's host arrays -- as ONE graph: a decoder's step once the first prediction is out.
// Returns when the new probabilities are on the host.
extern "C" int gmx_lockstep_learn_predict(gmx_lockstep* ls) {
  if (!ls || !ls->g) return GMX_ERR_INVALID;
  if (!ls->predicted) return GMX_ERR_STATE;
  gmx_group* g = ls->g;
  HIPCHK(hipSetDevice(g->device));
  for (int s = 0; s < g->S; ++s)
    if (ls->b->h_bits[s] > 1) return GMX_ERR_INVALID;
  if (ls->persistent) {
    int rc = ls_persist_ready(ls);
    if (rc) return rc;
    if (!ls->predicted) return GMX_ERR_STATE;
    for (int s = 0; s < g->S; ++s) ls->bits_host[s] = ls->b->h_bits[s];
    ls_fill_decay(ls, 1);  // of the NEXT learn: latched with the forward of this command
    rc = ls_publish(ls, GMX_MB_LEARN0_FWD);
    if (rc) return rc;
    for (int s = 0; s < g->S; ++s) g->steps[s] += 1;
    return ls_wait(ls);
  }
  {
    int rc = sessions_close(g, false);
    if (rc) return rc;
  }
  for (int s = 0; s < g->S; ++s) ls->bits_host[s] = ls->b->h_bits[s];
  ls_fill_decay(ls, 0);
  HIPCHK(hipGraphLaunch(ls->x_step, g->stream));
  ls->b->x.idle = false;  // (the graph works on the batch's arrays: a download is ordered behind it again)
  for (int s = 0; s < g->S; ++s) g->steps[s] += 1;
  HIPCHK(hipStreamSynchronize(g->stream));
  return GMX_OK;
}
