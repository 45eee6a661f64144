// gmx_session.inc -- host side of the per-bit sessions (included by gmx_capi.cpp).
//
// gmx_bank_forward / gmx_bank_learn on a bank of the reference's own shape do not launch a
// kernel per call: the first call starts gmx_stock_session_kernel (gmx_stock.hip), one
// persistent wave that takes commands from a mailbox and keeps the bit's state in registers
// between forward and learn.  gmx_bank_learn only notes the bit: it travels with the next
// forward as one LEARN*_FWD command (Predictor::Learn of bit t and Predictor::Predict of bit t+1
// have nothing between them that needs the device), so a coded bit costs one round trip; anything
// else that needs the bank up to date sends the noted learn on its own first.  The command half
// of the mailbox lives in device memory when the host can store there (large BAR), so the wave
// polls and reads locally.  Any other operation on the group (batched run, export, import, copy,
// reset, destroy) first stops the sessions, which writes their rows back.  A session that sees
// no command for kIdleTicks leaves by itself; the next call relaunches it (with a replay of the
// forward if its learn is still to come).
//
// A persistent kernel occupies the hardware queue its stream maps to, and a process has only
// a few of those, so at most kMaxOpenSessions sessions are open per process: opening another
// one in the same group stops the least recently used, and a group that cannot get one uses
// the two-launch path for that call.
//
// The protocol itself (command word, wait with restart and bounded time-out, the count of open sessions) is
// gmx_mailbox.h, which needs no HIP; the HIP half that every kind of session has (GmxSessionHw: the blocks and the
// stream, start prologue, stop, release) comes first below and also serves gmx_indirect.inc and gmx_lstm.inc.

static_assert(kMbStop == GMX_MB_STOP && kMbSlotShift == GMX_MB_SLOT_SHIFT && kMbSeqShift == GMX_MB_SEQ_SHIFT &&
                  kMbRunning == GMX_MB_RUNNING && kMbExitIdle == GMX_MB_EXIT_IDLE,
              "gmx_mailbox.h and the kernels speak the same protocol");
static const long kSessionTimeoutS = 10;

// ---- the HIP half of a session, the same for the mixers, the Indirect models and the LSTM -------------------
// The protocol state (gmx_mailbox.h) with the two blocks it points into and the stream its wave lives on.  A bank's
// own session struct derives from this and adds the typed pointers to its blocks and what it keeps per payload.
struct GmxSessionHw : GmxMailbox {
  bool mc_on_device = false;     // the command block is device memory (else pinned host memory)
  hipStream_t stream = nullptr;
};
#define GMX_MB_LAYOUT_CHECK(Cmd, Reply)                                                                       \
  static_assert(offsetof(Cmd, cmd_seq) == 0 && offsetof(Reply, done_seq) == 0 && offsetof(Reply, state) == 4, \
                #Cmd " / " #Reply ": the words GmxMailbox points at")
GMX_MB_LAYOUT_CHECK(GmxMbCmd, GmxMbReply);
GMX_MB_LAYOUT_CHECK(GmxIndMbCmd, GmxIndMbReply);
GMX_MB_LAYOUT_CHECK(GmxLstmMbCmd, GmxLstmMbReply);

// The stream a persistent kernel lives on.  The runtime maps streams onto a handful of hardware queues per
// priority level (four by default), and a kernel that does not end blocks everything queued behind it on ITS
// hardware queue: two sessions that happened to share one took turns by their 20 ms idle timers (measured: 40 ms
// per bit for an Indirect and a mixer session side by side, 28 us with more queues), and any ordinary launch
// could end up behind one.  Persistent kernels therefore get streams of the HIGHEST priority: a pool of hardware
// queues of their own, shared by nothing but the at most kMaxOpenSessions persistent kernels of the process.
static hipError_t persistent_stream_create(hipStream_t* out) {
  int least = 0, greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e != hipSuccess) return e;
  return hipStreamCreateWithPriority(out, hipStreamNonBlocking, greatest);
}

// The reply block (mapped, coherent: host pointer == device pointer), the command block and the stream.  The command
// block is device memory if the host can store into it and the caller allows it (measured on MI355X,
// scripts/probe_bar_mailbox.hip: 3.0 us per round trip instead of 4.5), else pinned host memory.
static int session_hw_alloc(GmxSessionHw* h, size_t cmd_bytes, size_t reply_bytes, bool allow_bar, int device) {
  void* p = nullptr;
  HIPCHK(hipHostMalloc(&p, reply_bytes, hipHostMallocMapped | hipHostMallocCoherent));
  memset(p, 0, reply_bytes);
  h->done_seq = (uint32_t*)p;
  h->state = h->done_seq + 1;
  int large_bar = 0;
  if (allow_bar && hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, device) == hipSuccess && large_bar) {
    void* q = nullptr;
    if (hipExtMallocWithFlags(&q, cmd_bytes, hipDeviceMallocFinegrained) == hipSuccess) {
      if (hipMemset(q, 0, cmd_bytes) == hipSuccess) {
        h->cmd_seq = (uint32_t*)q;
        h->mc_on_device = true;
      } else {
        (void)hipFree(q);
      }
    }
    (void)hipGetLastError();
  }
  if (!h->cmd_seq) {
    HIPCHK(hipHostMalloc(&p, cmd_bytes, hipHostMallocMapped | hipHostMallocCoherent));
    memset(p, 0, cmd_bytes);
    h->cmd_seq = (uint32_t*)p;
  }
  HIPCHK(persistent_stream_create(&h->stream));
  return GMX_OK;
}

// What every (re)start does before it launches the next instance; the previous one, if any, has left or is leaving.
static int session_hw_start_prologue(GmxSessionHw* h) {
  if (h->launched) {
    HIPCHK(hipStreamSynchronize(h->stream));
  } else {
    g_open_sessions.fetch_add(1);
  }
  __atomic_store_n(h->state, GMX_MB_RUNNING, __ATOMIC_RELEASE);
  h->launched = true;
  return GMX_OK;
}

// Stop the wave, if one was launched; `wait` is the bank's own wait for the newest command.
template <class Wait>
static int session_hw_stop(GmxSessionHw* h, Wait&& wait) {
  if (!h->launched) return GMX_OK;
  int rc = wait();
  if (rc) return rc;
  if (mb_load(h->state) == GMX_MB_RUNNING) mb_publish_stop(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  // an instance that left on its idle timer at that very moment never saw the STOP: mark it
  // consumed so that the next instance does not take it for a new command
  __atomic_store_n(h->done_seq, h->word, __ATOMIC_RELEASE);
  h->launched = false;
  g_open_sessions.fetch_sub(1);
  return GMX_OK;
}

// Free the stream and the blocks of a stopped session.  The wave of a dead one may still be polling: wait a bounded
// time for it, and if it is still there leave everything allocated rather than free memory a running kernel reads
// and writes.  False: it is still there -- and the caller must not free the banks it works on either.
static bool session_hw_release(GmxSessionHw* h) {
  if (h->dead && h->stream) {
    bool gone = false;
    for (int i = 0; i < 1000 && !gone; ++i) {
      gone = hipStreamQuery(h->stream) == hipSuccess;
      if (!gone) {
        timespec ts = {0, 1000000};
        nanosleep(&ts, nullptr);
      }
    }
    (void)hipGetLastError();
    if (!gone) return false;
  } else if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
  }
  if (h->stream) (void)hipStreamDestroy(h->stream);
  if (h->cmd_seq && h->mc_on_device) (void)hipFree(h->cmd_seq);
  if (h->cmd_seq && !h->mc_on_device) (void)hipHostFree(h->cmd_seq);
  if (h->done_seq) (void)hipHostFree(h->done_seq);
  return true;
}

// A bank's sessions, all of them.  Stop: every session is attempted; the first failure is what the caller sees.
template <class Stop>
static int sessions_stop_each(size_t n, Stop&& stop) {
  int first = GMX_OK;
  for (size_t s = 0; s < n; ++s) {
    int rc = stop((int)s);
    if (rc && !first) first = rc;
  }
  return first;
}
// Release: false if the wave of a dead one is still there (the bank then leaks what that wave works on).
template <class Se>
static bool sessions_release_each(std::vector<Se*>& sessions) {
  bool gone = true;
  for (Se* se : sessions) {
    if (!se) continue;
    if (!session_hw_release(se)) gone = false;
    delete se;
  }
  sessions.clear();
  return gone;
}

// ---- the mixers' sessions ------------------------------------------------------------------------------------
struct GmxSession : GmxSessionHw {
  GmxMbCmd* mc = nullptr;        // commands: fine-grained device memory (host stores through the BAR) or pinned host memory
  GmxMbReply* mb = nullptr;      // replies: host pointer == device pointer (mapped, coherent)
  uint32_t slot = 0;             // payload slot of the newest forward published
  uint32_t live_slot = 0;        // payload slot of the newest forward COMPLETED (the one a restart replays)
  int pending_learn = 0;         // 1 + bit: gmx_bank_learn noted, not yet published
  bool fwd_live = false;         // a forward has completed whose learn has not (replay on restart)
  bool learn_inflight = false;   // the newest command is that learn, on its own
  uint64_t last_use = 0;
};

extern "C" hipError_t gmx_launch_stock_session(const GmxTopoDev* tp_dev, uint8_t* banks, int stream_idx,
                                               GmxMbCmd* mc, GmxMbReply* mr, unsigned long long idle_ticks,
                                               int replay_forward, int exact, unsigned lds_bytes,
                                               hipStream_t stream);

static std::atomic<uint64_t> g_session_clock{0};

static bool group_is_stock(const gmx_group* g) {
  const GmxTopoDev& t = g->topo;
  return t.n == 90 && t.l0 == 24 && t.l1 == 8 && t.n_skip == 1 && t.has_final && t.mx[23].stride == 128;
}

static void session_note_done(GmxSession* se) {
  if (se->learn_inflight && mb_load(se->done_seq) == se->word) {
    se->learn_inflight = false;
    se->fwd_live = false;
  }
}

// (Re)start the wave of session s; the previous instance, if any, has left or is leaving.
static int session_start(gmx_group* g, int s) {
  GmxSession* se = g->sessions[s];
  int rc = session_hw_start_prologue(se);
  if (rc) return rc;
  session_note_done(se);
  HIPCHK(gmx_launch_stock_session(g->topo_dev, g->banks, s, se->mc, se->mb, kIdleTicks,
                                  se->fwd_live ? 1 + (int)se->live_slot : 0, g->stock_exact ? 1 : 0,
                                  GMX_STK_LDS_BYTES(g->topo.lds_misc), se->stream));
  return GMX_OK;
}

static int session_dead(GmxSession* se) {
  g_last_error = "per-bit session does not answer";
  se->pending_learn = 0;
  se->fwd_live = false;
  return GMX_ERR_HIP;
}

// Wait until the newest command has been completed, restarting the session if it left first.
static int session_wait(gmx_group* g, int s) {
  GmxSession* se = g->sessions[s];
  int rc = mb_wait(se, kSessionTimeoutS, [&] { return session_start(g, s); });
  if (rc) return rc == kMbDead ? session_dead(se) : rc;
  session_note_done(se);
  return GMX_OK;
}

static int session_ensure(gmx_group* g, int s, bool force);

// A learn that gmx_bank_learn noted and no forward has taken along yet: send it on its own.
static int session_flush_learn(gmx_group* g, int s) {
  GmxSession* se = s < (int)g->sessions.size() ? g->sessions[s] : nullptr;
  if (!se || !se->pending_learn) return GMX_OK;
  int rc = session_ensure(g, s, true);  // restarts (with replay) a session that left after the forward
  if (rc) return rc;
  const int bit = se->pending_learn - 1;
  se->pending_learn = 0;
  se->learn_inflight = true;
  mb_publish(se, se->slot, bit ? GMX_MB_LEARN1 : GMX_MB_LEARN0);  // not waited for: the next command does that
  return GMX_OK;
}

// Stop session s: its rows and counters go back to HBM.  The forward state survives in the
// mailbox (fwd_live) unless the caller is about to change the bank.
static int session_stop(gmx_group* g, int s, bool keep_forward) {
  GmxSession* se = s < (int)g->sessions.size() ? g->sessions[s] : nullptr;
  if (!se) return GMX_OK;
  if (se->dead) return session_dead(se);
  int rc = session_flush_learn(g, s);
  if (rc) return rc;
  rc = session_hw_stop(se, [&] { return session_wait(g, s); });
  if (rc) return rc;
  if (!keep_forward) se->fwd_live = false;
  return GMX_OK;
}

static int sessions_close_perbit(gmx_group* g, bool keep_forward) {
  return sessions_stop_each(g->sessions.size(), [&](int s) { return session_stop(g, s, keep_forward); });
}

// Nothing may hold rows in registers while something else works on the banks: the per-bit sessions and the
// persistent lock-step waves (gmx_lockstep.inc) hand them back.
static int sessions_close(gmx_group* g, bool keep_forward) {
  int first = sessions_close_perbit(g, keep_forward);
  int rc = locksteps_stop(g, nullptr, keep_forward);
  return first ? first : rc;
}

static void sessions_free(gmx_group* g) {
  (void)sessions_close(g, false);
  // (a wave that is still there has its rows in the group's banks: gmx_group_destroy leaks them)
  if (!sessions_release_each(g->sessions)) g->banks_in_use_by_dead_kernel = true;
}

// Make sure session s exists and runs.  GMX_ERR_STATE: no session slot available (the caller
// falls back to the two-launch path); `force` takes one beyond the limit instead (a learn
// whose forward went through a session has no other way).
static int session_ensure(gmx_group* g, int s, bool force) {
  if (g->sessions.empty()) g->sessions.assign(g->S, nullptr);
  GmxSession* se = g->sessions[s];
  if (se && se->dead) return session_dead(se);
  const bool running = se && se->launched && mb_load(se->state) == GMX_MB_RUNNING;
  if (!running && !(se && se->launched) && g_open_sessions.load() >= kMaxOpenSessions) {
    int victim = -1;
    for (int i = 0; i < g->S; ++i) {
      GmxSession* o = g->sessions[i];
      if (i != s && o && o->launched && (victim < 0 || o->last_use < g->sessions[victim]->last_use))
        victim = i;
    }
    if (victim < 0 && !force) return GMX_ERR_STATE;
    if (victim >= 0) {
      int rc = session_stop(g, victim, true);
      if (rc) return rc;
    }
  }
  if (!se) {
    se = new (std::nothrow) GmxSession();
    if (!se) return GMX_ERR_NOMEM;
    g->sessions[s] = se;
    int rc = session_hw_alloc(se, sizeof(GmxMbCmd), sizeof(GmxMbReply), g->mailbox_on_device, g->device);
    se->mc = (GmxMbCmd*)se->cmd_seq;
    se->mb = (GmxMbReply*)se->done_seq;
    if (rc) return rc;
  }
  se->last_use = g_session_clock.fetch_add(1) + 1;
  if (!running) {
    HIPCHK(hipStreamSynchronize(g->stream));  // batched work on the banks is finished
    return session_start(g, s);
  }
  return GMX_OK;
}

// A forward up to ringing the doorbell: the payload is in its slot and se->word is its command word (with the
// learn gmx_bank_learn noted, if any).  `not_yet`: bits of the active mask somebody else fills in later (the
// Indirect models' slots of a chained forward), cleared here.
static int session_forward_prepare(gmx_group* g, int s, const float* predictions, const int32_t* active_models,
                                   int n_active, const uint32_t* contexts, const uint32_t* not_yet) {
  const GmxTopoDev& t = g->topo;
  uint32_t m[4] = {0, 0, 0, 0};
  if (n_active < 0) {
    m[0] = m[1] = m[2] = 0xffffffffu;
  } else {
    for (int i = 0; i < n_active; ++i) {
      const int idx = active_models[i];
      if (idx < 0 || idx >= t.n) return GMX_ERR_INVALID;
      m[idx >> 5] |= 1u << (idx & 31);
    }
  }
  if (not_yet)
    for (int w = 0; w < 4; ++w) m[w] &= ~not_yet[w];
  {
    // a noted learn rides along only if the wave that made its forward is still there; after an
    // idle exit the learn goes first, on its own, through the replay path
    GmxSession* se0 = s < (int)g->sessions.size() ? g->sessions[s] : nullptr;
    if (se0 && se0->pending_learn && !(se0->launched && mb_load(se0->state) == GMX_MB_RUNNING)) {
      int rc = session_flush_learn(g, s);
      if (rc) return rc;
    }
  }
  int rc = locksteps_stop(g, nullptr, false);  // persistent lock-step waves hand the banks back first
  if (rc) return rc;
  rc = session_ensure(g, s, false);
  if (rc) return rc;
  // a lock-step Predict's latch does not survive per-bit traffic on the same banks: its Learn must not
  // run the graph kernel on rows this session now holds in registers
  for (gmx_lockstep* ls : g->locksteps) ls->predicted = false;
  GmxSession* se = g->sessions[s];
  rc = session_wait(g, s);  // the previous command is done with its payload slot
  if (rc) return rc;
  // the other payload slot: the one of the forward still waiting for its learn stays intact
  se->slot ^= 1u;
  GmxMbPayload* pay = &se->mc->slot[se->slot];
  GmxMbPayload img;
  memset(&img, 0, sizeof img);
  memcpy(img.pred, predictions, t.n * sizeof(float));
  memcpy(img.mask, m, sizeof m);
  memcpy(img.ctx, contexts, t.m * sizeof(uint32_t));
  const float dec = decay_base(g->steps[s]);
  memcpy(&img.dec_bits, &dec, 4);
  memcpy(pay, &img, sizeof img);  // one sequential burst (write-combined when `pay` is behind the BAR)
  uint32_t cmd = GMX_MB_FORWARD;
  if (se->pending_learn) {
    cmd = se->pending_learn == 2 ? GMX_MB_LEARN1_FWD : GMX_MB_LEARN0_FWD;
    se->pending_learn = 0;
  }
  mb_next_word(se, se->slot, cmd);
  return GMX_OK;
}

// ... and from the moment the doorbell has been rung: wait for the answer, take the results.
static int session_forward_finish(gmx_group* g, int s, float* p_final, float* out_all) {
  GmxSession* se = g->sessions[s];
  int rc = session_wait(g, s);
  if (rc) return rc;
  se->fwd_live = true;
  se->live_slot = se->slot;
  if (p_final) *p_final = se->mb->p;
  if (out_all) memcpy(out_all, se->mb->outs, g->topo.m * sizeof(float));
  return GMX_OK;
}

static int session_forward(gmx_group* g, int s, const float* predictions, const int32_t* active_models,
                           int n_active, const uint32_t* contexts, float* p_final, float* out_all) {
  int rc = session_forward_prepare(g, s, predictions, active_models, n_active, contexts, nullptr);
  if (rc) return rc;
  mb_ring(g->sessions[s]);
  return session_forward_finish(g, s, p_final, out_all);
}

static int session_learn(gmx_group* g, int s, int bit) {
  GmxSession* se = s < (int)g->sessions.size() ? g->sessions[s] : nullptr;
  if (!se || !se->fwd_live || se->pending_learn) return GMX_ERR_STATE;
  se->pending_learn = 1 + (bit ? 1 : 0);
  g->steps[s] += 1;
  return GMX_OK;
}
