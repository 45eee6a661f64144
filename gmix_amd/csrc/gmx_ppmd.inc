// gmx_ppmd.inc -- host side of the PPMd bank (included by gmx_capi.cpp; include/gmxmix_ppmd.h, DESIGN.md section 4.24).
//
// A gmx_ppmd holds S state blocks (GmxPpmdState, gmx_ppmd.h) and S arenas of arena_mb MiB in ONE allocation each, and
// one stream: kernels, record transfers and the per-byte surface's copies all ride on it, as the Match bank's do.
// Nothing of a stream's model lives on the host; gmx_ppmd_memory_usage and gmx_ppmd_restores read the state block.
// Compute is gmx_ppmd.hip; nothing here falls back to the CPU.

struct gmx_ppmd_batch : GmxBatchCore {
  gmx_ppmd* p = nullptr;
  uint64_t& max_bytes = max_rows;
  uint8_t* d_bytes = nullptr;
  float* d_ppm = nullptr;
  float* d_pred = nullptr;
  uint8_t* d_act = nullptr;
  uint64_t* d_used = nullptr;
  uint8_t* h_bytes = nullptr;
  float* h_ppm = nullptr;
  float* h_pred = nullptr;
  uint8_t* h_act = nullptr;
  uint64_t* h_used = nullptr;
};

struct gmx_ppmd {
  int device = 0, S = 0, order = 0, arena_mb = 0;
  uint64_t arena_bytes = 0, arena_stride = 0;
  GmxPpmdState* states = nullptr;  // [S]
  uint8_t* arena = nullptr;        // [S][arena_stride]
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // kernel timing
  GmxBatchBank bb;
  GmxCountList counts;
  // the per-byte surface: staging in, the distributions out
  uint8_t *h_last = nullptr, *d_last = nullptr;  // [2][S]: last_byte, then take
  uint64_t* d_take = nullptr;                    // [S] the step's byte counts (0 / 1), widened on the device's side
  uint64_t* h_take = nullptr;
  float *h_step_ppm = nullptr, *d_step_ppm = nullptr;  // [S][256]
  hipEvent_t ev_step = nullptr;
  bool step_queued = false;
  int64_t launches = 0;
};

static void ppmd_batch_free(gmx_ppmd_batch* b) {
  if (!b) return;
  batch_core_free(*b);
  delete b;
}

extern "C" void gmx_ppmd_destroy(gmx_ppmd* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  batch_bank_detach_all(p->bb);  // shells, as for gmx_batch
  void* dv[] = {p->states, p->arena, p->d_last, p->d_take, p->d_step_ppm};
  for (void* q : dv)
    if (q) (void)hipFree(q);
  void* hv[] = {p->h_last, p->h_take, p->h_step_ppm};
  for (void* q : hv)
    if (q) (void)hipHostFree(q);
  hipEvent_t evs[] = {p->ev0, p->ev1, p->ev_step};
  for (hipEvent_t ev : evs)
    if (ev) (void)hipEventDestroy(ev);
  count_list_free(p->counts);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  (void)hipGetLastError();
  delete p;
}

// New models for streams s0 .. s0 + n - 1: zeroed arenas (the model reads units it never wrote), then Init.
static int ppmd_reset_range(gmx_ppmd* p, int s0, int n) {
  HIPCHK(hipMemsetAsync(p->arena + (size_t)s0 * p->arena_stride, 0, (size_t)n * p->arena_stride, p->stream));
  HIPCHK(gmx_launch_ppmd_init(p->states, p->arena, p->arena_stride, p->arena_bytes, p->order, s0, n, p->stream));
  return GMX_OK;
}

extern "C" int gmx_ppmd_create(gmx_ppmd** out, int n_streams, int order, int arena_mb, int device) {
  if (!out) return GMX_ERR_INVALID;
  *out = nullptr;
  if (n_streams < 1 || order < GMX_PPMD_MIN_ORDER || order > GMX_PPMD_MAX_ORDER || arena_mb < 1 ||
      arena_mb > GMX_PPMD_MAX_ARENA_MB || device < 0)
    return GMX_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return GMX_ERR_NO_DEVICE;
  }
  if (device >= ndev) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(device));
  gmx_ppmd* p = new (std::nothrow) gmx_ppmd();
  if (!p) return GMX_ERR_NOMEM;
  p->device = device;
  p->S = n_streams;
  p->order = order;
  p->arena_mb = arena_mb;
  p->arena_bytes = (uint64_t)arena_mb << 20;
  p->arena_stride = p->arena_bytes + GMX_PPMD_ARENA_SLACK;
  batch_bank_init(p->bb, p, device, &p->stream);
  const size_t S = (size_t)n_streams;
#define PCHK(call)                                           \
  do {                                                       \
    hipError_t e_ = (call);                                  \
    if (e_ != hipSuccess) {                                  \
      int r_ = hip_fail(e_, #call);                          \
      gmx_ppmd_destroy(p);                                   \
      return e_ == hipErrorOutOfMemory ? GMX_ERR_NOMEM : r_; \
    }                                                        \
  } while (0)
  PCHK(bank_stream_create(&p->stream, 1));
  PCHK(hipEventCreate(&p->ev0));
  PCHK(hipEventCreate(&p->ev1));
  PCHK(hipEventCreateWithFlags(&p->ev_step, hipEventDisableTiming));
  PCHK(hipMalloc((void**)&p->arena, S * p->arena_stride));
  PCHK(hipMalloc((void**)&p->states, S * sizeof(GmxPpmdState)));
  PCHK(hipMalloc((void**)&p->d_last, S));
  PCHK(hipMalloc((void**)&p->d_take, S * 8));
  PCHK(hipMalloc((void**)&p->d_step_ppm, S * 1024));
  PCHK(hipHostMalloc((void**)&p->h_last, S, hipHostMallocDefault));
  PCHK(hipHostMalloc((void**)&p->h_take, S * 8, hipHostMallocDefault));
  PCHK(hipHostMalloc((void**)&p->h_step_ppm, S * 1024, hipHostMallocDefault));
  memset(p->h_step_ppm, 0, S * 1024);
#undef PCHK
  int rc = ppmd_reset_range(p, 0, n_streams);
  if (!rc) {
    hipError_t e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
  }
  if (rc) {
    gmx_ppmd_destroy(p);
    return rc;
  }
  *out = p;
  return GMX_OK;
}

extern "C" int gmx_ppmd_n_streams(const gmx_ppmd* p) { return p ? p->S : GMX_ERR_INVALID; }
extern "C" uint64_t gmx_ppmd_bank_bytes(const gmx_ppmd* p) { return p ? p->arena_stride + sizeof(GmxPpmdState) : 0; }
extern "C" int gmx_ppmd_reset(gmx_ppmd* p, int stream) {
  if (!p || stream < -1 || stream >= p->S) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(p->device));
  return stream < 0 ? ppmd_reset_range(p, 0, p->S) : ppmd_reset_range(p, stream, 1);
}
extern "C" int gmx_ppmd_sync(gmx_ppmd* p) {
  if (!p) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipStreamSynchronize(p->stream));
  return GMX_OK;
}

// ---- record batches ------------------------------------------------------------------------
extern "C" int gmx_ppmd_batch_create(gmx_ppmd_batch** out, gmx_ppmd* p, uint64_t max_bytes) {
  if (!out) return GMX_ERR_INVALID;
  *out = nullptr;
  if (!p || max_bytes == 0) return GMX_ERR_INVALID;
  gmx_ppmd_batch* b = new (std::nothrow) gmx_ppmd_batch();
  if (!b) return GMX_ERR_NOMEM;
  b->back = (void**)&b->p;
  gmx_ppmd_batch_cols(b->cols, b);
  int rc = batch_core_alloc(*b, &p->bb, p->S, max_bytes, false);
  if (rc) {
    ppmd_batch_free(b);
    return rc;
  }
  *out = b;
  return GMX_OK;
}
extern "C" void gmx_ppmd_batch_destroy(gmx_ppmd_batch* b) { ppmd_batch_free(b); }
extern "C" uint64_t gmx_ppmd_batch_max_bytes(const gmx_ppmd_batch* b) { return b ? b->max_bytes : 0; }
extern "C" uint8_t* gmx_ppmd_batch_bytes(gmx_ppmd_batch* b) {
  return b ? (uint8_t*)batch_core_host(*b, &b->h_bytes) : nullptr;
}
extern "C" const float* gmx_ppmd_batch_ppm(gmx_ppmd_batch* b) {
  return b ? (const float*)batch_core_host(*b, &b->h_ppm) : nullptr;
}
extern "C" const float* gmx_ppmd_batch_predictions(gmx_ppmd_batch* b) {
  return b ? (const float*)batch_core_host(*b, &b->h_pred) : nullptr;
}
extern "C" const uint8_t* gmx_ppmd_batch_active(gmx_ppmd_batch* b) {
  return b ? (const uint8_t*)batch_core_host(*b, &b->h_act) : nullptr;
}
extern "C" const uint64_t* gmx_ppmd_batch_used(gmx_ppmd_batch* b) {
  return b ? (const uint64_t*)batch_core_host(*b, &b->h_used) : nullptr;
}
extern "C" int gmx_ppmd_batch_upload(gmx_ppmd_batch* b, uint64_t n_bytes) {
  return batch_core_transfer(b, n_bytes, GMX_COL_UP);
}
// The columns `what` names, on the bank's stream behind the kernels that wrote them (ppm is 1 KiB a byte: a caller
// that feeds it on the device, or wants `used` alone, leaves it there).
extern "C" int gmx_ppmd_batch_download(gmx_ppmd_batch* b, uint64_t n_bytes, unsigned what) {
  if (!b || !b->bank || n_bytes > b->max_bytes || (what & ~(unsigned)GMX_PPMD_ALL) || !what) return GMX_ERR_INVALID;
  if (what == GMX_PPMD_ALL) return batch_core_transfer(b, n_bytes, GMX_COL_DOWN);
  if (n_bytes == 0) return GMX_OK;
  HIPCHK(hipSetDevice(b->bank->device));
  const void* skip[3] = {what & GMX_PPMD_PPM ? nullptr : (const void*)&b->h_ppm,
                         what & GMX_PPMD_PREDICTIONS ? nullptr : (const void*)&b->h_pred,
                         what & GMX_PPMD_USED ? nullptr : (const void*)&b->h_used};
  auto wanted = [&](const GmxBatchCol& col) {
    if (col.dir != GMX_COL_DOWN) return false;
    if ((const void*)col.host == (const void*)&b->h_act) return (what & GMX_PPMD_PREDICTIONS) != 0;
    for (const void* k : skip)
      if (k && (const void*)col.host == k) return false;
    return true;
  };
  for (const GmxBatchCol& col : b->cols)
    if (wanted(col) && !batch_core_host(*b, col.host)) return GMX_ERR_NOMEM;
  hipStream_t st = *b->bank->main;
  for (const GmxBatchCol& col : b->cols) {
    if (!wanted(col)) continue;
    const GmxRowCopy r = gmx_row_copy(b->S, b->max_rows, n_bytes, col.row_bytes);
    if (r.height)
      HIPCHK(hipMemcpy2DAsync(*col.host, r.pitch, *col.dev, r.pitch, r.width, r.height, hipMemcpyDeviceToHost, st));
    else
      HIPCHK(hipMemcpyAsync(*col.host, *col.dev, r.bytes, hipMemcpyDeviceToHost, st));
  }
  return xfer_end_download(b->x, st);
}
extern "C" int gmx_ppmd_batch_wait(gmx_ppmd_batch* b) { return batch_core_wait(b); }

// ---- compute -------------------------------------------------------------------------------
static int ppmd_launch(gmx_ppmd* p, gmx_ppmd_batch* b, uint64_t n, const uint64_t* n_list, float* kernel_ms) {
  GmxPpmdRunArgs a;
  memset(&a, 0, sizeof a);
  a.states = p->states;
  a.arena = p->arena;
  a.arena_stride = p->arena_stride;
  a.bytes = b->d_bytes;
  a.byte_pitch = b->max_bytes;
  a.n = n;
  a.ppm_out = b->d_ppm;
  a.pred_out = b->d_pred;
  a.act_out = b->d_act;
  a.used_out = b->d_used;
  a.rec_pitch = b->max_bytes;
  if (n_list) {
    int rcl = count_list_stage(p->counts, n_list, p->S, p->stream, &a.n_list);
    if (rcl) return rcl;
  }
  {
    int rcx = xfer_before_run(b->x, p->stream);
    if (rcx) return rcx;
  }
  if (kernel_ms) HIPCHK(hipEventRecord(p->ev0, p->stream));
  HIPCHK(gmx_launch_ppmd_run(&a, p->S, p->stream));
  p->launches++;
  if (n_list) {
    int rcl = count_list_used(p->counts, p->stream);
    if (rcl) return rcl;
  }
  {
    int rcx = xfer_note_device_use(b->x, p->stream);
    if (rcx) return rcx;
  }
  if (kernel_ms) {
    HIPCHK(hipEventRecord(p->ev1, p->stream));
    HIPCHK(hipEventSynchronize(p->ev1));
    HIPCHK(hipEventElapsedTime(kernel_ms, p->ev0, p->ev1));
  }
  return GMX_OK;
}

extern "C" int gmx_ppmd_run(gmx_ppmd* p, gmx_ppmd_batch* b, uint64_t n_bytes, float* kernel_ms) {
  if (!p || !b || b->p != p || n_bytes > b->max_bytes) return GMX_ERR_INVALID;
  if (kernel_ms) *kernel_ms = 0.0f;
  if (n_bytes == 0) return GMX_OK;
  HIPCHK(hipSetDevice(p->device));
  return ppmd_launch(p, b, n_bytes, nullptr, kernel_ms);
}

extern "C" int gmx_ppmd_run_ragged(gmx_ppmd* p, gmx_ppmd_batch* b, const uint64_t* n_bytes) {
  if (!p || !b || b->p != p || !n_bytes) return GMX_ERR_INVALID;
  uint64_t maxn = 0;
  for (int s = 0; s < p->S; ++s) {
    if (n_bytes[s] > b->max_bytes) return GMX_ERR_INVALID;
    maxn = std::max(maxn, n_bytes[s]);
  }
  if (maxn == 0) return GMX_OK;
  HIPCHK(hipSetDevice(p->device));
  return ppmd_launch(p, b, 0, n_bytes, nullptr);
}

extern "C" int gmx_ppmd_feed(gmx_ppmd* p, gmx_ppmd_batch* b, uint64_t n_bytes, gmx_lstm_batch* lstm_batch,
                             gmx_batch* mixer_batch, int slot) {
  if (!p || !b || b->p != p || n_bytes > b->max_bytes || (!lstm_batch && !mixer_batch)) return GMX_ERR_INVALID;
  GmxPpmdFeedArgs a;
  memset(&a, 0, sizeof a);
  a.ppm = b->d_ppm;
  a.pred = b->d_pred;
  a.act = b->d_act;
  a.rec_pitch = b->max_bytes;
  a.n_bytes = n_bytes;
  if (lstm_batch) {
    gmx_lstm_batch* lb = lstm_batch;
    if (!lb->l || lb->S != p->S || lb->l->device != p->device || n_bytes > lb->max_bytes) return GMX_ERR_INVALID;
    a.lstm_ppm = lb->d_ppm;
    a.lstm_pitch = lb->max_bytes;
  }
  if (mixer_batch) {
    gmx_batch* m = mixer_batch;
    if (!m->g || m->S != p->S || m->g->device != p->device || n_bytes * 8 > m->max_bits || !(m->flags & GMX_BATCH_MASK) ||
        !m->d_mask || slot < 0 || slot >= m->g->topo.n)
      return GMX_ERR_INVALID;
    a.mx_pred = m->d_pred;
    a.mx_mask = m->d_mask;
    a.mx_pitch = m->max_bits;
    a.mx_n_pad = m->g->topo.n_pad;
    a.mx_mask_words = m->g->topo.mask_words;
    a.slot = slot;
  }
  if (n_bytes == 0) return GMX_OK;
  HIPCHK(hipSetDevice(p->device));
  // behind the targets' own uploads and last uses, in front of their next work (as gmx_lstm_feed)
  hipStream_t fs = p->stream;
  if (lstm_batch) {
    int rcw = xfer_writer_waits(lstm_batch->x, fs);
    if (rcw) return rcw;
  }
  if (mixer_batch) {
    int rcw = xfer_writer_waits(mixer_batch->x, fs);
    if (rcw) return rcw;
  }
  HIPCHK(gmx_launch_ppmd_feed(&a, p->S, fs));
  if (lstm_batch) {
    int rcn = xfer_writer_done(lstm_batch->x, fs, lstm_batch->l->stream);
    if (rcn) return rcn;
  }
  if (mixer_batch) {
    int rcn = xfer_writer_done(mixer_batch->x, fs, mixer_batch->g->stream);
    if (rcn) return rcn;
  }
  return xfer_note_device_use(b->x, fs);  // the feed read this batch's results
}

// ---- the per-byte surface ------------------------------------------------------------------
extern "C" int gmx_ppmd_step_launch(gmx_ppmd* p, const uint8_t* last_byte, const uint8_t* take) {
  if (!p || !last_byte || !take) return GMX_ERR_INVALID;
  if (p->step_queued) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(p->device));
  const size_t S = (size_t)p->S;
  bool any = false;
  for (size_t s = 0; s < S; ++s) {
    p->h_last[s] = last_byte[s];
    p->h_take[s] = take[s] ? 1 : 0;
    any = any || take[s];
  }
  if (any) {
    hipStream_t st = p->stream;
    HIPCHK(hipMemcpyAsync(p->d_last, p->h_last, S, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(p->d_take, p->h_take, S * 8, hipMemcpyHostToDevice, st));
    GmxPpmdRunArgs a;
    memset(&a, 0, sizeof a);
    a.states = p->states;
    a.arena = p->arena;
    a.arena_stride = p->arena_stride;
    a.bytes = p->d_last;
    a.byte_pitch = 1;
    a.n_list = p->d_take;
    a.ppm_out = p->d_step_ppm;
    a.rec_pitch = 1;
    a.explicit_last = 1;
    HIPCHK(gmx_launch_ppmd_run(&a, p->S, st));
    p->launches++;
    // (the rows of the streams that sat out keep their last distribution on both sides)
    HIPCHK(hipMemcpyAsync(p->h_step_ppm, p->d_step_ppm, S * 1024, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipEventRecord(p->ev_step, p->stream));
  p->step_queued = true;
  return GMX_OK;
}
extern "C" int gmx_ppmd_step_wait(gmx_ppmd* p) {
  if (!p) return GMX_ERR_INVALID;
  if (!p->step_queued) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipEventSynchronize(p->ev_step));
  p->step_queued = false;
  return GMX_OK;
}
extern "C" int gmx_ppmd_step(gmx_ppmd* p, const uint8_t* last_byte, const uint8_t* take) {
  const int rc = gmx_ppmd_step_launch(p, last_byte, take);
  return rc ? rc : gmx_ppmd_step_wait(p);
}
extern "C" const float* gmx_ppmd_step_ppm(gmx_ppmd* p) { return p ? p->h_step_ppm : nullptr; }

// ---- what the model holds ------------------------------------------------------------------
static int ppmd_read_state(gmx_ppmd* p, int stream, GmxPpmdState* st) {
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipStreamSynchronize(p->stream));
  HIPCHK(hipMemcpy(st, p->states + stream, sizeof *st, hipMemcpyDeviceToHost));
  return GMX_OK;
}
extern "C" uint64_t gmx_ppmd_memory_usage(gmx_ppmd* p, int stream) {
  if (!p || stream < 0 || stream >= p->S) return 0;
  GmxPpmdState st;
  if (ppmd_read_state(p, stream, &st)) return 0;
  return 16 + gmx_ppmd_used_memory(&st);
}
extern "C" int64_t gmx_ppmd_restores(gmx_ppmd* p, int stream) {
  if (!p || stream < 0 || stream >= p->S) return -1;
  GmxPpmdState st;
  if (ppmd_read_state(p, stream, &st)) return -1;
  return (int64_t)st.restores;
}
extern "C" int64_t gmx_debug_ppmd_launches(gmx_ppmd* p) { return p ? p->launches : (int64_t)GMX_ERR_INVALID; }
