// gmx_analysis.inc -- the analysis averages on the device: per-model entropy averages out of a batch (included by
// gmx_capi.cpp; include/gmxmix_analysis.h, DESIGN.md section 4.23).
//
// A gmx_analysis holds the reference's entropy[] for S streams x C columns, a rows area of max_samples x C averages and
// max_samples labels per stream, and a pinned buffer the take's kernel packs into.  bits_seen, the rows captured since
// the last take and the sample frequency of every stream live in the host's mirror, which is exact -- they depend on
// the counts of the calls alone -- and travel to a launch in its staged list.  It reads a gmx_batch's device arrays on
// the batch's group's stream, right behind the kernel that wrote them, or host arrays on a stream of its own; one event
// orders its work across the two.

struct gmx_analysis {
  int device = 0, S = 0, C = 0;
  uint64_t max_samples = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_last = nullptr;   // behind the newest work on the device state, whatever stream it ran on
  hipEvent_t ev_stage = nullptr;  // behind the newest kernel that read the staging arrays below
  hipEvent_t tm0 = nullptr, tm1 = nullptr;
  bool last_rec = false, last_own = false, stage_rec = false;
  std::vector<gmx_analysis_column> cols;
  uint32_t* d_cols = nullptr;
  double* d_ema = nullptr;
  double* d_rows = nullptr;
  uint64_t* d_labels = nullptr;
  GmxCountList lists;
  // the host's mirror
  std::vector<uint64_t> seen, rows, freq;
  // gmx_analysis_update's copies of the caller's arrays (lazily, grown on demand), gmx_analysis_reset's averages
  float *d_val = nullptr, *h_val = nullptr;
  uint8_t *d_bits = nullptr, *h_bits = nullptr;
  size_t stage_bits = 0;          // bits per stream the staging arrays hold
  double *d_set = nullptr, *h_set = nullptr;
  // the take
  uint8_t *h_pack = nullptr, *h_pack_dev = nullptr;
  size_t body_off = 0;
  bool take_queued = false, taken = false;
  int64_t d2h = 0;
  std::vector<uint64_t> q_seen, q_rows, q_off;  // of the take in flight
  std::vector<uint64_t> t_seen, t_rows, t_off;  // of the last take
};

static uint64_t an_line_up(uint64_t n) { return (n + (GMX_AN_LINE - 1)) & ~(uint64_t)(GMX_AN_LINE - 1); }
static uint64_t an_section_bytes(const gmx_analysis* a, uint64_t n_rows) {
  return 8ull * (uint64_t)a->C + 8ull * ((uint64_t)a->C + 1) * n_rows;
}

// Work on the object's device state is about to be queued on `st` / has been.
static int an_begin(gmx_analysis* a, hipStream_t st) {
  if (a->last_rec && !(a->last_own && st == a->stream)) HIPCHK(hipStreamWaitEvent(st, a->ev_last, 0));
  return GMX_OK;
}
static int an_end(gmx_analysis* a, hipStream_t st) {
  HIPCHK(hipEventRecord(a->ev_last, st));
  a->last_rec = true;
  a->last_own = st == a->stream;
  return GMX_OK;
}
static int an_stage_free(gmx_analysis* a) {
  if (a->stage_rec) HIPCHK(hipEventSynchronize(a->ev_stage));
  a->stage_rec = false;
  return GMX_OK;
}
static int an_stage_used(gmx_analysis* a) {
  HIPCHK(hipEventRecord(a->ev_stage, a->stream));
  a->stage_rec = true;
  return GMX_OK;
}
// The counts of a call: within `limit`, and no stream captures beyond its rows area.  Nothing is written.
static bool an_counts_fit(const gmx_analysis* a, const uint64_t* n_bits, uint64_t limit) {
  for (int s = 0; s < a->S; ++s) {
    if (n_bits[s] > limit) return false;
    if (a->rows[s] + gmx_an_captures(a->seen[s], a->freq[s], n_bits[s]) > a->max_samples) return false;
  }
  return true;
}
// The launch's list from the mirror, the kernel, and the mirror's step.
static int an_launch(gmx_analysis* a, GmxAnArgs* k, const uint64_t* n_bits, hipStream_t st, float* kernel_ms) {
  const size_t S = (size_t)a->S;
  std::vector<uint64_t> list(GMX_AN_L_COUNT * S);
  for (size_t s = 0; s < S; ++s) {
    list[GMX_AN_L_NBITS * S + s] = n_bits[s];
    list[GMX_AN_L_SEEN * S + s] = a->seen[s];
    list[GMX_AN_L_ROWS * S + s] = a->rows[s];
    list[GMX_AN_L_FREQ * S + s] = a->freq[s];
  }
  k->ema = a->d_ema;
  k->rows = a->d_rows;
  k->labels = a->d_labels;
  k->cols = a->d_cols;
  k->n_columns = (uint32_t)a->C;
  k->max_samples = (uint32_t)a->max_samples;
  k->n_streams = a->S;
  int rc = an_begin(a, st);
  if (rc) return rc;
  rc = count_list_stage(a->lists, list.data(), (int)list.size(), st, &k->list);
  if (rc) return rc;
  if (kernel_ms) HIPCHK(hipEventRecord(a->tm0, st));
  HIPCHK(gmx_launch_analysis(k, st));
  if (kernel_ms) HIPCHK(hipEventRecord(a->tm1, st));
  rc = count_list_used(a->lists, st);
  if (rc) return rc;
  for (size_t s = 0; s < S; ++s) {
    a->rows[s] += gmx_an_captures(a->seen[s], a->freq[s], n_bits[s]);
    a->seen[s] += n_bits[s];
  }
  return GMX_OK;
}

extern "C" void gmx_analysis_destroy(gmx_analysis* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  if (a->last_rec) (void)hipEventSynchronize(a->ev_last);
  if (a->stage_rec) (void)hipEventSynchronize(a->ev_stage);
  if (a->stream) (void)hipStreamSynchronize(a->stream);
  count_list_free(a->lists);
  void* dv[] = {a->d_cols, a->d_ema, a->d_rows, a->d_labels, a->d_val, a->d_bits, a->d_set};
  for (void* q : dv)
    if (q) (void)hipFree(q);
  void* hv[] = {a->h_val, a->h_bits, a->h_set, a->h_pack};
  for (void* q : hv)
    if (q) (void)hipHostFree(q);
  hipEvent_t evs[] = {a->ev_last, a->ev_stage, a->tm0, a->tm1};
  for (hipEvent_t ev : evs)
    if (ev) (void)hipEventDestroy(ev);
  if (a->stream) (void)hipStreamDestroy(a->stream);
  (void)hipGetLastError();
  delete a;
}

extern "C" int gmx_analysis_create(gmx_analysis** out, int n_streams, const gmx_analysis_column* cols, int n_columns,
                                   uint64_t max_samples, int device) {
  if (!out) return GMX_ERR_INVALID;
  *out = nullptr;
  if (n_streams < 1 || !cols || n_columns < 1 || n_columns > 512 || max_samples > (1ull << 20) || device < 0)
    return GMX_ERR_INVALID;
  for (int c = 0; c < n_columns; ++c)
    if (cols[c].kind > GMX_AN_FINAL_P) return GMX_ERR_INVALID;
  int n_dev = 0;
  HIPCHK(hipGetDeviceCount(&n_dev));
  if (device >= n_dev) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(device));
  gmx_analysis* a = new (std::nothrow) gmx_analysis();
  if (!a) return GMX_ERR_NOMEM;
  a->device = device;
  a->S = n_streams;
  a->C = n_columns;
  a->max_samples = max_samples;
  a->cols.assign(cols, cols + n_columns);
  const size_t S = (size_t)n_streams, C = (size_t)n_columns, R = (size_t)(max_samples ? max_samples : 1);
#define ACHK(call)                                           \
  do {                                                       \
    hipError_t e_ = (call);                                  \
    if (e_ != hipSuccess) {                                  \
      int r_ = hip_fail(e_, #call);                          \
      gmx_analysis_destroy(a);                               \
      return e_ == hipErrorOutOfMemory ? GMX_ERR_NOMEM : r_; \
    }                                                        \
  } while (0)
  ACHK(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
  ACHK(hipEventCreateWithFlags(&a->ev_last, hipEventDisableTiming));
  ACHK(hipEventCreateWithFlags(&a->ev_stage, hipEventDisableTiming));
  ACHK(hipEventCreate(&a->tm0));
  ACHK(hipEventCreate(&a->tm1));
  ACHK(hipMalloc((void**)&a->d_cols, C * 8));
  ACHK(hipMalloc((void**)&a->d_ema, S * C * 8));
  ACHK(hipMalloc((void**)&a->d_rows, S * R * C * 8));
  ACHK(hipMalloc((void**)&a->d_labels, S * R * 8));
  ACHK(hipMalloc((void**)&a->d_set, C * 8));
  ACHK(hipHostMalloc((void**)&a->h_set, C * 8, hipHostMallocDefault));
  ACHK(hipMemset(a->d_rows, 0, S * R * C * 8));
  ACHK(hipMemset(a->d_labels, 0, S * R * 8));
  ACHK(hipMemcpy(a->d_cols, cols, C * 8, hipMemcpyHostToDevice));
  a->body_off = (size_t)an_line_up(S * GMX_AN_HEAD);
  const size_t pack_bytes = a->body_off + S * (size_t)an_line_up(an_section_bytes(a, max_samples));
  ACHK(hipHostMalloc((void**)&a->h_pack, pack_bytes, hipHostMallocMapped | hipHostMallocCoherent));
  memset(a->h_pack, 0, pack_bytes);
  ACHK(hipHostGetDevicePointer((void**)&a->h_pack_dev, a->h_pack, 0));
  a->seen.assign(S, 0);
  a->rows.assign(S, 0);
  a->freq.assign(S, 0);
  for (auto* v : {&a->q_seen, &a->q_rows, &a->q_off, &a->t_seen, &a->t_rows, &a->t_off}) v->assign(S, 0);
  ACHK(gmx_launch_analysis_reset(a->d_ema, nullptr, 0, n_streams, (uint32_t)n_columns, a->stream));
  ACHK(hipStreamSynchronize(a->stream));
#undef ACHK
  *out = a;
  return GMX_OK;
}

extern "C" int gmx_analysis_reset(gmx_analysis* a, int s, const double* ema, uint64_t bits_seen) {
  if (!a || s < -1 || s >= a->S) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(a->device));
  const int s0 = s < 0 ? 0 : s, n = s < 0 ? a->S : 1;
  hipStream_t st = a->stream;
  if (ema) {
    int rc = an_stage_free(a);
    if (rc) return rc;
    memcpy(a->h_set, ema, (size_t)a->C * 8);
    HIPCHK(hipMemcpyAsync(a->d_set, a->h_set, (size_t)a->C * 8, hipMemcpyHostToDevice, st));
  }
  int rc = an_begin(a, st);
  if (rc) return rc;
  HIPCHK(gmx_launch_analysis_reset(a->d_ema, ema ? a->d_set : nullptr, s0, n, (uint32_t)a->C, st));
  if (ema) {
    rc = an_stage_used(a);
    if (rc) return rc;
  }
  rc = an_end(a, st);
  if (rc) return rc;
  for (int i = s0; i < s0 + n; ++i) {
    a->seen[i] = bits_seen;
    a->rows[i] = 0;
  }
  return GMX_OK;
}

extern "C" int gmx_analysis_set_frequency(gmx_analysis* a, int s, uint64_t frequency) {
  if (!a || s < -1 || s >= a->S) return GMX_ERR_INVALID;
  for (int i = (s < 0 ? 0 : s); i < (s < 0 ? a->S : s + 1); ++i) a->freq[i] = frequency;
  return GMX_OK;
}

extern "C" int gmx_analysis_update_batch(gmx_analysis* a, gmx_batch* b, const uint64_t* n_bits, float* kernel_ms) {
  if (!a || !b || !n_bits) return GMX_ERR_INVALID;
  gmx_group* g = b->g;
  if (!g || b->S != a->S || g->device != a->device) return GMX_ERR_INVALID;  // (a dead group's batch is a shell)
  for (const gmx_analysis_column& c : a->cols) {
    if (c.kind == GMX_AN_INPUT && c.index >= (uint32_t)g->topo.n) return GMX_ERR_INVALID;
    if (c.kind == GMX_AN_MIXER && (c.index >= (uint32_t)g->topo.m || !(b->flags & GMX_BATCH_OUTPUTS))) return GMX_ERR_INVALID;
  }
  if (!an_counts_fit(a, n_bits, b->max_bits)) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(a->device));
  hipStream_t st = g->stream;
  GmxAnArgs k;
  memset(&k, 0, sizeof k);
  k.pred = b->d_pred;
  k.mask = (b->flags & GMX_BATCH_MASK) ? b->d_mask : nullptr;
  k.out = (b->flags & GMX_BATCH_OUTPUTS) ? b->d_out : nullptr;
  k.p = b->d_p;
  k.bits = b->d_bits;
  k.pitch = b->max_bits;
  k.n_pad = (uint32_t)g->topo.n_pad;
  k.mask_words = (uint32_t)g->topo.mask_words;
  k.m = (uint32_t)g->topo.m;
  int rc = an_launch(a, &k, n_bits, st, kernel_ms);
  if (rc) return rc;
  // a use of the batch as a run is: the next upload, fill or run of it stands behind this kernel
  rc = batch_note_device_use(b);
  if (rc) return rc;
  rc = an_end(a, st);
  if (rc) return rc;
  if (kernel_ms) {
    HIPCHK(hipEventSynchronize(a->tm1));
    HIPCHK(hipEventElapsedTime(kernel_ms, a->tm0, a->tm1));
  }
  return GMX_OK;
}

extern "C" int gmx_analysis_update(gmx_analysis* a, const float* values, const uint8_t* bits, uint64_t pitch,
                                   const uint64_t* n_bits) {
  if (!a || !values || !bits || !n_bits) return GMX_ERR_INVALID;
  if (!an_counts_fit(a, n_bits, pitch)) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(a->device));
  const size_t S = (size_t)a->S, C = (size_t)a->C;
  size_t T = 0;
  for (size_t s = 0; s < S; ++s) T = std::max(T, (size_t)n_bits[s]);
  if (T == 0) return GMX_OK;
  int rc = an_stage_free(a);
  if (rc) return rc;
  if (T > a->stage_bits) {
    void* old[] = {a->d_val, a->d_bits};
    for (void* q : old)
      if (q) (void)hipFree(q);
    if (a->h_val) (void)hipHostFree(a->h_val);
    if (a->h_bits) (void)hipHostFree(a->h_bits);
    a->d_val = a->h_val = nullptr;
    a->d_bits = a->h_bits = nullptr;
    a->stage_bits = 0;
    BCHK(hipMalloc((void**)&a->d_val, S * T * C * 4));
    BCHK(hipMalloc((void**)&a->d_bits, S * T));
    BCHK(hipHostMalloc((void**)&a->h_val, S * T * C * 4, hipHostMallocDefault));
    BCHK(hipHostMalloc((void**)&a->h_bits, S * T, hipHostMallocDefault));
    a->stage_bits = T;
  }
  const size_t P = a->stage_bits;
  for (size_t s = 0; s < S; ++s) {
    memcpy(a->h_val + s * P * C, values + s * pitch * C, (size_t)n_bits[s] * C * 4);
    memcpy(a->h_bits + s * P, bits + s * pitch, (size_t)n_bits[s]);
  }
  hipStream_t st = a->stream;
  HIPCHK(hipMemcpyAsync(a->d_val, a->h_val, S * P * C * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(a->d_bits, a->h_bits, S * P, hipMemcpyHostToDevice, st));
  GmxAnArgs k;
  memset(&k, 0, sizeof k);
  k.values = a->d_val;
  k.bits = a->d_bits;
  k.pitch = P;
  rc = an_launch(a, &k, n_bits, st, nullptr);
  if (rc) return rc;
  rc = an_stage_used(a);
  if (rc) return rc;
  return an_end(a, st);
}

extern "C" int gmx_analysis_take_launch(gmx_analysis* a) {
  if (!a) return GMX_ERR_INVALID;
  if (a->take_queued) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(a->device));
  const size_t S = (size_t)a->S;
  std::vector<uint64_t> list(3 * S);
  uint64_t at = 0;
  for (size_t s = 0; s < S; ++s) {
    list[s] = a->q_seen[s] = a->seen[s];
    list[S + s] = a->q_rows[s] = a->rows[s];
    list[2 * S + s] = a->q_off[s] = at;
    at += an_line_up(an_section_bytes(a, a->rows[s]));
  }
  GmxAnPackArgs k;
  memset(&k, 0, sizeof k);
  k.ema = a->d_ema;
  k.rows = a->d_rows;
  k.labels = a->d_labels;
  k.packed = a->h_pack_dev;
  k.body_off = a->body_off;
  k.n_columns = (uint32_t)a->C;
  k.max_samples = (uint32_t)a->max_samples;
  k.n_streams = a->S;
  hipStream_t st = a->stream;
  int rc = an_begin(a, st);
  if (rc) return rc;
  rc = count_list_stage(a->lists, list.data(), (int)list.size(), st, &k.list);
  if (rc) return rc;
  HIPCHK(gmx_launch_analysis_pack(&k, st));
  rc = count_list_used(a->lists, st);
  if (rc) return rc;
  rc = an_end(a, st);
  if (rc) return rc;
  std::fill(a->rows.begin(), a->rows.end(), 0);
  a->take_queued = true;
  a->taken = false;
  return GMX_OK;
}

extern "C" int gmx_analysis_take_wait(gmx_analysis* a) {
  if (!a) return GMX_ERR_INVALID;
  if (!a->take_queued) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(a->device));
  if (a->last_rec) HIPCHK(hipEventSynchronize(a->ev_last));
  a->take_queued = false;
  uint64_t wrote = (uint64_t)a->S * GMX_AN_HEAD;
  for (int s = 0; s < a->S; ++s) {
    const uint64_t* line = (const uint64_t*)(a->h_pack + (size_t)s * GMX_AN_HEAD);
    a->t_seen[s] = line[0];
    a->t_rows[s] = line[1];
    a->t_off[s] = a->q_off[s];
    wrote += an_section_bytes(a, line[1]);
  }
  a->d2h = (int64_t)wrote;
  a->taken = true;
  return GMX_OK;
}

extern "C" int gmx_analysis_take(gmx_analysis* a) {
  const int rc = gmx_analysis_take_launch(a);
  return rc ? rc : gmx_analysis_take_wait(a);
}

extern "C" const double* gmx_analysis_ema(gmx_analysis* a, int s) {
  if (!a || s < 0 || s >= a->S || !a->taken) return nullptr;
  return (const double*)(a->h_pack + a->body_off + a->t_off[s]);
}
extern "C" uint64_t gmx_analysis_bits_seen(gmx_analysis* a, int s) {
  return (!a || s < 0 || s >= a->S || !a->taken) ? 0 : a->t_seen[s];
}
extern "C" uint64_t gmx_analysis_n_samples(gmx_analysis* a, int s) {
  return (!a || s < 0 || s >= a->S || !a->taken) ? 0 : a->t_rows[s];
}
extern "C" const double* gmx_analysis_samples(gmx_analysis* a, int s) {
  if (!a || s < 0 || s >= a->S || !a->taken) return nullptr;
  return (const double*)(a->h_pack + a->body_off + a->t_off[s]) + a->C;
}
extern "C" const uint64_t* gmx_analysis_sample_bits(gmx_analysis* a, int s) {
  if (!a || s < 0 || s >= a->S || !a->taken) return nullptr;
  return (const uint64_t*)((const double*)(a->h_pack + a->body_off + a->t_off[s]) + a->C + (size_t)a->C * a->t_rows[s]);
}
extern "C" int64_t gmx_debug_analysis_d2h_bytes(gmx_analysis* a) { return a ? a->d2h : (int64_t)GMX_ERR_INVALID; }
