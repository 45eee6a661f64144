// gmx_encoder.inc -- the arithmetic encoder on the device: compressed bytes out of a batch (included by gmx_capi.cpp;
// include/gmxmix_encoder.h, DESIGN.md section 4.22).
//
// A gmx_encoder holds Encoder's two words for S streams, an output area of 4 * max_bits + 5 bytes per stream (a bit
// emits at most 4 bytes and a flush at most 5: a round can never overflow it) and a pinned buffer the take's kernels
// pack the round into.  It codes a gmx_batch's device `bits` and `p` on the batch's group's stream, right behind the
// kernel that wrote p, or host arrays on a stream of its own; one event orders its work across the two.

struct gmx_encoder {
  int device = 0, S = 0;
  uint64_t max_bits = 0;
  uint32_t area_words = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_last = nullptr;   // behind the newest work on the encoder's device state, whatever stream it ran on
  hipEvent_t ev_stage = nullptr;  // behind the newest kernel that read the staging arrays below
  hipEvent_t tm0 = nullptr, tm1 = nullptr;
  bool last_rec = false, last_own = false, stage_rec = false;
  GmxEncStream* d_streams = nullptr;
  uint64_t* d_coded = nullptr;
  uint32_t* d_out = nullptr;
  uint64_t* d_off = nullptr;
  GmxCountList counts;
  // gmx_encoder_encode's copies of the caller's arrays, gmx_encoder_flush's `which` (lazily)
  float *d_p = nullptr, *h_p = nullptr;
  uint8_t *d_bits = nullptr, *h_bits = nullptr, *d_which = nullptr, *h_which = nullptr;
  // the take
  uint8_t *h_pack = nullptr, *h_pack_dev = nullptr;
  size_t body_off = 0;
  bool take_queued = false, taken = false;
  int64_t d2h = 0;
  std::vector<uint64_t> worst;    // the most bytes the round can hold by now: 4 per bit given, 5 per flush
  std::vector<uint64_t> off, n_bytes, total;
  std::vector<int64_t> bad;
};

static uint64_t enc_line_up(uint64_t n) { return (n + (GMX_ENC_LINE - 1)) & ~(uint64_t)(GMX_ENC_LINE - 1); }
static uint64_t enc_area_bytes(const gmx_encoder* e) { return 4ull * e->max_bits + 5ull; }

// Work on the encoder's device state is about to be queued on `st` / has been.
static int enc_begin(gmx_encoder* e, hipStream_t st) {
  if (e->last_rec && !(e->last_own && st == e->stream)) HIPCHK(hipStreamWaitEvent(st, e->ev_last, 0));
  return GMX_OK;
}
static int enc_end(gmx_encoder* e, hipStream_t st) {
  HIPCHK(hipEventRecord(e->ev_last, st));
  e->last_rec = true;
  e->last_own = st == e->stream;
  e->taken = false;
  return GMX_OK;
}
static int enc_sync(gmx_encoder* e) {
  if (e->last_rec) HIPCHK(hipEventSynchronize(e->ev_last));
  return GMX_OK;
}
static void enc_args(const gmx_encoder* e, GmxEncArgs* a) {
  memset(a, 0, sizeof *a);
  a->streams = e->d_streams;
  a->n_coded = e->d_coded;
  a->out = e->d_out;
  a->area_words = e->area_words;
  a->n_streams = e->S;
}
// The counts of a call: within `limit`, and the round stays within the area.  Nothing is written.
static bool enc_counts_fit(const gmx_encoder* e, const uint64_t* n_bits, uint64_t limit) {
  for (int s = 0; s < e->S; ++s) {
    if (n_bits[s] > limit || n_bits[s] > e->max_bits) return false;
    if (e->worst[s] + 4ull * n_bits[s] > 4ull * e->max_bits) return false;  // (the 5 are a flush's)
  }
  return true;
}

extern "C" void gmx_encoder_destroy(gmx_encoder* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->last_rec) (void)hipEventSynchronize(e->ev_last);
  if (e->stage_rec) (void)hipEventSynchronize(e->ev_stage);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  count_list_free(e->counts);
  void* dv[] = {e->d_streams, e->d_coded, e->d_out, e->d_off, e->d_p, e->d_bits, e->d_which};
  for (void* q : dv)
    if (q) (void)hipFree(q);
  void* hv[] = {e->h_p, e->h_bits, e->h_which, e->h_pack};
  for (void* q : hv)
    if (q) (void)hipHostFree(q);
  hipEvent_t evs[] = {e->ev_last, e->ev_stage, e->tm0, e->tm1};
  for (hipEvent_t ev : evs)
    if (ev) (void)hipEventDestroy(ev);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  (void)hipGetLastError();
  delete e;
}

extern "C" int gmx_encoder_create(gmx_encoder** out, int n_streams, uint64_t max_bits, int device) {
  if (!out) return GMX_ERR_INVALID;
  *out = nullptr;
  if (n_streams < 1 || max_bits < 1 || max_bits > (1ull << 28) || device < 0) return GMX_ERR_INVALID;
  int n_dev = 0;
  HIPCHK(hipGetDeviceCount(&n_dev));
  if (device >= n_dev) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(device));
  gmx_encoder* e = new (std::nothrow) gmx_encoder();
  if (!e) return GMX_ERR_NOMEM;
  e->device = device;
  e->S = n_streams;
  e->max_bits = max_bits;
  e->area_words = (uint32_t)((enc_area_bytes(e) + 3) / 4 + 1);
  const size_t S = (size_t)n_streams;
#define ECHK(call)                                           \
  do {                                                       \
    hipError_t e_ = (call);                                  \
    if (e_ != hipSuccess) {                                  \
      int r_ = hip_fail(e_, #call);                          \
      gmx_encoder_destroy(e);                                \
      return e_ == hipErrorOutOfMemory ? GMX_ERR_NOMEM : r_; \
    }                                                        \
  } while (0)
  ECHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  ECHK(hipEventCreateWithFlags(&e->ev_last, hipEventDisableTiming));
  ECHK(hipEventCreateWithFlags(&e->ev_stage, hipEventDisableTiming));
  ECHK(hipEventCreate(&e->tm0));
  ECHK(hipEventCreate(&e->tm1));
  ECHK(hipMalloc((void**)&e->d_streams, S * sizeof(GmxEncStream)));
  ECHK(hipMalloc((void**)&e->d_coded, S * sizeof(uint64_t)));
  ECHK(hipMalloc((void**)&e->d_off, S * sizeof(uint64_t)));
  ECHK(hipMalloc((void**)&e->d_out, S * (size_t)e->area_words * 4));
  ECHK(hipMemset(e->d_streams, 0, S * sizeof(GmxEncStream)));
  ECHK(hipMemset(e->d_off, 0, S * sizeof(uint64_t)));
  ECHK(hipMemset(e->d_out, 0, S * (size_t)e->area_words * 4));
  e->body_off = (size_t)enc_line_up(S * sizeof(GmxEncStream));
  const size_t pack_bytes = e->body_off + S * (size_t)enc_line_up((uint64_t)e->area_words * 4);
  ECHK(hipHostMalloc((void**)&e->h_pack, pack_bytes, hipHostMallocMapped | hipHostMallocCoherent));
  memset(e->h_pack, 0, pack_bytes);
  ECHK(hipHostGetDevicePointer((void**)&e->h_pack_dev, e->h_pack, 0));
  e->worst.assign(S, 0);
  e->off.assign(S, 0);
  e->n_bytes.assign(S, 0);
  e->total.assign(S, 0);
  e->bad.assign(S, -1);
  ECHK(gmx_launch_encoder_reset(e->d_streams, e->d_coded, 0, n_streams, 0u, 0xffffffffu, e->stream));
  ECHK(hipStreamSynchronize(e->stream));
#undef ECHK
  *out = e;
  return GMX_OK;
}

extern "C" int gmx_encoder_reset(gmx_encoder* e, int s, const uint32_t* state) {
  if (!e || s < -1 || s >= e->S) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  const int s0 = s < 0 ? 0 : s, n = s < 0 ? e->S : 1;
  int rc = enc_begin(e, e->stream);
  if (rc) return rc;
  HIPCHK(gmx_launch_encoder_reset(e->d_streams, e->d_coded, s0, n, state ? state[0] : 0u, state ? state[1] : 0xffffffffu,
                                  e->stream));
  rc = enc_end(e, e->stream);
  if (rc) return rc;
  for (int i = s0; i < s0 + n; ++i) {
    e->worst[i] = 0;
    e->total[i] = 0;
    e->n_bytes[i] = 0;
    e->bad[i] = -1;
  }
  return GMX_OK;
}

extern "C" int gmx_encoder_state(gmx_encoder* e, int s, uint32_t out[2]) {
  if (!e || s < 0 || s >= e->S || !out) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  int rc = enc_sync(e);
  if (rc) return rc;
  GmxEncStream rec;
  HIPCHK(hipMemcpy(&rec, e->d_streams + s, sizeof rec, hipMemcpyDeviceToHost));
  out[0] = rec.x1;
  out[1] = rec.x2;
  e->total[s] = rec.total;
  e->bad[s] = rec.bad_bit;
  return GMX_OK;
}

extern "C" int gmx_encoder_encode_batch(gmx_encoder* e, gmx_batch* b, const uint64_t* n_bits, float* kernel_ms) {
  if (!e || !b || !n_bits) return GMX_ERR_INVALID;
  gmx_group* g = b->g;
  if (!g || b->S != e->S || g->device != e->device) return GMX_ERR_INVALID;  // (a dead group's batch is a shell)
  if (!enc_counts_fit(e, n_bits, b->max_bits)) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = g->stream;
  GmxEncArgs a;
  enc_args(e, &a);
  a.p = b->d_p;
  a.bits = b->d_bits;
  a.pitch = b->max_bits;
  int rc = enc_begin(e, st);
  if (rc) return rc;
  rc = count_list_stage(e->counts, n_bits, e->S, st, &a.n_bits);
  if (rc) return rc;
  if (kernel_ms) HIPCHK(hipEventRecord(e->tm0, st));
  HIPCHK(gmx_launch_encoder(&a, st));
  if (kernel_ms) HIPCHK(hipEventRecord(e->tm1, st));
  rc = count_list_used(e->counts, st);
  if (rc) return rc;
  for (int s = 0; s < e->S; ++s) e->worst[s] += 4ull * n_bits[s];
  // a use of the batch as a run is: the next upload, fill or run of it stands behind this kernel
  rc = batch_note_device_use(b);
  if (rc) return rc;
  rc = enc_end(e, st);
  if (rc) return rc;
  if (kernel_ms) {
    HIPCHK(hipEventSynchronize(e->tm1));
    HIPCHK(hipEventElapsedTime(kernel_ms, e->tm0, e->tm1));
  }
  return GMX_OK;
}

// The staging arrays may be written: the kernel that read them last is done.
static int enc_stage_free(gmx_encoder* e) {
  if (e->stage_rec) HIPCHK(hipEventSynchronize(e->ev_stage));
  e->stage_rec = false;
  return GMX_OK;
}
static int enc_stage_used(gmx_encoder* e) {
  HIPCHK(hipEventRecord(e->ev_stage, e->stream));
  e->stage_rec = true;
  return GMX_OK;
}

extern "C" int gmx_encoder_encode(gmx_encoder* e, const float* p, const uint8_t* bits, uint64_t pitch,
                                  const uint64_t* n_bits) {
  if (!e || !p || !bits || !n_bits) return GMX_ERR_INVALID;
  if (!enc_counts_fit(e, n_bits, pitch)) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  const size_t S = (size_t)e->S, T = (size_t)e->max_bits;
  if (!e->d_p) {
    BCHK(hipMalloc((void**)&e->d_p, S * T * 4));
    BCHK(hipMalloc((void**)&e->d_bits, S * T));
    BCHK(hipHostMalloc((void**)&e->h_p, S * T * 4, hipHostMallocDefault));
    BCHK(hipHostMalloc((void**)&e->h_bits, S * T, hipHostMallocDefault));
  }
  int rc = enc_stage_free(e);
  if (rc) return rc;
  for (size_t s = 0; s < S; ++s) {
    memcpy(e->h_p + s * T, p + s * pitch, (size_t)n_bits[s] * 4);
    memcpy(e->h_bits + s * T, bits + s * pitch, (size_t)n_bits[s]);
  }
  hipStream_t st = e->stream;
  HIPCHK(hipMemcpyAsync(e->d_p, e->h_p, S * T * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(e->d_bits, e->h_bits, S * T, hipMemcpyHostToDevice, st));
  GmxEncArgs a;
  enc_args(e, &a);
  a.p = e->d_p;
  a.bits = e->d_bits;
  a.pitch = e->max_bits;
  rc = enc_begin(e, st);
  if (rc) return rc;
  rc = count_list_stage(e->counts, n_bits, e->S, st, &a.n_bits);
  if (rc) return rc;
  HIPCHK(gmx_launch_encoder(&a, st));
  rc = count_list_used(e->counts, st);
  if (rc) return rc;
  for (int s = 0; s < e->S; ++s) e->worst[s] += 4ull * n_bits[s];
  rc = enc_stage_used(e);
  if (rc) return rc;
  return enc_end(e, st);
}

extern "C" int gmx_encoder_flush(gmx_encoder* e, const uint8_t* which) {
  if (!e) return GMX_ERR_INVALID;
  for (int s = 0; s < e->S; ++s)
    if ((!which || which[s]) && e->worst[s] + 5ull > enc_area_bytes(e)) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = e->stream;
  if (which) {
    if (!e->d_which) {
      BCHK(hipMalloc((void**)&e->d_which, (size_t)e->S));
      BCHK(hipHostMalloc((void**)&e->h_which, (size_t)e->S, hipHostMallocDefault));
    }
    int rc = enc_stage_free(e);
    if (rc) return rc;
    memcpy(e->h_which, which, (size_t)e->S);
    HIPCHK(hipMemcpyAsync(e->d_which, e->h_which, (size_t)e->S, hipMemcpyHostToDevice, st));
  }
  GmxEncArgs a;
  enc_args(e, &a);
  int rc = enc_begin(e, st);
  if (rc) return rc;
  HIPCHK(gmx_launch_encoder_flush(&a, which ? e->d_which : nullptr, st));
  for (int s = 0; s < e->S; ++s)
    if (!which || which[s]) e->worst[s] += 5ull;
  if (which) {
    rc = enc_stage_used(e);
    if (rc) return rc;
  }
  return enc_end(e, st);
}

extern "C" int gmx_encoder_take_launch(gmx_encoder* e) {
  if (!e) return GMX_ERR_INVALID;
  if (e->take_queued) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(e->device));
  GmxEncPackArgs a;
  memset(&a, 0, sizeof a);
  a.streams = e->d_streams;
  a.out = e->d_out;
  a.offsets = e->d_off;
  a.packed = e->h_pack_dev;
  a.body_off = e->body_off;
  a.area_words = e->area_words;
  a.n_streams = e->S;
  int rc = enc_begin(e, e->stream);
  if (rc) return rc;
  HIPCHK(gmx_launch_encoder_pack(&a, e->stream));
  rc = enc_end(e, e->stream);
  if (rc) return rc;
  std::fill(e->worst.begin(), e->worst.end(), 0);
  e->take_queued = true;
  return GMX_OK;
}

extern "C" int gmx_encoder_take_wait(gmx_encoder* e) {
  if (!e) return GMX_ERR_INVALID;
  if (!e->take_queued) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(e->device));
  int rc = enc_sync(e);
  if (rc) return rc;
  e->take_queued = false;
  const GmxEncStream* line = (const GmxEncStream*)e->h_pack;
  uint64_t at = 0, wrote = (uint64_t)e->S * sizeof(GmxEncStream);
  bool any_bad = false;
  for (int s = 0; s < e->S; ++s) {
    e->off[s] = at;
    e->n_bytes[s] = line[s].n_round;
    e->total[s] = line[s].total;
    e->bad[s] = line[s].bad_bit;
    at += enc_line_up(line[s].n_round);
    wrote += ((uint64_t)line[s].n_round + 3u) / 4u * 4u;
    any_bad = any_bad || line[s].bad_bit >= 0;
  }
  e->d2h = (int64_t)wrote;
  e->taken = true;
  return any_bad ? GMX_ERR_INVALID : GMX_OK;  // (the other streams' bytes are valid and delivered)
}

extern "C" int gmx_encoder_take(gmx_encoder* e) {
  const int rc = gmx_encoder_take_launch(e);
  return rc ? rc : gmx_encoder_take_wait(e);
}

extern "C" const uint8_t* gmx_encoder_bytes(gmx_encoder* e, int s) {
  if (!e || s < 0 || s >= e->S || !e->taken) return nullptr;
  return e->h_pack + e->body_off + e->off[s];
}
extern "C" uint64_t gmx_encoder_n_bytes(gmx_encoder* e, int s) {
  return (!e || s < 0 || s >= e->S || !e->taken) ? 0 : e->n_bytes[s];
}
extern "C" uint64_t gmx_encoder_total_bytes(gmx_encoder* e, int s) {
  return (!e || s < 0 || s >= e->S) ? 0 : e->total[s];
}
extern "C" int64_t gmx_encoder_bad_bit(gmx_encoder* e, int s) {
  return (!e || s < 0 || s >= e->S) ? (int64_t)GMX_ERR_INVALID : e->bad[s];
}
extern "C" int64_t gmx_debug_encoder_d2h_bytes(gmx_encoder* e) { return e ? e->d2h : (int64_t)GMX_ERR_INVALID; }
