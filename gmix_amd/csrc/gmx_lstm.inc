// gmx_lstm.inc -- host side of the LSTM byte-model banks (included by gmx_capi.cpp).
//
// Replaces the reference's LstmModel (models/lstm-model.{h,cpp}: Lstm(256, 256, 50, 1, 100, 0.03,
// 10)) together with its share of LongTermMemory (neuron_layer_weights, lstm_output_layer,
// long-term-memory.h:55-76) for S independent streams.  Compute is gmx_lstm.hip; no CPU fallback.

struct gmx_lstm_batch : GmxBatchCore {
  gmx_lstm* l = nullptr;
  uint64_t& max_bytes = max_rows;  // (its records are bytes)
  float* d_ppm = nullptr;
  uint8_t* d_bytes = nullptr;
  float* d_pred = nullptr;
  uint8_t* d_act = nullptr;
  uint32_t* d_ctx = nullptr;
  float* h_ppm = nullptr;
  uint8_t* h_bytes = nullptr;
  float* h_pred = nullptr;
  uint8_t* h_act = nullptr;
  uint32_t* h_ctx = nullptr;
};

struct gmx_lstm {
  int device = 0, S = 0;
  GmxLstmDev dev;
  GmxLstmDev* dev_d = nullptr;
  float* banks = nullptr;
  hipStream_t stream = nullptr;
  int cus = 0;                          // compute units its kernels may use (the device's, or the CU mask's)
  hipStream_t up_stream = nullptr, down_stream = nullptr;   // record batches beside the kernels
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // kernel timing

  std::vector<uint64_t> bytes_seen;     // host mirror: Lstm::Predict calls so far (decides when backward passes fall)
  std::vector<uint32_t> update_steps;   // host mirror of LstmLayer::update_steps_
  // Adam's scalars of a launch: four staging slots in turn, a slot reused when the launch that read it is done (a
  // launch must not wait for the one before it: queued back to back, the kernels of neighbouring chunks follow each
  // other without the host in between)
  static constexpr int kAdamSlots = 4;
  float* adam_dev[kAdamSlots] = {};
  float* adam_host[kAdamSlots] = {};
  hipEvent_t adam_done[kAdamSlots] = {};
  bool adam_busy[kAdamSlots] = {};
  size_t adam_cap = 0;
  unsigned adam_seq = 0;
  GmxCountList counts;                  // per-stream byte counts of ragged launches
  GmxBatchBank bb;                      // its record batches
  gmx_lstm_batch* one = nullptr;        // record arrays of the per-byte surface
  std::vector<uint8_t> fwd_done;
  // The range state LstmModel keeps beside the network (top_/mid_/bot_, lstm-model.h) is the caller's inside a byte.
  // What a checkpoint file said about it is kept until the bank moves on, so that a bank written out right after an
  // import gives back the file it was given, wherever in the byte that file was taken.
  struct Range {
    bool valid = false;
    int32_t tmb[3] = {255, 127, 0};
  };
  std::vector<Range> range_read;
  std::vector<struct GmxLstmSession*> sessions;  // per-byte sessions (gmx_lstm_kernel<.., true>), per stream
  bool use_sessions = true;
  bool banks_in_use_by_dead_kernel = false;  // a session block that stopped answering may still hold them: never freed
  struct GmxLstmCkptState* ckpt = nullptr;  // gmx_lstm_group_export / _import: layout tables and staging (gmx_lstm_ckpt.inc), lazily
  // The shape (gmx_lstm_create_shaped).  any == false: the stock shape on the GMX_L_* layout, run by gmx_lstm.hip.
  // any == true: any other shape -- or the stock one created under GMX_LSTM_BUILD=any -- on the layout of
  // gmx_lstm_any.h, run by gmx_lstm_any.hip; `dev` then holds adev.o, so that what only needs offsets reads one place
  gmx_lstm_shape shape = kLstmStockShape;
  bool any = false;
  GmxLstmAnyDev adev;
  GmxLstmAnyDev* adev_d = nullptr;
  int64_t any_launches = 0;
};
static LstmDims lstm_dims(const gmx_lstm* l) { return lstm_dims_of(l->shape, l->any); }
static void lstm_ckpt_free(gmx_lstm* l);

// ---- per-byte sessions: gmx_lstm_forward / gmx_lstm_perceive without a kernel launch per call -----------
// The protocol and its bounded waits are gmx_mailbox.h, the blocks and the stream of a session GmxSessionHw
// (gmx_session.inc), as for the mixers and the Indirect models: the Perceive is only noted and travels with the next
// forward as one command; every other entry point that touches the bank first stops the session, which writes the
// model's state back.  Nothing is ever replayed: Predict and Perceive are separate steps of the bank as they are of
// the launch-per-call path, so a block that left on its idle timer in between simply comes back.  One payload, so
// the slot bit of its command words is always 0.
struct GmxLstmSession : GmxSessionHw {
  GmxLstmMbCmd* mc = nullptr;
  GmxLstmMbReply* mb = nullptr;
  int pending_byte = -1;       // noted by gmx_lstm_perceive, not yet published
  float pending_adam[4] = {0, 0, 0, 0};
};
static int lstm_sessions_close(gmx_lstm* l);
static void lstm_sessions_free(gmx_lstm* l);
#define LSTM_CLOSE_SESSIONS(l)            \
  do {                                    \
    int rcs_ = lstm_sessions_close(l);    \
    if (rcs_) return rcs_;                \
  } while (0)
extern "C" hipError_t gmx_launch_lstm_session(const GmxLstmDev* dv, const GmxLstmRunArgs* args, hipStream_t stream);

extern "C" hipError_t gmx_launch_lstm_kernel(const GmxLstmDev* dv, const GmxLstmRunArgs* args, int n_streams, int cus,
                                             hipStream_t stream);

// The bank layout of a shape: the stock one's offsets are what they always were (its kernels read the compile-time
// GMX_L_* extents); any other comes from lstm_layout_any (gmx_lstm_any.inc)
static void lstm_layout_stock(GmxLstmDev* d);
static void lstm_layout(gmx_lstm* l) {
  if (l->any) {
    lstm_layout_any(&l->adev, l->shape);
    l->dev = l->adev.o;
  } else {
    lstm_layout_stock(&l->dev);
  }
}
static void lstm_layout_stock(GmxLstmDev* d) {
  uint64_t off = 0;
  auto take = [&off](uint64_t n) {
    uint64_t o = off;
    off += (n + 63) / 64 * 64;
    return o;
  };
  const uint64_t H = GMX_L_H, CP = GMX_L_CP;
  d->out_layer = take(H * GMX_L_HID * GMX_L_NO);
  for (int g = 0; g < 3; ++g) {
    GmxLstmGateOff& o = d->gate[g];
    o.weights = take(GMX_L_MAT_FLOATS);
    o.update = take(GMX_L_MAT_FLOATS);
    o.m = take(GMX_L_MAT_FLOATS);
    o.v = take(GMX_L_MAT_FLOATS);
    uint64_t* vecs[] = {&o.gamma, &o.gamma_u, &o.gamma_m, &o.gamma_v, &o.beta, &o.beta_u, &o.beta_m, &o.beta_v, &o.error};
    for (uint64_t* p : vecs) *p = take(CP);
    o.state = take(H * CP);
    o.norm = take(H * CP);
    o.ivar = take(H);
    o.transpose = take((uint64_t)GMX_L_HID * CP);
  }
  d->state = take(CP);
  d->state_error = take(CP);
  d->stored_error = take(CP);
  d->tanh_state = take(H * CP);
  d->input_gate_state = take(H * CP);
  d->last_state = take(H * CP);
  d->hidden = take(CP);
  d->hidden_error = take(CP);
  d->layer_input = take(H * GMX_L_LINP);
  d->lin_t = take((uint64_t)GMX_L_LIN * GMX_L_HP);
  d->errs = take(3 * H * CP);
  d->output = take(H * GMX_L_NO);
  d->input_history = take(H);
  d->probs = take(GMX_L_NO);
  d->scal = take(16);
  d->bank_floats = off;
}

static void lstm_batch_free(gmx_lstm_batch* b) {
  if (!b) return;
  batch_core_free(*b);
  delete b;
}

extern "C" void gmx_lstm_destroy(gmx_lstm* l) {
  if (!l) return;
  (void)hipSetDevice(l->device);
  lstm_sessions_free(l);
  if (l->stream) (void)hipStreamSynchronize(l->stream);
  lstm_ckpt_free(l);
  if (l->one) {
    lstm_batch_free(l->one);
    l->one = nullptr;
  }
  batch_bank_detach_all(l->bb);  // shells, as for gmx_batch
  if (!l->banks_in_use_by_dead_kernel) {  // (as gmx_group_destroy: leaked rather than freed under a running kernel)
    if (l->banks) (void)hipFree(l->banks);
    if (l->dev_d) (void)hipFree(l->dev_d);
    if (l->adev_d) (void)hipFree(l->adev_d);
  }
  for (int k = 0; k < gmx_lstm::kAdamSlots; ++k) {
    if (l->adam_host[k]) (void)hipHostFree(l->adam_host[k]);
    if (l->adam_done[k]) (void)hipEventDestroy(l->adam_done[k]);
  }
  if (l->ev0) (void)hipEventDestroy(l->ev0);
  if (l->ev1) (void)hipEventDestroy(l->ev1);

  hipStream_t xs[] = {l->up_stream, l->down_stream};
  for (hipStream_t x : xs)
    if (x) {
      (void)hipStreamSynchronize(x);
      (void)hipStreamDestroy(x);
    }
  count_list_free(l->counts);
  if (l->stream) (void)hipStreamDestroy(l->stream);
  delete l;
}

// The constructed state (lstm.cpp:9-43, lstm-layer.cpp:36-56, :155-178, lstm-model.cpp:7-11) with
// all-zero gate weights: the random initialisation (lstm-layer.cpp:179-194 draws from rand()) is
// the caller's to supply through gmx_lstm_set_weights.
extern "C" int gmx_lstm_reset(gmx_lstm* l) {
  if (!l) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  std::vector<float> img(l->dev.bank_floats, 0.0f);
  const GmxLstmDev& d = l->dev;
  const LstmDims k = lstm_dims(l);
  for (int g = 0; g < 3; ++g)
    for (int i = 0; i < k.NC; ++i) img[d.gate[g].gamma + i] = 1.0f;
  img[d.hidden + k.HID - 1] = 1.0f;
  for (int e = 0; e < k.H; ++e) {
    img[d.layer_input + (uint64_t)e * k.LINP + k.LIN - 1] = 1.0f;
    for (int i = 0; i < GMX_L_NO; ++i) img[d.output + (uint64_t)e * GMX_L_NO + i] = (float)(1.0 / GMX_L_NO);
  }
  for (int i = 0; i < GMX_L_NO; ++i) img[d.probs + i] = (float)(1.0 / 256);
  HIPCHK(hipStreamSynchronize(l->stream));
  for (int s = 0; s < l->S; ++s)
    HIPCHK(hipMemcpy(l->banks + (size_t)s * d.bank_floats, img.data(), img.size() * 4, hipMemcpyHostToDevice));
  std::fill(l->bytes_seen.begin(), l->bytes_seen.end(), 0);
  std::fill(l->update_steps.begin(), l->update_steps.end(), 0);
  std::fill(l->fwd_done.begin(), l->fwd_done.end(), 0);
  for (auto& r : l->range_read) r.valid = false;
  return GMX_OK;
}

static int lstm_create(gmx_lstm** out, const gmx_lstm_shape& shape, int n_streams, int device) {
  if (!out) return GMX_ERR_INVALID;
  *out = nullptr;
  if (n_streams < 1 || !gmx_lstm_shape_supported(&shape)) return GMX_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return GMX_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(device));
  gmx_lstm* l = new (std::nothrow) gmx_lstm();
  if (!l) return GMX_ERR_NOMEM;
  l->device = device;
  batch_bank_init(l->bb, l, device, &l->stream, &l->up_stream, &l->down_stream);
  l->S = n_streams;
  l->shape = shape;
  l->any = !lstm_shape_is_stock(shape) || lstm_env_forces_any();
  l->use_sessions = !l->any;  // (the per-byte session is a build of the stock kernel)
  lstm_layout(l);
  l->bytes_seen.assign(n_streams, 0);
  l->update_steps.assign(n_streams, 0);
  l->fwd_done.assign(n_streams, 0);
  l->range_read.assign(n_streams, gmx_lstm::Range());
#define LCHK(call)                                 \
  do {                                             \
    hipError_t e_ = (call);                        \
    if (e_ != hipSuccess) {                        \
      int r_ = hip_fail(e_, #call);                \
      gmx_lstm_destroy(l);                         \
      return e_ == hipErrorOutOfMemory ? GMX_ERR_NOMEM : r_; \
    }                                              \
  } while (0)
  LCHK(bank_stream_create(&l->stream, 2));
  {
    int n = 0;
    LCHK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device));
    l->cus = n;
  }
  LCHK(hipEventCreate(&l->ev0));
  LCHK(hipEventCreate(&l->ev1));
  LCHK(hipMalloc((void**)&l->dev_d, sizeof(GmxLstmDev)));
  LCHK(hipMemcpy(l->dev_d, &l->dev, sizeof(GmxLstmDev), hipMemcpyHostToDevice));
  if (l->any) {
    LCHK(hipMalloc((void**)&l->adev_d, sizeof(GmxLstmAnyDev)));
    LCHK(hipMemcpy(l->adev_d, &l->adev, sizeof(GmxLstmAnyDev), hipMemcpyHostToDevice));
  }
  LCHK(hipMalloc((void**)&l->banks, (size_t)n_streams * l->dev.bank_floats * sizeof(float)));
#undef LCHK
  int rc = gmx_lstm_reset(l);
  if (rc) {
    gmx_lstm_destroy(l);
    return rc;
  }
  *out = l;
  return GMX_OK;
}

extern "C" int gmx_lstm_create(gmx_lstm** out, int n_streams, int device) {
  return lstm_create(out, kLstmStockShape, n_streams, device);
}
extern "C" int gmx_lstm_create_shaped(gmx_lstm** out, const gmx_lstm_shape* shape, int n_streams, int device) {
  if (out) *out = nullptr;
  if (!shape) return GMX_ERR_INVALID;
  return lstm_create(out, *shape, n_streams, device);
}
extern "C" int gmx_lstm_get_shape(const gmx_lstm* l, gmx_lstm_shape* out) {
  if (!l || !out) return GMX_ERR_INVALID;
  *out = l->shape;
  return GMX_OK;
}
extern "C" int64_t gmx_debug_lstm_any_launches(const gmx_lstm* l) { return l ? l->any_launches : -1; }

extern "C" int gmx_lstm_n_streams(const gmx_lstm* l) { return l ? l->S : GMX_ERR_INVALID; }
extern "C" uint64_t gmx_lstm_bank_bytes(const gmx_lstm* l) { return l ? l->dev.bank_floats * 4 : 0; }
extern "C" int gmx_lstm_sync(gmx_lstm* l) {
  if (!l) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  HIPCHK(hipStreamSynchronize(l->stream));
  return GMX_OK;
}

// Gate weights in the reference's layout: LongTermMemory::neuron_layer_weights[gate][cell][563]
// (gate 0 forget, 1 input node, 2 output).
extern "C" int gmx_lstm_set_weights(gmx_lstm* l, int stream, const float* w) {
  if (!l || stream < 0 || stream >= l->S || !w) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  HIPCHK(hipStreamSynchronize(l->stream));
  const LstmDims k = lstm_dims(l);
  std::vector<float> t((size_t)k.mat_floats, 0.0f);
  for (int g = 0; g < 3; ++g) {
    std::fill(t.begin(), t.end(), 0.0f);
    for (int i = 0; i < k.NC; ++i)
      for (int j = 0; j < k.W; ++j) t[k.mat(j, i)] = w[((size_t)g * k.NC + i) * k.W + j];
    HIPCHK(hipMemcpy(l->banks + (size_t)stream * l->dev.bank_floats + l->dev.gate[g].weights, t.data(), t.size() * 4,
                     hipMemcpyHostToDevice));
  }
  return GMX_OK;
}

// The learned parameters back in the reference's layouts (what LongTermMemory::WriteToDisk stores,
// long-term-memory.cpp:57-68): weights [3][50][563]; output_layer [100][256][51] (nullable).
extern "C" int gmx_lstm_get_weights(gmx_lstm* l, int stream, float* w, float* output_layer) {
  if (!l || stream < 0 || stream >= l->S || !w) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  HIPCHK(hipStreamSynchronize(l->stream));
  const LstmDims k = lstm_dims(l);
  std::vector<float> t((size_t)k.mat_floats);
  const float* bank = l->banks + (size_t)stream * l->dev.bank_floats;
  for (int g = 0; g < 3; ++g) {
    HIPCHK(hipMemcpy(t.data(), bank + l->dev.gate[g].weights, t.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < k.NC; ++i)
      for (int j = 0; j < k.W; ++j) w[((size_t)g * k.NC + i) * k.W + j] = t[k.mat(j, i)];
  }
  if (output_layer) {
    std::vector<float> o((size_t)k.H * k.HID * GMX_L_NO);
    HIPCHK(hipMemcpy(o.data(), bank + l->dev.out_layer, o.size() * 4, hipMemcpyDeviceToHost));
    for (int e = 0; e < k.H; ++e)
      for (int i = 0; i < GMX_L_NO; ++i)
        for (int j = 0; j < k.HID; ++j)
          output_layer[((size_t)e * GMX_L_NO + i) * k.HID + j] = o[((size_t)e * k.HID + j) * GMX_L_NO + i];
  }
  return GMX_OK;
}

// ---- record batches ------------------------------------------------------------------------
static int lstm_batch_alloc(gmx_lstm_batch** out, gmx_lstm* l, int S, uint64_t max_bytes) {
  if (!out || !l || max_bytes == 0) return GMX_ERR_INVALID;
  *out = nullptr;
  gmx_lstm_batch* b = new (std::nothrow) gmx_lstm_batch();
  if (!b) return GMX_ERR_NOMEM;
  b->back = (void**)&b->l;
  gmx_lstm_batch_cols(b->cols, b, GMX_L_NI);
  int rc = batch_core_alloc(*b, &l->bb, S, max_bytes, true);  // (the pinned arrays too: the accessors below never allocate)
  if (rc) {
    lstm_batch_free(b);
    return rc;
  }
  *out = b;
  return GMX_OK;
}
extern "C" int gmx_lstm_batch_create(gmx_lstm_batch** out, gmx_lstm* l, uint64_t max_bytes) {
  if (!l) return GMX_ERR_INVALID;
  int rc = lstm_batch_alloc(out, l, l->S, max_bytes);
  if (rc) return rc;
  return xfer_streams_ready(l->stream, &l->up_stream, &l->down_stream);
}
extern "C" void gmx_lstm_batch_destroy(gmx_lstm_batch* b) { lstm_batch_free(b); }
extern "C" float* gmx_lstm_batch_ppm(gmx_lstm_batch* b) { return (b && b->l) ? b->h_ppm : nullptr; }
extern "C" uint8_t* gmx_lstm_batch_bytes(gmx_lstm_batch* b) { return (b && b->l) ? b->h_bytes : nullptr; }
extern "C" const float* gmx_lstm_batch_predictions(gmx_lstm_batch* b) { return (b && b->l) ? b->h_pred : nullptr; }
extern "C" const uint8_t* gmx_lstm_batch_active(gmx_lstm_batch* b) { return (b && b->l) ? b->h_act : nullptr; }
extern "C" const uint32_t* gmx_lstm_batch_contexts(gmx_lstm_batch* b) { return (b && b->l) ? b->h_ctx : nullptr; }

// beside the kernels, on streams of their own (see gmx_batch_upload)
extern "C" int gmx_lstm_batch_upload(gmx_lstm_batch* b, uint64_t n_bytes) {
  return batch_core_transfer(b, n_bytes, GMX_COL_UP);
}
extern "C" int gmx_lstm_batch_download(gmx_lstm_batch* b, uint64_t n_bytes) {
  return batch_core_transfer(b, n_bytes, GMX_COL_DOWN);
}
extern "C" int gmx_lstm_batch_wait(gmx_lstm_batch* b) { return batch_core_wait(b); }  // this batch's upload, runs and download

// The host's share of a launch over bytes [0, n) of streams s0 .. s0 + ns - 1: Adam's scalars (lstm-layer.cpp:15-21,
// :27-32) of every backward pass the launch will run -- they depend on the step count only and are computed here with
// the libm the reference calls (powf, sqrtf), one row of `adam_host` ([ns][max_bptt][4]) per pass -- and the mirrors
// that say when passes fall (bytes_seen, update_steps).  n_list (nullable, [ns]): a byte count per stream.
static void lstm_stage_rows(gmx_lstm* l, int s0, int ns, uint64_t n_bytes, int learn, unsigned phases,
                            const uint64_t* n_list, float* adam_host, uint32_t max_bptt) {
  const float beta1 = 0.025, beta2 = 0.9999, learning_rate = l->shape.learning_rate;
  const unsigned long long limit = 3000;
  const uint64_t horizon = (uint64_t)l->shape.horizon;
  const bool perceives = learn && (phases & 4u);
  for (int i = 0; i < ns; ++i) {
    const int s = s0 + i;
    uint32_t steps = l->update_steps[s];
    uint32_t k = 0;
    const uint64_t nb = n_list ? n_list[i] : n_bytes;
    for (uint64_t n = 0; n < nb && perceives; ++n) {
      // Lstm::Perceive runs its backward pass when epoch_ has wrapped to 0 (lstm.cpp:57), and
      // epoch_ counts Lstm::Predict calls (learned from or not)
      if ((l->bytes_seen[s] + ((phases & 1u) ? n + 1 : 0)) % horizon != 0) continue;
      if (steps < limit) ++steps;
      const float t = (float)steps;
      float* row = adam_host + ((size_t)i * max_bptt + k) * 4;
      if (t < limit) {
        row[0] = learning_rate * 0.1f / sqrtf(5e-5f * t + 1.0f);
        row[1] = (float)(1.0f - powf(beta1, t));
        row[2] = (float)(1.0f - powf(beta2, t));
      } else {
        row[0] = learning_rate * 0.1f / sqrtf(5e-5f * limit + 1.0f);
        row[1] = (float)(1.0f - powf(beta1, limit));
        row[2] = (float)(1.0f - powf(beta2, limit));
      }
      row[3] = 0.0f;
      ++k;
    }
    if (perceives) l->update_steps[s] = steps;
    if (phases & 1u) l->bytes_seen[s] += nb;
    if (phases == 7u && nb) {  // a batched run: whole bytes, the bank stands where a byte ends afterwards
      l->range_read[s].valid = false;
      l->fwd_done[s] = 0;
    }
  }
}

static int lstm_launch(gmx_lstm* l, gmx_lstm_batch* b, int s0, int ns, uint64_t n_bytes, int learn, unsigned phases,
                       float* kernel_ms, int last_byte = -1, int rec0 = 0, const uint64_t* n_list = nullptr) {
  // n_list (host, [ns]): bytes of each stream of the range, at most n_bytes (one launch for streams of different lengths)
  // Adam's scalars (lstm-layer.cpp:15-21, :27-32) depend on the step count only: computed here
  // with the libm the reference calls (powf, sqrtf), one row per backward pass of each stream
  const uint32_t max_bptt = (uint32_t)(n_bytes / (uint64_t)l->shape.horizon + 2);
  const size_t need = (size_t)ns * max_bptt * 4;
  const int slot = (int)(l->adam_seq++ % gmx_lstm::kAdamSlots);
  if (l->adam_busy[slot]) {
    HIPCHK(hipEventSynchronize(l->adam_done[slot]));
    l->adam_busy[slot] = false;
  }
  if (need > l->adam_cap) {
    HIPCHK(hipStreamSynchronize(l->stream));  // (every slot is replaced: nothing may still read the old ones)
    for (int k = 0; k < gmx_lstm::kAdamSlots; ++k) {
      if (l->adam_host[k]) (void)hipHostFree(l->adam_host[k]);
      l->adam_dev[k] = nullptr;
      l->adam_host[k] = nullptr;
      l->adam_busy[k] = false;
    }
    l->adam_cap = 0;
    for (int k = 0; k < gmx_lstm::kAdamSlots; ++k) {
      // the kernel reads its few rows straight from pinned host memory (three floats per backward pass): a copy
      // on the bank's stream would be one more hand-shake between the kernels of neighbouring chunks
      HIPCHK(hipHostMalloc((void**)&l->adam_host[k], need * 4, hipHostMallocDefault));
      HIPCHK(hipHostGetDevicePointer((void**)&l->adam_dev[k], l->adam_host[k], 0));
      if (!l->adam_done[k]) HIPCHK(hipEventCreateWithFlags(&l->adam_done[k], hipEventDisableTiming));
    }
    l->adam_cap = need;
  }
  float* const adam_host = l->adam_host[slot];
  float* const adam_dev = l->adam_dev[slot];
  lstm_stage_rows(l, s0, ns, n_bytes, learn, phases, n_list, adam_host, max_bptt);
  GmxLstmRunArgs a;
  memset(&a, 0, sizeof a);
  a.banks = l->banks;
  // (block i works on bank s0 + i and on record stream rec0 + i)
  a.ppm = b->d_ppm + (size_t)rec0 * b->max_bytes * 256;
  a.bytes = b->d_bytes + (size_t)rec0 * b->max_bytes;
  a.adam = adam_dev;
  a.pred_out = b->d_pred + (size_t)rec0 * b->max_bytes * 8;
  a.act_out = b->d_act + (size_t)rec0 * b->max_bytes * 8;
  a.ctx_out = b->d_ctx + (size_t)rec0 * b->max_bytes;
  a.rec_stride = b->max_bytes;
  a.n_bytes = n_bytes;
  if (n_list) {
    int rcl = count_list_stage(l->counts, n_list, ns, l->stream, &a.n_list);
    if (rcl) return rcl;
  }
  a.learn = learn ? 1u : 0u;
  a.max_bptt = max_bptt;
  a.phases = phases;
  a.stream_base = s0;
  a.last_byte = last_byte;
  {
    int rcx = xfer_before_run(b->x, l->stream);  // the results of the previous run are out
    if (rcx) return rcx;
  }
  if (kernel_ms) HIPCHK(hipEventRecord(l->ev0, l->stream));
  if (l->any) {
    HIPCHK(gmx_launch_lstm_any_kernel(l->adev_d, &a, ns, l->stream));
    ++l->any_launches;
  } else {
    HIPCHK(gmx_launch_lstm_kernel(l->dev_d, &a, ns, l->cus, l->stream));
  }
  HIPCHK(hipEventRecord(l->adam_done[slot], l->stream));
  l->adam_busy[slot] = true;
  if (n_list) {
    int rcl = count_list_used(l->counts, l->stream);
    if (rcl) return rcl;
  }
  {
    int rcx = xfer_note_device_use(b->x, l->stream);
    if (rcx) return rcx;
  }
  if (kernel_ms) {
    HIPCHK(hipEventRecord(l->ev1, l->stream));
    HIPCHK(hipEventSynchronize(l->ev1));
    HIPCHK(hipEventElapsedTime(kernel_ms, l->ev0, l->ev1));
  }
  return GMX_OK;
}

// LstmModel::Predict for the 8 bits of each of n_bytes bytes (+ LstmModel::Learn, i.e.
// Lstm::Perceive with its backward pass every 100th byte, when learn != 0).
extern "C" int gmx_lstm_run(gmx_lstm* l, gmx_lstm_batch* b, uint64_t n_bytes, int learn, float* kernel_ms) {
  if (!l || !b || b->l != l || b->S != l->S || n_bytes > b->max_bytes) return GMX_ERR_INVALID;
  if (n_bytes == 0) return GMX_OK;
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  return lstm_launch(l, b, 0, l->S, n_bytes, learn, 7u, kernel_ms);
}

// The same for streams that stand at different lengths (files compressed side by side end at different bytes), in
// one launch (the kernel takes a count per block); a stream with 0 bytes sits out.
extern "C" int gmx_lstm_run_ragged(gmx_lstm* l, gmx_lstm_batch* b, const uint64_t* n_bytes, int learn) {
  if (!l || !b || b->l != l || b->S != l->S || !n_bytes) return GMX_ERR_INVALID;
  for (int s = 0; s < l->S; ++s)
    if (n_bytes[s] > b->max_bytes) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  uint64_t maxn = 0;
  bool same = true;
  for (int s = 0; s < l->S; ++s) {
    maxn = std::max(maxn, n_bytes[s]);
    same = same && n_bytes[s] == n_bytes[0];
  }
  if (maxn == 0) return GMX_OK;
  return lstm_launch(l, b, 0, l->S, maxn, learn, 7u, nullptr, -1, 0, same ? nullptr : n_bytes);
}

// ---- per-byte sessions (see GmxLstmSession above) -----------------------------------------------
static int lstm_session_start(gmx_lstm* l, int s) {
  GmxLstmSession* se = l->sessions[s];
  int rc = session_hw_start_prologue(se);
  if (rc) return rc;
  GmxLstmRunArgs a;
  memset(&a, 0, sizeof a);
  a.banks = l->banks;
  a.stream_base = s;
  a.last_byte = -1;
  a.max_bptt = 1;
  a.mc = se->mc;
  a.mb = se->mb;
  a.idle_ticks = kIdleTicks;
  HIPCHK(gmx_launch_lstm_session(l->dev_d, &a, se->stream));
  return GMX_OK;
}

static int lstm_session_dead(GmxLstmSession* se) {
  g_last_error = "per-byte LSTM session does not answer";
  se->pending_byte = -1;
  return GMX_ERR_HIP;
}

// Wait until the newest command has been completed, restarting the session if it left first (bounded).
static int lstm_session_wait(gmx_lstm* l, int s) {
  GmxLstmSession* se = l->sessions[s];
  int rc = mb_wait(se, kSessionTimeoutS, [&] { return lstm_session_start(l, s); });
  return rc == kMbDead ? lstm_session_dead(se) : rc;
}

// Make sure session s exists and runs.  GMX_ERR_STATE: no session slot is free (the caller uses the
// launch-per-call path); `force` starts one beyond the limit (a noted Perceive has no other way).
static int lstm_session_ensure(gmx_lstm* l, int s, bool force) {
  if (l->sessions.empty()) l->sessions.assign(l->S, nullptr);
  GmxLstmSession* se = l->sessions[s];
  if (se && se->dead) return lstm_session_dead(se);
  const bool running = se && se->launched && mb_load(se->state) == GMX_MB_RUNNING;
  if (!running && !(se && se->launched) && g_open_sessions.load() >= kMaxOpenSessions && !force) return GMX_ERR_STATE;
  if (!se) {
    se = new (std::nothrow) GmxLstmSession();
    if (!se) return GMX_ERR_NOMEM;
    l->sessions[s] = se;
    int rc = session_hw_alloc(se, sizeof(GmxLstmMbCmd), sizeof(GmxLstmMbReply), true, l->device);
    se->mc = (GmxLstmMbCmd*)se->cmd_seq;
    se->mb = (GmxLstmMbReply*)se->done_seq;
    if (rc) return rc;
  }
  if (!running) {
    HIPCHK(hipStreamSynchronize(l->stream));  // batched work on the bank is finished
    return lstm_session_start(l, s);
  }
  return GMX_OK;
}

static void lstm_session_put_perceive(GmxLstmSession* se) {
  se->mc->byte = (uint32_t)se->pending_byte;
  for (int i = 0; i < 4; ++i) se->mc->adam[i] = se->pending_adam[i];
  se->pending_byte = -1;
}

// A Perceive that gmx_lstm_perceive noted and no forward has taken along yet: send it on its own.
static int lstm_session_flush(gmx_lstm* l, int s) {
  GmxLstmSession* se = s < (int)l->sessions.size() ? l->sessions[s] : nullptr;
  if (!se || se->pending_byte < 0) return GMX_OK;
  int rc = lstm_session_ensure(l, s, true);
  if (rc) return rc;
  rc = lstm_session_wait(l, s);
  if (rc) return rc;
  lstm_session_put_perceive(se);
  mb_publish(se, 0, GMX_MB_LEARN0);
  return GMX_OK;
}

static int lstm_session_stop(gmx_lstm* l, int s) {
  GmxLstmSession* se = s < (int)l->sessions.size() ? l->sessions[s] : nullptr;
  if (!se) return GMX_OK;
  if (se->dead) return lstm_session_dead(se);
  int rc = lstm_session_flush(l, s);
  if (rc) return rc;
  return session_hw_stop(se, [&] { return lstm_session_wait(l, s); });
}

static int lstm_sessions_close(gmx_lstm* l) {
  return sessions_stop_each(l->sessions.size(), [&](int s) { return lstm_session_stop(l, s); });
}

static void lstm_sessions_free(gmx_lstm* l) {
  (void)lstm_sessions_close(l);
  // (a block that is still there writes the model's state into the bank: gmx_lstm_destroy leaks it)
  if (!sessions_release_each(l->sessions)) l->banks_in_use_by_dead_kernel = true;
}

// Adam's scalars of the backward pass the Perceive of the byte just predicted runs, if it runs one
// (lstm_launch has the same for a batch): Lstm::Perceive runs it when epoch_ has wrapped to 0 (lstm.cpp:57).
static void lstm_perceive_scalars(gmx_lstm* l, int s, float row[4]) {
  row[0] = row[1] = row[2] = row[3] = 0.0f;
  if (l->bytes_seen[s] % (uint64_t)l->shape.horizon != 0) return;
  const float beta1 = 0.025, beta2 = 0.9999, learning_rate = l->shape.learning_rate;
  const unsigned long long limit = 3000;
  uint32_t steps = l->update_steps[s];
  if (steps < limit) ++steps;
  const float t = (float)steps;
  if (t < limit) {
    row[0] = learning_rate * 0.1f / sqrtf(5e-5f * t + 1.0f);
    row[1] = (float)(1.0f - powf(beta1, t));
    row[2] = (float)(1.0f - powf(beta2, t));
  } else {
    row[0] = learning_rate * 0.1f / sqrtf(5e-5f * limit + 1.0f);
    row[1] = (float)(1.0f - powf(beta1, limit));
    row[2] = (float)(1.0f - powf(beta2, limit));
  }
  l->update_steps[s] = steps;
}

static int lstm_session_forward(gmx_lstm* l, int s, int last_byte, const float* ppm, float* probs, uint32_t* context) {
  int rc = lstm_session_ensure(l, s, false);
  if (rc) return rc;
  GmxLstmSession* se = l->sessions[s];
  rc = lstm_session_wait(l, s);  // the previous command is done with the payload
  if (rc) return rc;
  memcpy((void*)se->mc->ppm, ppm, GMX_L_NI * 4);
  se->mc->last_byte = (uint32_t)last_byte;
  uint32_t cmd = GMX_MB_FORWARD;
  if (se->pending_byte >= 0) {
    lstm_session_put_perceive(se);
    cmd = GMX_MB_LEARN0_FWD;
  }
  mb_publish(se, 0, cmd);
  rc = lstm_session_wait(l, s);
  if (rc) return rc;
  if (probs) memcpy(probs, (const void*)se->mb->probs, GMX_L_NO * 4);
  if (context) *context = se->mb->context;
  return GMX_OK;
}

// ---- per-byte surface (decode: a byte is not known when its prediction is needed) -----------
static int lstm_ensure_one(gmx_lstm* l) {
  if (l->one) return GMX_OK;
  // a one-stream, one-byte batch; its record arrays serve whichever stream is stepped
  return lstm_batch_alloc(&l->one, l, 1, 1);
}

extern "C" int gmx_lstm_forward(gmx_lstm* l, int stream, int last_byte, const float* ppm, float* probs,
                                uint32_t* context) {
  if (!l || stream < 0 || stream >= l->S || !ppm || last_byte < 0 || last_byte > 255) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(l->device));
  if (l->use_sessions) {
    int rcs = lstm_session_forward(l, stream, last_byte, ppm, probs, context);
    if (rcs == GMX_OK) {
      l->bytes_seen[stream] += 1;
      l->range_read[stream].valid = false;
      l->fwd_done[stream] = 2;  // 2: through the session
      return GMX_OK;
    }
    if (rcs != GMX_ERR_STATE) return rcs;  // GMX_ERR_STATE: no session slot free, launch instead
  }
  LSTM_CLOSE_SESSIONS(l);
  int rc = lstm_ensure_one(l);
  if (rc) return rc;
  gmx_lstm_batch* b = l->one;
  HIPCHK(hipStreamSynchronize(l->stream));
  memcpy(b->h_ppm, ppm, GMX_L_NI * 4);
  HIPCHK(hipMemcpyAsync(b->d_ppm, b->h_ppm, GMX_L_NI * 4, hipMemcpyHostToDevice, l->stream));
  rc = lstm_launch(l, b, stream, 1, 1, 0, 1u, nullptr, last_byte);
  if (rc) return rc;
  const float* bank = l->banks + (size_t)stream * l->dev.bank_floats;
  uint32_t scal[8];
  if (probs) HIPCHK(hipMemcpyAsync(probs, bank + l->dev.probs, GMX_L_NO * 4, hipMemcpyDeviceToHost, l->stream));
  HIPCHK(hipMemcpyAsync(scal, bank + l->dev.scal, sizeof scal, hipMemcpyDeviceToHost, l->stream));
  HIPCHK(hipStreamSynchronize(l->stream));
  if (context) *context = scal[4];
  l->range_read[stream].valid = false;
  l->fwd_done[stream] = 1;
  return GMX_OK;
}

extern "C" int gmx_lstm_perceive(gmx_lstm* l, int stream, int byte) {
  if (!l || stream < 0 || stream >= l->S || byte < 0 || byte > 255) return GMX_ERR_INVALID;
  if (!l->fwd_done[stream]) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(l->device));
  if (l->fwd_done[stream] == 2) {
    // through the session: noted here, published with the next forward (or by whatever touches the bank next)
    GmxLstmSession* se = l->sessions[stream];
    se->pending_byte = byte;
    lstm_perceive_scalars(l, stream, se->pending_adam);
    l->range_read[stream].valid = false;
    l->fwd_done[stream] = 0;
    return GMX_OK;
  }
  {
    int rc1 = lstm_ensure_one(l);  // (the forward may have been another bank's: a copy, a checkpoint)
    if (rc1) return rc1;
  }
  gmx_lstm_batch* b = l->one;
  HIPCHK(hipStreamSynchronize(l->stream));
  b->h_bytes[0] = (uint8_t)byte;
  HIPCHK(hipMemcpyAsync(b->d_bytes, b->h_bytes, 1, hipMemcpyHostToDevice, l->stream));
  int rc = lstm_launch(l, b, stream, 1, 1, 1, 4u, nullptr);
  if (rc) return rc;
  // not waited for (see gmx_indirect_learn): the next call on this bank synchronises its stream first
  l->range_read[stream].valid = false;
  l->fwd_done[stream] = 0;
  return GMX_OK;
}

extern "C" int gmx_debug_lstm_use_sessions(gmx_lstm* l, int on) {
  if (!l) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  l->use_sessions = on != 0 && !l->any;  // (a bank on the general layout never starts a session)
  return GMX_OK;
}

// ---- into the downstream models' batches (device to device) --------------------------------
struct GmxLstmScatterArgs {
  const float* pred;
  const uint8_t* act;
  const uint32_t* ctx;
  uint64_t rec_stride, n_bytes;
  float* mx_pred;
  uint32_t* mx_mask;
  uint32_t* mx_ctx;
  uint64_t mx_stride;
  int32_t mx_n_pad, mx_mask_words, mx_m, slot, mixer_ctx_col;
  uint32_t* ind_ctx;
  uint64_t ind_stride;
  int32_t ind_k, ind_ctx_col;
};
extern "C" hipError_t gmx_launch_lstm_scatter(const GmxLstmScatterArgs* args, int n_streams, hipStream_t stream);

extern "C" int gmx_lstm_feed(gmx_lstm* l, gmx_lstm_batch* b, uint64_t n_bytes, gmx_batch* mixer_batch, int slot,
                             int mixer_ctx_col, gmx_ind_batch* ind_batch, int ind_ctx_col) {
  if (!l || !b || b->l != l || b->S != l->S || n_bytes > b->max_bytes || (!mixer_batch && !ind_batch))
    return GMX_ERR_INVALID;
  GmxLstmScatterArgs a;
  memset(&a, 0, sizeof a);
  a.pred = b->d_pred;
  a.act = b->d_act;
  a.ctx = b->d_ctx;
  a.rec_stride = b->max_bytes;
  a.n_bytes = n_bytes;
  a.mixer_ctx_col = -1;
  if (mixer_batch) {
    gmx_batch* m = mixer_batch;
    if (!m->g || m->S != l->S || m->g->device != l->device || n_bytes * 8 > m->max_bits || !m->d_mask || slot < 0 ||
        slot >= m->g->topo.n || mixer_ctx_col >= m->g->topo.m)
      return GMX_ERR_INVALID;
    a.mx_pred = m->d_pred;
    a.mx_mask = m->d_mask;
    a.mx_ctx = m->d_ctx;
    a.mx_stride = m->max_bits;
    a.mx_n_pad = m->g->topo.n_pad;
    a.mx_mask_words = m->g->topo.mask_words;
    a.mx_m = m->g->topo.m;
    a.slot = slot;
    a.mixer_ctx_col = mixer_ctx_col;
  }
  if (ind_batch) {
    gmx_ind_batch* ib = ind_batch;
    if (!ib->ib || ib->S != l->S || ib->ib->device != l->device || n_bytes * 8 > ib->max_bits || ind_ctx_col < 0 ||
        ind_ctx_col >= ib->ib->dev.k)
      return GMX_ERR_INVALID;
    a.ind_ctx = ib->d_ctx;
    a.ind_stride = ib->max_bits;
    a.ind_k = ib->ib->dev.k;
    a.ind_ctx_col = ind_ctx_col;
  }
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  // ordered after the consumers' batches' own uploads / last uses, and before the consumers' next work.  (On the
  // bank's own stream: a stream of its own for the scatter was tried -- the LSTM kernels of neighbouring chunks then
  // no longer have it between them -- and lost: 3.3 instead of 3.15 us per bit for one compressor, the hand-shakes
  // between three streams cost more than the one in line.)
  hipStream_t fs = l->stream;
  if (mixer_batch) {
    int rcw = xfer_writer_waits(mixer_batch->x, fs);
    if (rcw) return rcw;
  }
  if (ind_batch) {
    int rcw = xfer_writer_waits(ind_batch->x, fs);
    if (rcw) return rcw;
  }
  HIPCHK(gmx_launch_lstm_scatter(&a, l->S, fs));
  if (mixer_batch) {
    int rcn = xfer_writer_done(mixer_batch->x, fs, mixer_batch->g->stream);
    if (rcn) return rcn;
  }
  if (ind_batch) {
    int rcn = xfer_writer_done(ind_batch->x, fs, ind_batch->ib->stream);
    if (rcn) return rcn;
  }
  return xfer_note_device_use(b->x, fs);  // the scatter read this batch's results
}

// ---- persistence ---------------------------------------------------------------------------
// The model's stretch of the `.short` file -- LstmModel::WriteToDisk (lstm-model.cpp:62-68) with
// Lstm::WriteToDisk (lstm.cpp:124-140), LstmLayer::WriteToDisk (lstm-layer.cpp:356-374) and the
// three NeuronLayer::WriteToDisk (lstm-layer.cpp:62-91) behind it -- and the LSTM section of
// LongTermMemory::WriteToDisk (long-term-memory.cpp:57-67) of the `.long` file: raw arrays in
// declaration order, no headers.  A bank stands at a byte boundary, so top_/mid_/bot_ are what
// the eighth LstmModel::Predict of the last coded byte left (lstm-model.cpp:34-41).
namespace {

size_t lstm_long_bytes(const LstmDims& k) { return ((size_t)k.H * GMX_L_NO * k.HID + 3u * (size_t)k.NC * k.W) * 4u; }

// One pass over the `.short` layout; `dir` false: bank image -> file bytes, true: file -> image.
struct LstmShortIo {
  const GmxLstmDev& d;
  const LstmDims& k;
  std::vector<float>& img;  // host copy of one bank
  uint8_t* buf;             // file bytes (null: count only)
  bool rd;
  size_t off = 0;
  void raw(void* host, size_t n) {
    if (buf) {
      if (rd) memcpy(host, buf + off, n);
      else memcpy(buf + off, host, n);
    }
    off += n;
  }
  // `rows` rows of `n` floats, stored in the bank `pitch` floats apart
  void rows(uint64_t at, int rows_, int n, int pitch) {
    for (int r = 0; r < rows_; ++r) raw(&img[at + (uint64_t)r * pitch], (size_t)n * 4);
  }
  // a reference [cell][W] matrix, stored in the bank input-major (LstmDims::mat)
  void cell_major(uint64_t at) {
    for (int i = 0; i < k.NC; ++i)
      for (int j = 0; j < k.W; ++j) raw(&img[at + k.mat(j, i)], 4);
  }
};

size_t lstm_short_io(const GmxLstmDev& d, const LstmDims& k, std::vector<float>& img, uint8_t* buf, bool rd,
                     int32_t tmb[3], uint32_t* epoch, uint32_t* l_epoch, uint64_t* update_steps) {
  LstmShortIo io{d, k, img, buf, rd};
  const int H = k.H, NC = k.NC, CP = k.CP;
  io.raw(tmb, 12);
  io.rows(d.probs, 1, GMX_L_NO, 0);
  io.rows(d.input_history, 1, H, 0);
  io.rows(d.hidden, 1, k.HID, 0);
  io.rows(d.hidden_error, 1, NC, 0);
  io.rows(d.layer_input, H, k.LIN, k.LINP);
  io.rows(d.output, H, GMX_L_NO, GMX_L_NO);
  io.raw(epoch, 4);
  io.rows(d.state, 1, NC, 0);
  io.rows(d.state_error, 1, NC, 0);
  io.rows(d.stored_error, 1, NC, 0);
  io.rows(d.tanh_state, H, NC, CP);
  io.rows(d.input_gate_state, H, NC, CP);
  io.rows(d.last_state, H, NC, CP);
  io.raw(l_epoch, 4);
  io.raw(update_steps, 8);
  for (int g = 0; g < 3; ++g) {
    const GmxLstmGateOff& o = d.gate[g];
    // error_: what the last step (epoch 0) of the last backward pass left (lstm-layer.cpp:311-316); the general
    // layout keeps the vector itself
    io.rows(k.any ? o.error : d.errs + (uint64_t)g * H * CP, 1, NC, 0);
    io.rows(o.ivar, 1, H, 0);
    const uint64_t vecs[] = {o.gamma, o.gamma_u, o.gamma_m, o.gamma_v, o.beta, o.beta_u, o.beta_m, o.beta_v};
    for (uint64_t v : vecs) io.rows(v, 1, NC, 0);
    io.rows(o.state, H, NC, CP);
    io.cell_major(o.update);
    io.cell_major(o.m);
    io.cell_major(o.v);
    io.rows(o.transpose, k.HID, NC, CP);
    io.rows(o.norm, H, NC, CP);
  }
  return io.off;
}

size_t lstm_long_io(const GmxLstmDev& d, const LstmDims& k, std::vector<float>& img, uint8_t* buf, bool rd) {
  LstmShortIo io{d, k, img, buf, rd};
  // lstm_output_layer[epoch][symbol][hidden], stored in the bank as [epoch][hidden][symbol]
  for (int e = 0; e < k.H; ++e)
    for (int i = 0; i < GMX_L_NO; ++i)
      for (int j = 0; j < k.HID; ++j) io.raw(&img[d.out_layer + ((uint64_t)e * k.HID + j) * GMX_L_NO + i], 4);
  for (int g = 0; g < 3; ++g) io.cell_major(d.gate[g].weights);
  return io.off;
}

}  // namespace

extern "C" int gmx_lstm_export(gmx_lstm* l, int stream, void* long_buf, size_t* long_bytes, void* short_buf,
                               size_t* short_bytes) {
  if (!l || stream < 0 || stream >= l->S || !long_bytes || !short_bytes) return GMX_ERR_INVALID;
  std::vector<float> img(l->dev.bank_floats);
  int32_t tmb[3] = {255, 127, 0};
  uint32_t epoch = 0, l_epoch = 0;
  uint64_t steps = 0;
  const LstmDims k = lstm_dims(l);
  const size_t need_long = lstm_long_bytes(k);
  const size_t need_short = lstm_short_io(l->dev, k, img, nullptr, false, tmb, &epoch, &l_epoch, &steps);
  if (!long_buf && !short_buf) {
    *long_bytes = need_long;
    *short_bytes = need_short;
    return GMX_OK;
  }
  if ((long_buf && *long_bytes < need_long) || (short_buf && *short_bytes < need_short)) {
    *long_bytes = need_long;
    *short_bytes = need_short;
    return GMX_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  HIPCHK(hipStreamSynchronize(l->stream));
  HIPCHK(hipMemcpy(img.data(), l->banks + (size_t)stream * l->dev.bank_floats, img.size() * 4, hipMemcpyDeviceToHost));
  const uint32_t* scal = (const uint32_t*)&img[l->dev.scal];
  epoch = scal[0];
  l_epoch = scal[1];
  steps = scal[2];
  if (l->range_read[stream].valid) {
    memcpy(tmb, l->range_read[stream].tmb, sizeof tmb);  // nothing has moved since this bank was read from a file
  } else if (l->fwd_done[stream]) {
    // between Lstm::Predict and Lstm::Perceive of a byte (LstmModel::WriteToDisk works at any bit,
    // lstm-model.cpp:62-68; the reference's TestGeneration checkpoints there, tester.cpp:284, :312): the network's
    // state is what the forward left.  The range state is the caller's from here on (it codes the byte's bits on the
    // host, lstm-model.cpp:34-48): written as the forward's own Predict leaves it, top_ 255 / mid_ 127 / bot_ 0
  } else if (scal[6]) {  // range of the eighth bit of the last coded byte: [b & ~1, b | 1], mid_ = bot_
    tmb[2] = (int32_t)(scal[3] & 0xfeu);
    tmb[1] = tmb[2];
    tmb[0] = tmb[2] + 1;
  }
  if (long_buf) *long_bytes = lstm_long_io(l->dev, k, img, (uint8_t*)long_buf, false);
  if (short_buf) *short_bytes = lstm_short_io(l->dev, k, img, (uint8_t*)short_buf, false, tmb, &epoch, &l_epoch, &steps);
  return GMX_OK;
}

extern "C" int gmx_lstm_import(gmx_lstm* l, int stream, const void* long_buf, size_t long_bytes,
                               const void* short_buf, size_t short_bytes) {
  if (!l || stream < 0 || stream >= l->S || !long_buf || !short_buf) return GMX_ERR_INVALID;
  std::vector<float> img(l->dev.bank_floats, 0.0f);
  int32_t tmb[3] = {255, 127, 0};
  uint32_t epoch = 0, l_epoch = 0;
  uint64_t steps = 0;
  const LstmDims k = lstm_dims(l);
  if (long_bytes != lstm_long_bytes(k) ||
      short_bytes != lstm_short_io(l->dev, k, img, nullptr, true, tmb, &epoch, &l_epoch, &steps))
    return GMX_ERR_FORMAT;
  const GmxLstmDev& d = l->dev;
  lstm_long_io(d, k, img, (uint8_t*)const_cast<void*>(long_buf), true);
  lstm_short_io(d, k, img, (uint8_t*)const_cast<void*>(short_buf), true, tmb, &epoch, &l_epoch, &steps);
  const float* probs = &img[d.probs];
  // a model nobody has run: the constructor's range and byte distribution (lstm-model.cpp:7-10)
  bool fresh = tmb[0] == 255 && tmb[1] == 127 && tmb[2] == 0;
  for (int i = 0; fresh && i < GMX_L_NO; ++i) fresh = probs[i] == 1.0f / 256;
  // where a byte ends the range is that of its eighth bit: [b & ~1, b | 1], mid_ = bot_.  Anything else is a
  // checkpoint taken inside a byte (LstmModel::WriteToDisk works at any bit): the forward of that byte is done,
  // its Perceive still to come
  const bool boundary = !fresh && tmb[2] >= 0 && tmb[2] <= 254 && !(tmb[2] & 1) && tmb[1] == tmb[2] && tmb[0] == tmb[2] + 1;
  if (epoch >= (uint32_t)k.H || l_epoch >= (uint32_t)k.H || steps > 3000 ||
      !(0 <= tmb[2] && tmb[2] <= tmb[1] && tmb[1] <= tmb[0] && tmb[0] <= 255))
    return GMX_ERR_FORMAT;
  // what the file leaves implicit: the constant inputs, the input-major copy of the layer inputs,
  // and the blackboard values LstmModel::Predict derives from probs_ (lstm-model.cpp:25-47)
  img[d.hidden + k.HID - 1] = 1.0f;  // hidden_[num_cells] (lstm.cpp:31) -- also in the file; kept as read
  for (int e = 0; e < GMX_L_H && !k.any; ++e)  // (the general layout has no input-major copy)
    for (int j = 0; j < GMX_L_LIN; ++j)
      img[d.lin_t + (uint64_t)j * GMX_L_HP + e] = img[d.layer_input + (uint64_t)e * GMX_L_LINP + j];
  uint32_t* scal = (uint32_t*)&img[d.scal];
  const uint32_t* hist = (const uint32_t*)&img[d.input_history];
  scal[0] = epoch;
  scal[1] = l_epoch;
  scal[2] = (uint32_t)steps;
  uint32_t last_byte = 0, context = 0;
  float prediction = 0.0f;
  if (!fresh) {
    // the byte itself is ShortTermMemory's to remember; Lstm::Perceive left it in input_history_ (one entry further
    // back when this byte's forward has already advanced epoch_)
    const uint32_t newest = hist[(epoch + (uint32_t)k.H - (boundary ? 1 : 2)) % (uint32_t)k.H];
    if (boundary)
      last_byte = (newest < 256 && (int32_t)(newest & 0xfeu) == tmb[2]) ? newest : (uint32_t)tmb[2];
    else
      last_byte = newest < 256 ? newest : 0;
    float max_pred = 0;
    for (int i = 0; i < GMX_L_NO; ++i)
      if (probs[i] > max_pred) {
        max_pred = probs[i];
        context = (uint32_t)i;
      }
    float num = 0.0f;  // lstm-model.cpp:41-47 on the range as read
    for (int i = tmb[1] + 1; i <= tmb[0]; ++i) num += probs[i];
    float denom = num;
    for (int i = tmb[2]; i <= tmb[1]; ++i) denom += probs[i];
    if (denom != 0) {
      float p = num / denom;  // Sigmoid::Logit (sigmoid.cpp:7-13)
      if (p < 0.0001) p = 0.0001;
      else if (p > 0.9999) p = 0.9999;
      prediction = logf(p / (1 - p));
    }
  }
  scal[3] = last_byte;
  scal[4] = context;
  memcpy(&scal[5], &prediction, 4);
  scal[6] = fresh ? 0u : 1u;
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  HIPCHK(hipStreamSynchronize(l->stream));
  HIPCHK(hipMemcpy(l->banks + (size_t)stream * d.bank_floats, img.data(), img.size() * 4, hipMemcpyHostToDevice));
  l->bytes_seen[stream] = epoch;  // only its value mod 100 matters (lstm_launch)
  l->update_steps[stream] = (uint32_t)steps;
  // the file does not say whether the newest forward has been perceived (the reference keeps no such flag: where the
  // byte stands is ShortTermMemory's knowledge), so a Perceive is accepted next unless the model is untouched
  l->fwd_done[stream] = fresh ? 0 : 1;
  l->range_read[stream].valid = true;
  memcpy(l->range_read[stream].tmb, tmb, sizeof tmb);
  return GMX_OK;
}

// LstmModel::Copy (lstm-model.cpp:78-85) + the LSTM share of LongTermMemory::Copy
// (long-term-memory.cpp:216-219): the whole bank, device to device.
extern "C" int gmx_lstm_copy(gmx_lstm* dst, int dst_stream, gmx_lstm* src, int src_stream) {
  if (!dst || !src || dst_stream < 0 || dst_stream >= dst->S || src_stream < 0 || src_stream >= src->S)
    return GMX_ERR_INVALID;
  if (dst->any != src->any || memcmp(&dst->shape, &src->shape, sizeof dst->shape) != 0) return GMX_ERR_INVALID;
  if (dst == src && dst_stream == src_stream) return GMX_OK;
  HIPCHK(hipSetDevice(src->device));
  LSTM_CLOSE_SESSIONS(src);
  HIPCHK(hipStreamSynchronize(src->stream));
  HIPCHK(hipSetDevice(dst->device));
  LSTM_CLOSE_SESSIONS(dst);
  HIPCHK(hipStreamSynchronize(dst->stream));
  HIPCHK(hipMemcpy(dst->banks + (size_t)dst_stream * dst->dev.bank_floats,
                   src->banks + (size_t)src_stream * src->dev.bank_floats, src->dev.bank_floats * 4,
                   hipMemcpyDefault));
  dst->bytes_seen[dst_stream] = src->bytes_seen[src_stream];
  dst->update_steps[dst_stream] = src->update_steps[src_stream];
  dst->fwd_done[dst_stream] = src->fwd_done[src_stream] ? 1 : 0;  // (a copy taken inside a byte: its Perceive is still to come)
  dst->range_read[dst_stream] = src->range_read[src_stream];
  return GMX_OK;
}

// LstmModel::GetMemoryUsage (lstm-model.cpp:87-101) with Lstm:: (lstm.cpp:173-184), LstmLayer::
// (lstm-layer.cpp:411-423) and NeuronLayer::GetMemoryUsage (lstm-layer.cpp:144-154) for the one
// shape the reference builds.
extern "C" int gmx_lstm_memory_usage(gmx_lstm* l, uint64_t* bytes) {
  if (!l || !bytes) return GMX_ERR_INVALID;
  const LstmDims k = lstm_dims(l);
  const uint64_t H = k.H, NC = k.NC, W = k.W, NO = GMX_L_NO, HID = k.HID, LIN = k.LIN;
  const uint64_t neuron = 4 + 40 * NC + 4 * H * NC + 3 * (4 * NC * W) + 4 * (W - NO - GMX_L_NI) * NC + 4 * H * NC;
  const uint64_t layer = 44 + 3 * (4 * NC) + 3 * (4 * H * NC) + 3 * neuron;
  const uint64_t lstm = 24 + 4 * H + 4 * HID + 4 * NC + 4 * H * LIN + 4 * H * NO + layer;
  *bytes = 16 + 256 * 4 + 4 * H * NO * HID + 3 * (4 * NC * W) + lstm;
  return GMX_OK;
}
