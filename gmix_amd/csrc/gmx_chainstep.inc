// gmx_chainstep.inc -- S decoders in lock step through ALL device-side models: one device step per coded bit
// (included by gmx_capi.cpp behind gmx_lockstep.inc, gmx_indirect.inc and gmx_lstm.inc).
//
// A decoder learns its bit from Predict's own result (coder/decoder.cpp:19-39), so the files of a many-file
// decompression advance together, a bit per step.  gmx_lockstep_* does that for the mixers alone; here the LSTM byte
// model and the Indirect models step with them, so that -- as in the run-ahead compressor -- 83 of the mixers' 90
// inputs never leave the device.  One step, for every stream that asks (what[s]):
//
//   GMX_STEP_LEARN    Predictor::Learn of the bit the stream decoded from the last step's probability (bits[s]):
//                     Mixer::Learn x M from the latched forward, Indirect::Learn x K on the latched table entries,
//                     and -- when that bit completes a byte -- Lstm::Perceive(byte)
//   GMX_STEP_PREDICT  Predictor::Predict of the next bit: Lstm::Predict on the caller's PPM distribution when the bit
//                     opens a byte, LstmModel::Predict's range walk for the bit, Indirect::Predict x K on the caller's
//                     contexts, Mixer::Predict x M on the caller's record with the device-side models' slots filled in
//
// With a Match bank attached (gmx_chainstep_attach_match) a step is also the history push of BasicContexts::Learn and
// Match::Learn x K, then Match::Predict x K, of every stream that asks (gmx_match_step.h): in lanes 56..63 of the Indirect
// models' launch, or -- without Indirect models, or with more than 56 -- in gmx_match_step_kernel in front of the mixers'.
// Then 89 of the 90 inputs and the gate contexts of mixers 6 and 30 never leave the device; the host supplies the bit
// context per predict and the models' context words per byte-opening predict.
//
// With a context bank attached (gmx_chainstep_attach_ctx) the step begins with gmx_ctx_step_kernel (gmx_ctx_step.h): the
// bank takes the stream's bit and writes the routed context columns, the Match models' context words and the bit context
// of this step's device copy, so the host supplies none of them and the arrays it owns no column of leave the slices.
//
// as ONE hipGraph of kernels only.  No copy node: a graph's small memcpy nodes cost 9-11 us EACH on this part
// (scripts/trace_chainstep.sh: three uploads and a download were 35 of a step's 53 us).
//
// How a step's inputs reach the device.  Control words (bits, what, decay factors, the step's number) and records live
// in one block, of which the device holds TWO copies used alternately: Mixer::Learn works on the records of the forward
// it learns from, which are the step before's, so the learn reads the other copy.  (Hence a stream with a forward
// outstanding may not sit a step out: its record would be two copies old.)  Where the host can store into device memory
// (large BAR) the copies are fine-grained device memory and the HOST writes them: gmx_chainstep_commit(cs, s) -- callable
// by S threads at once, each for its own streams -- copies stream s's records from the pinned staging arrays the accessors
// hand out, 700 bytes of posted writes; gmx_chainstep_step does it for whoever did not, and adds the control words.
// Reads across the link by the device itself are what this replaced: the link answers about 100 M small reads a
// second whoever asks (a copy kernel, or every block fetching its own slices), 7 us at 64 streams and 25 at 256.
// Without a large BAR (or with GMX_CS_NO_BAR) the step's first kernel fetches them (gmx_step_upload, gmx_step_dev.h).
//
// With the reference's own mixer shape a step that opens no byte is TWO launches -- the LSTM's bit prediction and the
// Indirect models in one (gmx_indirect_step_kernel), Mixer::Learn and Mixer::Predict in the other
// (gmx_stock_step_kernel: the rows stay in registers in between).  The probabilities and outputs are stored straight
// into pinned host memory by the mixers' kernel, every block stamping the step's number behind its own: those S stamps
// are what gmx_chainstep_step waits for, not the stream (hipStreamSynchronize came back 12 us after the last kernel
// had ended).  Steps that open a byte take a graph with the LSTM's two launches in it: four graphs in all (parity x
// opens).  Same floats as every other surface (tests/test_gpu_chainstep.py: against the oracle chain; the reference's
// own Decoder on top of it in dropin/, tests/test_gpu_batched.py).

extern "C" hipError_t gmx_launch_indirect_step(const GmxIndDev* dv, const GmxIndStepArgs* args, int n_streams,
                                               hipStream_t stream);
extern "C" hipError_t gmx_launch_lstm_bitstep(const GmxLstmDev* dv, const GmxLstmBitArgs* args, int n_streams,
                                              hipStream_t stream);
extern "C" hipError_t gmx_launch_copy16(void* dst, const void* src, uint64_t n16, hipStream_t stream);
extern "C" hipError_t gmx_launch_step_upload(const GmxStepUpload* u, int n_streams, hipStream_t stream);
extern "C" hipError_t gmx_launch_stock_step(const GmxTopoDev* tp_dev, const GmxStkStepArgs* args, unsigned lds_bytes,
                                            hipStream_t stream);
extern "C" hipError_t gmx_launch_models_step(const GmxIndDev* dv, const GmxIndStepArgs* args, const GmxLstmDev* ldv,
                                             const GmxLstmBitArgs* largs, int n_streams, hipStream_t stream);
extern "C" hipError_t gmx_launch_models_step_match(const GmxIndDev* dv, int k_ind, const GmxIndStepArgs* args,
                                                   const GmxLstmDev* ldv, const GmxLstmBitArgs* largs,
                                                   const GmxMatchDev* mdv, const GmxMatchStepArgs* margs, int n_streams,
                                                   hipStream_t stream);
extern "C" hipError_t gmx_launch_match_step(const GmxMatchDev* dv, const GmxMatchStepArgs* args, hipStream_t stream);
extern "C" hipError_t gmx_launch_coder_step(const GmxCtxDev* dv, const GmxCoderStepArgs* args, hipStream_t stream);
extern "C" hipError_t gmx_launch_coder_tail(const GmxCoderStepArgs* args, hipStream_t stream);

// The device arithmetic decoder of a lock-step object (gmx_chainstep_attach_decoder, gmx_coder.inc).
struct gmx_cs_decoder {
  int ppmd_slot = -1;
  GmxCoderStream* streams = nullptr;      // device [S]
  std::vector<uint8_t*> input;            // device: the streams' compressed payloads
  GmxCoderByteIn* h_in = nullptr;         // pinned [S]: what the host says per byte ...
  GmxCoderByteIn* in_dev = nullptr;       // ... where the byte's first step reads it (device memory the host stores into,
  GmxCoderByteIn* in_bar = nullptr;       //     where there is such a thing: in_bar; else the pinned block itself)
  float* p_dev = nullptr;                 // device [S]: the mixers' p of the step before
  float* outs_dev = nullptr;              // device [S][M]: the mixers' outputs of a byte graph's steps (nobody reads them)
  uint32_t* stamp_dev = nullptr;          // device [S]: ... and their stamps
  uint8_t* h_ans = nullptr;               // pinned: take [S] | decoded [S] | byte_p [S][8] | state [S][4]
  uint8_t *take = nullptr, *decoded = nullptr;
  float* byte_p = nullptr;
  uint32_t* state = nullptr;
  uint8_t* ans_dev = nullptr;
  std::vector<GmxCoderState> st;          // the state after the last answered byte (or as set)
  std::vector<uint8_t> has_input, via_byte, taking;
  hipGraph_t graph[2] = {};               // [parity of the byte's first step]
  hipGraphExec_t exec[2] = {};
  bool in_flight = false;                 // the step in flight is a byte
};

// Where a byte graph's steps put what a per-bit step hands to the host, and which step of the byte is recorded.
struct CsByteRoute {
  int j;            // 1..8
  float* p;         // device [S]
  float* outs;      // device [S][M]
  uint32_t* stamp;  // device [S]
};

struct gmx_chainstep {
  gmx_group* g = nullptr;
  gmx_indirect* ib = nullptr;
  gmx_lstm* l = nullptr;
  gmx_match* mb = nullptr;         // gmx_chainstep_attach_match: the Match models step on the device too
  bool mb_gone = false;            // ... and that bank has been destroyed: the captured steps would write freed memory
  int n_mcols = 0;                 // mixer context columns that receive longest_match
  int32_t mcols[GMX_MATCH_MAX_CTX_COLS] = {};
  uint32_t* mctx = nullptr;        // host view [S][K_match]: the Match models' context words (room for 8 a stream)
  std::vector<uint32_t> m_bc;      // bit_context of the stream's outstanding Predict (does its Learn complete a byte?)
  std::vector<uint8_t> m_seen;     // the stream has predicted through this object (its first Predict reads mctx)
  gmx_ctx* cb = nullptr;           // gmx_chainstep_attach_ctx: the context variables step on the device too
  bool cb_gone = false;            // ... and that bank has been destroyed
  bool broken = false;             // an attach failed while it captured the graphs anew: there is nothing to launch
  GmxCtxTarget c_tg[3] = {};       // its routes into the mixers', the Indirect models' and the Match models' words
  std::vector<uint8_t> c_pos;      // where in its byte the stream's next Predict falls (from the board at attach)
  hipEvent_t t_ev[2] = {};         // gmx_chainstep_timed_step: around the step's graph, on the group's stream
  bool timed = false, timed_ok = false;
  int S = 0, lstm_slot = -1, mixer_ctx_col = -1, ind_ctx_col = -1;
  // h_in: ONE pinned host block [control words | records], uploaded by the step's first kernel into d_in[parity];
  // h_bd: what a byte-opening step adds (PPM distributions, the bytes just completed, the LSTM's counts) -> d_bd;
  // h_out: pinned host memory the mixers' kernel stores p and the outputs into (d_out = the device's address of it)
  uint8_t *h_in = nullptr, *h_in_dev = nullptr, *d_in[2] = {nullptr, nullptr};
  uint8_t *h_bd = nullptr, *h_bd_dev = nullptr, *d_bd = nullptr;
  uint8_t *h_out = nullptr, *d_out = nullptr;
  size_t in_bytes = 0, bd_bytes = 0, out_bytes = 0;
  // host views
  uint8_t *bits = nullptr, *what = nullptr;     // the CALLER's: what each stream asks of the next step
  uint8_t* what_dev = nullptr;                  // what the kernels see (+ bit 2: the predict opens a byte)
  float* dec = nullptr;
  uint64_t *tl_learn = nullptr, *tl_pred = nullptr;
  float* pred = nullptr;
  uint32_t *mask = nullptr, *ctx = nullptr, *ictx = nullptr, *ibc = nullptr;
  float* ppm = nullptr;
  uint8_t* bytes = nullptr;
  uint64_t *nl_perceive = nullptr, *nl_forward = nullptr;
  float *p = nullptr, *outs = nullptr;
  // device-only
  uint32_t* idx_dev = nullptr;     // [S] identity (decay table row of stream s)
  uint32_t* ind_latch = nullptr;   // [S][64][4]
  float* adam_host = nullptr;      // pinned [S][2][4], read by the LSTM kernel where it lies
  float* adam_dev = nullptr;
  float* l_pred = nullptr;         // scratch the LSTM kernel's record outputs point at
  uint8_t* l_act = nullptr;
  uint32_t* l_ctx = nullptr;
  GmxStepUpload up = {};           // a stream's slices of h_in: control words first (n_ctl of them), then records
  int n_ctl = 0;
  bool bar = false;                // d_in / d_bd are fine-grained device memory the host stores into
  bool stock = false;              // the mixers' share of a step is one launch of gmx_stock_step_kernel ...
  uint32_t* seq = nullptr;         // ... which stamps the step's number (host view, in h_in) ...
  uint32_t* stamp = nullptr;       // ... into these S words of h_out
  uint32_t seq_no = 0;
  bool in_flight = false;          // between gmx_chainstep_launch and gmx_chainstep_wait
  size_t bd_ppm_off = 0;
  std::vector<uint8_t> committed;  // the stream's records are in the device copy of the coming step
  hipGraph_t graph[2][2] = {};        // [parity of the step][opens a byte]
  hipGraphExec_t exec[2][2] = {};
  // per stream
  std::vector<uint8_t> pending;    // a forward waits for its learn
  std::vector<uint8_t> nbits;      // bits of the current byte learned so far
  std::vector<uint8_t> acc;        // ... and their value
  uint64_t steps = 0;
  uint64_t bit_launches = 0;       // per-bit graphs launched so far (gmx_debug_chainstep_bit_launches)
  gmx_cs_decoder* dc = nullptr;    // gmx_chainstep_attach_decoder
};

static void cs_decoder_free(gmx_chainstep* cs);
static void cs_decoder_answered(gmx_chainstep* cs);
static hipError_t cs_coder_args(gmx_chainstep* cs, int par, int j, GmxCoderStepArgs* ca);

static size_t cs_round(size_t n) { return (n + 255) / 256 * 256; }

static void chainstep_match_gone(gmx_chainstep* cs) {
  if (cs->g) {
    (void)hipSetDevice(cs->g->device);
    if (cs->g->stream) (void)hipStreamSynchronize(cs->g->stream);  // (a step in flight still writes the bank)
  }
  cs->mb = nullptr;
  cs->mb_gone = true;
}

static void chainstep_ctx_gone(gmx_chainstep* cs) {
  if (cs->g) {
    (void)hipSetDevice(cs->g->device);
    if (cs->g->stream) (void)hipStreamSynchronize(cs->g->stream);  // (a step in flight still writes the bank)
  }
  cs->cb = nullptr;
  cs->cb_gone = true;
}

// What a gmx_ctx_* call on an attached bank waits for: the steps run on the group's stream.
static int chainstep_settle(gmx_chainstep* cs) {
  if (!cs->g || !cs->g->stream) return GMX_OK;
  HIPCHK(hipSetDevice(cs->g->device));
  if (hipStreamQuery(cs->g->stream) != hipSuccess) HIPCHK(hipStreamSynchronize(cs->g->stream));
  (void)hipGetLastError();
  return GMX_OK;
}

extern "C" void gmx_chainstep_destroy(gmx_chainstep* cs) {
  if (!cs) return;
  if (cs->cb) cs->cb->chainstep = nullptr;
  if (cs->mb) {
    auto& v = cs->mb->chainsteps;
    v.erase(std::remove(v.begin(), v.end(), cs), v.end());
  }
  if (cs->g) {
    (void)hipSetDevice(cs->g->device);
    if (cs->g->stream) (void)hipStreamSynchronize(cs->g->stream);
  }
  for (int p = 0; p < 2; ++p)
    for (int o = 0; o < 2; ++o) {
      if (cs->exec[p][o]) (void)hipGraphExecDestroy(cs->exec[p][o]);
      if (cs->graph[p][o]) (void)hipGraphDestroy(cs->graph[p][o]);
    }
  for (hipEvent_t ev : cs->t_ev)
    if (ev) (void)hipEventDestroy(ev);
  cs_decoder_free(cs);
  void* hv[] = {cs->h_in, cs->h_bd, cs->h_out, cs->adam_host};
  for (void* q : hv)
    if (q) (void)hipHostFree(q);
  void* dv[] = {cs->d_in[0], cs->d_in[1], cs->d_bd, cs->idx_dev, cs->ind_latch, cs->l_pred, cs->l_act, cs->l_ctx};
  for (void* q : dv)
    if (q) (void)hipFree(q);
  delete cs;
}

// The step as a stream of work on `st` (captured four times: parity of the step x whether it opens a byte).  br
// (nullable): the step is step br->j of a byte graph (gmx_coder.inc) -- the device writes the step's words and records
// itself, gmx_coder_step_kernel in place of the context bank's node, so nothing is fetched from the host, and p, the
// outputs and the stamps stay in device memory.
static hipError_t cs_record(gmx_chainstep* cs, hipStream_t st, bool opens, int par, const CsByteRoute* br = nullptr) {
  gmx_group* g = cs->g;
  const GmxTopoDev& t = g->topo;
  hipError_t e = hipSuccess;
  auto cur = [&](const void* host_ptr) { return cs->d_in[par] + ((const uint8_t*)host_ptr - cs->h_in); };
  auto old = [&](const void* host_ptr) { return cs->d_in[par ^ 1] + ((const uint8_t*)host_ptr - cs->h_in); };
  auto bd = [&](const void* host_ptr) { return cs->d_bd + ((const uint8_t*)host_ptr - cs->h_bd); };
  auto res = [&](const void* host_ptr) { return cs->d_out + ((const uint8_t*)host_ptr - cs->h_out); };
  // everything of this step, control words and records, into this parity's device copy: by the step's first kernel
  GmxStepUpload up = cs->up;
  up.src = cs->h_in_dev;
  up.dst = cs->d_in[par];
  if (cs->bar || br) up.n = 0;  // the host has put them there (a byte graph: the step's first kernel writes them)
  if (br) {
    GmxCoderStepArgs ca;
    e = cs_coder_args(cs, par, br->j, &ca);
    if (e != hipSuccess) return e;
    e = gmx_launch_coder_step(cs->cb->dev_d, &ca, st);
    if (e != hipSuccess) return e;
  } else if (cs->cb) {
    // the context bank's bit: behind the step's words and in front of every consumer of the records it writes.  Where
    // the device fetches the step's inputs the fetch is a node of its own in front of it (inside the models' kernel it
    // would overwrite what this node wrote)
    if (up.n > 0) {
      e = gmx_launch_step_upload(&up, cs->S, st);
      if (e != hipSuccess) return e;
      up.n = 0;
    }
    GmxCtxStepArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.banks = cs->cb->banks;
    ca.bits = (const uint8_t*)cur(cs->bits);
    ca.what = (const uint8_t*)cur(cs->what_dev);
    ca.bc = (cs->ib || cs->mb) ? (uint32_t*)cur(cs->ibc) : nullptr;
    ca.n_streams = cs->S;
    const void* const rec[3] = {cs->ctx, cs->ictx, cs->mctx};
    for (int k = 0; k < 3; ++k) {
      ca.tg[k] = cs->c_tg[k];
      ca.tg[k].ctx = cs->c_tg[k].n_cols > 0 ? (uint32_t*)cur(rec[k]) : nullptr;
    }
    e = gmx_launch_ctx_step(cs->cb->dev_d, &ca, st);
    if (e != hipSuccess) return e;
  }
  const uint8_t* const bits_d = (const uint8_t*)cur(cs->bits);
  const uint8_t* const what_d = (const uint8_t*)cur(cs->what_dev);
  float* const pred_d = (float*)cur(cs->pred);
  uint32_t* const mask_d = (uint32_t*)cur(cs->mask);
  uint32_t* const ctx_d = (uint32_t*)cur(cs->ctx);
  if (cs->l && opens) {
    gmx_lstm* l = cs->l;
    if (!cs->bar && !br) {  // (a byte graph begins with this copy: its first kernel reads the distributions)
      e = gmx_launch_copy16(cs->d_bd, cs->h_bd_dev, cs->bd_bytes / 16, st);
      if (e != hipSuccess) return e;
    }
    GmxLstmRunArgs la;
    memset(&la, 0, sizeof la);
    la.banks = l->banks;
    la.ppm = (const float*)bd(cs->ppm);
    la.bytes = (const uint8_t*)bd(cs->bytes);
    la.adam = cs->adam_dev;
    la.pred_out = cs->l_pred;
    la.act_out = cs->l_act;
    la.ctx_out = cs->l_ctx;
    la.rec_stride = 1;
    la.n_bytes = 1;
    la.max_bptt = 2;
    la.stream_base = 0;
    la.last_byte = -1;
    // Lstm::Perceive of the bytes just completed (LstmModel::Learn at a byte's last bit, lstm-model.cpp:51-60) ...
    la.n_list = (const uint64_t*)bd(cs->nl_perceive);
    la.learn = 1;
    la.phases = 4u;
    e = gmx_launch_lstm_kernel(l->dev_d, &la, cs->S, l->cus, st);
    if (e != hipSuccess) return e;
    // ... and Lstm::SetInput + Lstm::Predict of the bytes that open (lstm-model.cpp:19-33)
    la.n_list = (const uint64_t*)bd(cs->nl_forward);
    la.learn = 0;
    la.phases = 1u;
    e = gmx_launch_lstm_kernel(l->dev_d, &la, cs->S, l->cus, st);
    if (e != hipSuccess) return e;
  }
  GmxLstmBitArgs ba;
  memset(&ba, 0, sizeof ba);
  ba.ind_ctx_col = -1;
  if (cs->l) {
    ba.banks = cs->l->banks;
    ba.bits = bits_d;
    ba.what = what_d;
    ba.mx_pred = pred_d;
    ba.mx_mask = mask_d;
    ba.mx_ctx = ctx_d;
    ba.mx_n_pad = t.n_pad;
    ba.mx_mask_words = t.mask_words;
    ba.mx_m = t.m;
    ba.slot = cs->lstm_slot;
    ba.mixer_ctx_col = cs->mixer_ctx_col;
    if (cs->ib && cs->ind_ctx_col >= 0) {
      ba.ind_ctx = (uint32_t*)cur(cs->ictx);
      ba.ind_k = cs->ib->dev.k;
      ba.ind_ctx_col = cs->ind_ctx_col;
    }
  }
  GmxMatchStepArgs ma;
  memset(&ma, 0, sizeof ma);
  // the Match lanes ride in the Indirect models' launch where its wave has the eight lanes to spare
  const bool m_fused = cs->mb && cs->ib && cs->ib->dev.k <= 56 && t.mask_words <= 8;
  if (cs->mb) {
    ma.banks = cs->mb->banks;
    ma.hist = cs->mb->hist;
    ma.ctx = (const uint32_t*)cur(cs->mctx);
    ma.bc = (const uint32_t*)cur(cs->ibc);
    ma.bits = bits_d;
    ma.what = what_d;
    ma.mx_pred = pred_d;
    ma.mx_mask = mask_d;
    ma.mx_ctx = ctx_d;
    ma.mx_n_pad = t.n_pad;
    ma.mx_mask_words = t.mask_words;
    ma.mx_m = t.m;
    ma.n_ctx_cols = cs->n_mcols;
    for (int c = 0; c < cs->n_mcols; ++c) ma.ctx_cols[c] = cs->mcols[c];
    ma.n_streams = cs->S;
  }
  if (cs->ib && cs->l) {
    // the LSTM's bit prediction and the Indirect models in one launch, the step's inputs fetched by it
    GmxIndStepArgs ia;
    memset(&ia, 0, sizeof ia);
    ia.banks = cs->ib->banks;
    ia.ctx = (const uint32_t*)cur(cs->ictx);
    ia.bc = (const uint32_t*)cur(cs->ibc);
    ia.bits = bits_d;
    ia.what = what_d;
    ia.latch = cs->ind_latch;
    ia.mx_pred = pred_d;
    ia.mx_mask = mask_d;
    ia.mx_n_pad = t.n_pad;
    ia.mx_mask_words = t.mask_words;
    ia.up = up;
    e = m_fused ? gmx_launch_models_step_match(cs->ib->dev_d, cs->ib->dev.k, &ia, cs->l->dev_d, &ba, cs->mb->dev_d, &ma,
                                               cs->S, st)
                : gmx_launch_models_step(cs->ib->dev_d, &ia, cs->l->dev_d, &ba, cs->S, st);
    if (e != hipSuccess) return e;
  } else {
    if (up.n > 0) {
      e = gmx_launch_step_upload(&up, cs->S, st);
      if (e != hipSuccess) return e;
    }
    if (cs->ib) {
      GmxIndStepArgs ia;
      memset(&ia, 0, sizeof ia);
      ia.banks = cs->ib->banks;
      ia.ctx = (const uint32_t*)cur(cs->ictx);
      ia.bc = (const uint32_t*)cur(cs->ibc);
      ia.bits = bits_d;
      ia.what = what_d;
      ia.latch = cs->ind_latch;
      ia.mx_pred = pred_d;
      ia.mx_mask = mask_d;
      ia.mx_n_pad = t.n_pad;
      ia.mx_mask_words = t.mask_words;
      e = m_fused ? gmx_launch_models_step_match(cs->ib->dev_d, cs->ib->dev.k, &ia, nullptr, nullptr, cs->mb->dev_d, &ma,
                                                 cs->S, st)
                  : gmx_launch_indirect_step(cs->ib->dev_d, &ia, cs->S, st);
      if (e != hipSuccess) return e;
    } else if (cs->l) {
      e = gmx_launch_lstm_bitstep(cs->l->dev_d, &ba, cs->S, st);
      if (e != hipSuccess) return e;
    }
  }
  if (cs->mb && !m_fused) {  // one node of their own in front of the mixers' (gmx_match_step_kernel)
    e = gmx_launch_match_step(cs->mb->dev_d, &ma, st);
    if (e != hipSuccess) return e;
  }
  if (cs->stock) {
    // Mixer::Learn x M of the streams that ask, on the records of their forward -- the step before's, in the other
    // copy -- and Mixer::Predict x M on this step's: one launch, the rows resident in between
    GmxStkStepArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.banks = g->banks;
    sa.what = what_d;
    sa.bits = bits_d;
    sa.dec = (const float*)cur(cs->dec);
    sa.pred_old = (const float*)old(cs->pred);
    sa.mask_old = (const uint32_t*)old(cs->mask);
    sa.ctx_old = (const uint32_t*)old(cs->ctx);
    sa.pred_new = pred_d;
    sa.mask_new = mask_d;
    sa.ctx_new = ctx_d;
    sa.p_out = br ? br->p : (float*)res(cs->p);
    sa.out_all = br ? br->outs : (float*)res(cs->outs);
    sa.latch = g->latch_out;
    sa.seq = (const uint32_t*)cur(cs->seq);
    sa.stamp = br ? br->stamp : (uint32_t*)res(cs->stamp);
    sa.n_streams = g->S;
    sa.exact = g->stock_exact ? 1 : 0;
    return gmx_launch_stock_step(g->topo_dev, &sa, GMX_STK_LDS_BYTES(g->topo.lds_misc), st);
  }
  // any other topology: a learn-only and a forward launch of the group's batched kernel (T = 1; outputs latched)
  GmxRunArgs a;
  memset(&a, 0, sizeof a);
  a.banks = g->banks;
  a.bits = bits_d;
  a.decay = (const float*)cur(cs->dec);
  a.decay_idx = cs->idx_dev;
  a.p_out = br ? br->p : (float*)res(cs->p);
  a.out_all = br ? br->outs : (float*)res(cs->outs);
  a.latch_out = g->latch_out;
  a.rec_stride = 1;
  a.T = 1;
  a.n_streams = g->S;
  a.pred = (const float*)old(cs->pred);
  a.mask = (const uint32_t*)old(cs->mask);
  a.ctx = (const uint32_t*)old(cs->ctx);
  a.mode = GMX_MODE_LEARN | (g->stock_exact ? GMX_MODE_EXACT : 0u);
  a.T_list = (const uint64_t*)cur(cs->tl_learn);
  e = lockstep_launch_kernel(g, a, st);
  if (e != hipSuccess) return e;
  a.pred = pred_d;
  a.mask = mask_d;
  a.ctx = ctx_d;
  a.mode = GMX_MODE_PREDICT | GMX_MODE_LATCH | (g->stock_exact ? GMX_MODE_EXACT : 0u);
  a.T_list = (const uint64_t*)cur(cs->tl_pred);
  return lockstep_launch_kernel(g, a, st);
}

// The four graphs (parity x opens a byte; two without an LSTM), dropping the ones there are.
static hipError_t cs_capture(gmx_chainstep* cs) {
  hipStream_t st = cs->g->stream;
  for (int par = 0; par < 2; ++par)
    for (int opens = 0; opens < 2; ++opens) {
      if (cs->exec[par][opens]) (void)hipGraphExecDestroy(cs->exec[par][opens]);
      if (cs->graph[par][opens]) (void)hipGraphDestroy(cs->graph[par][opens]);
      cs->exec[par][opens] = nullptr;
      cs->graph[par][opens] = nullptr;
    }
  // once outside a capture, with every stream sitting out (all counts and flags are zero): whatever a launcher
  // sets up on its first call (dynamic LDS limits) is set up
  hipError_t e = cs_record(cs, st, true, 0);
  if (e != hipSuccess) return e;
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  for (int par = 0; par < 2; ++par)
    for (int opens = 0; opens < (cs->l ? 2 : 1); ++opens) {
      e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
      if (e != hipSuccess) return e;
      e = cs_record(cs, st, opens != 0, par);
      const hipError_t e2 = hipStreamEndCapture(st, &cs->graph[par][opens]);
      if (e != hipSuccess) return e;
      if (e2 != hipSuccess) return e2;
      e = hipGraphInstantiate(&cs->exec[par][opens], cs->graph[par][opens], nullptr, nullptr, 0);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

extern "C" int gmx_chainstep_create(gmx_chainstep** out, gmx_group* g, gmx_indirect* ib, gmx_lstm* l, int lstm_slot,
                                    int mixer_ctx_col, int ind_ctx_col) {
  if (!out || !g) return GMX_ERR_INVALID;
  *out = nullptr;
  const GmxTopoDev& t = g->topo;
  if (ib && (ib->S != g->S || ib->device != g->device || t.mask_words > 8)) return GMX_ERR_INVALID;
  if (l && (l->S != g->S || l->device != g->device || lstm_slot < 0 || lstm_slot >= t.n || mixer_ctx_col >= t.m))
    return GMX_ERR_INVALID;
  if (l && l->any) return GMX_ERR_INVALID;  // the chain's launches are the stock kernel's, on the stock layout
  if (l && ib && ind_ctx_col >= ib->dev.k) return GMX_ERR_INVALID;
  if (ib)
    for (int i = 0; i < ib->dev.k; ++i)
      if (ib->dev.m[i].slot_a < 0 || ib->dev.m[i].slot_a >= t.n || ib->dev.m[i].slot_b < 0 || ib->dev.m[i].slot_b >= t.n)
        return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(g->device));
  int rc = sessions_close(g, false);
  if (rc) return rc;
  if (ib) {
    rc = ind_sessions_close(ib);
    if (rc) return rc;
    ind_sessions_drop_forward(ib, -1);
    HIPCHK(hipStreamSynchronize(ib->stream));
  }
  if (l) {
    rc = lstm_sessions_close(l);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(l->stream));
  }
  HIPCHK(hipStreamSynchronize(g->stream));
  gmx_chainstep* cs = new (std::nothrow) gmx_chainstep();
  if (!cs) return GMX_ERR_NOMEM;
  cs->g = g;
  cs->ib = ib;
  cs->l = l;
  cs->S = g->S;
  cs->lstm_slot = lstm_slot;
  cs->mixer_ctx_col = l ? mixer_ctx_col : -1;
  cs->ind_ctx_col = (l && ib) ? ind_ctx_col : -1;
  const size_t S = (size_t)g->S, K = ib ? (size_t)ib->dev.k : 0;
#define CCHK(call)                                 \
  do {                                             \
    hipError_t e_ = (call);                        \
    if (e_ != hipSuccess) {                        \
      int r_ = hip_fail(e_, #call);                \
      gmx_chainstep_destroy(cs);                   \
      return e_ == hipErrorOutOfMemory ? GMX_ERR_NOMEM : r_; \
    }                                              \
  } while (0)
  // layouts: every array on a 256-byte boundary of its block
  size_t o = 0;
  auto take = [&o](size_t n) {
    const size_t at = o;
    o += cs_round(n);
    return at;
  };
  const size_t c_bits = take(S), c_what = take(S), c_whatd = take(S), c_dec = take(S * 4), c_tll = take(S * 8),
               c_tlp = take(S * 8), c_seq = take(S * 4);
  const size_t r_pred = take(S * t.n_pad * 4), r_mask = take(S * t.mask_words * 4), r_ctx = take(S * t.m * 4),
               r_ictx = take((K ? S * K : 1) * 4), r_ibc = take(S * 4);
  // (room for an attached Match bank's context words: the block and the host views never move)
  const size_t r_mctx = take(S * GMX_MATCH_MAX_MODELS * 4);
  cs->in_bytes = o;
  {
    const size_t offs[] = {c_bits, c_whatd, c_dec, c_seq, c_tll, c_tlp, r_pred, r_mask, r_ctx, r_ictx, r_ibc};
    const size_t bps[] = {1, 1, 4, 4, 8, 8, (size_t)t.n_pad * 4, (size_t)t.mask_words * 4, (size_t)t.m * 4, K * 4, 4};
    for (size_t i = 0; i < sizeof offs / sizeof offs[0]; ++i) {
      if (!bps[i]) continue;
      cs->up.off[cs->up.n] = (uint32_t)offs[i];
      cs->up.bps[cs->up.n] = (uint32_t)bps[i];
      cs->up.n += 1;
      if (i < 6) cs->n_ctl = cs->up.n;
    }
  }
  cs->stock = group_is_stock(g) && !g->force_general;
  o = 0;
  const size_t b_ppm = take(S * GMX_L_NI * 4), b_bytes = take(S), b_nlp = take(S * 8), b_nlf = take(S * 8);
  cs->bd_bytes = o;
  o = 0;
  const size_t o_p = take(S * 4), o_outs = take(S * t.m * 4), o_stamp = take(S * 4);
  cs->out_bytes = o;
  const unsigned hflags = hipHostMallocMapped | hipHostMallocCoherent;
  CCHK(hipHostMalloc((void**)&cs->h_in, cs->in_bytes, hflags));
  CCHK(hipHostMalloc((void**)&cs->h_bd, cs->bd_bytes, hflags));
  CCHK(hipHostMalloc((void**)&cs->h_out, cs->out_bytes, hflags));
  CCHK(hipHostGetDevicePointer((void**)&cs->h_in_dev, cs->h_in, 0));
  CCHK(hipHostGetDevicePointer((void**)&cs->h_bd_dev, cs->h_bd, 0));
  CCHK(hipHostGetDevicePointer((void**)&cs->d_out, cs->h_out, 0));
  {
    // device memory the host can store into, if there is such a thing here
    int large_bar = 0;
    if (!getenv("GMX_CS_NO_BAR") && g->mailbox_on_device &&
        hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, g->device) == hipSuccess && large_bar) {
      void* q[3] = {nullptr, nullptr, nullptr};
      const size_t n[3] = {cs->in_bytes, cs->in_bytes, cs->bd_bytes};
      bool ok = true;
      for (int i = 0; i < 3 && ok; ++i) ok = hipExtMallocWithFlags(&q[i], n[i], hipDeviceMallocFinegrained) == hipSuccess;
      if (ok) {
        cs->d_in[0] = (uint8_t*)q[0];
        cs->d_in[1] = (uint8_t*)q[1];
        cs->d_bd = (uint8_t*)q[2];
        cs->bar = true;
      } else {
        for (void* x : q)
          if (x) (void)hipFree(x);
      }
      (void)hipGetLastError();
    }
  }
  if (!cs->bar) {
    CCHK(hipMalloc((void**)&cs->d_in[0], cs->in_bytes));
    CCHK(hipMalloc((void**)&cs->d_in[1], cs->in_bytes));
    CCHK(hipMalloc((void**)&cs->d_bd, cs->bd_bytes));
  }
  memset(cs->h_in, 0, cs->in_bytes);
  memset(cs->h_bd, 0, cs->bd_bytes);
  memset(cs->h_out, 0, cs->out_bytes);
  CCHK(hipMemset(cs->d_in[0], 0, cs->in_bytes));
  CCHK(hipMemset(cs->d_in[1], 0, cs->in_bytes));
  CCHK(hipMemset(cs->d_bd, 0, cs->bd_bytes));
  cs->bits = cs->h_in + c_bits;
  cs->what = cs->h_in + c_what;
  cs->what_dev = cs->h_in + c_whatd;
  cs->dec = (float*)(cs->h_in + c_dec);
  cs->tl_learn = (uint64_t*)(cs->h_in + c_tll);
  cs->tl_pred = (uint64_t*)(cs->h_in + c_tlp);
  cs->seq = (uint32_t*)(cs->h_in + c_seq);
  cs->pred = (float*)(cs->h_in + r_pred);
  cs->mask = (uint32_t*)(cs->h_in + r_mask);
  cs->ctx = (uint32_t*)(cs->h_in + r_ctx);
  cs->ictx = (uint32_t*)(cs->h_in + r_ictx);
  cs->ibc = (uint32_t*)(cs->h_in + r_ibc);
  cs->mctx = (uint32_t*)(cs->h_in + r_mctx);
  cs->ppm = (float*)(cs->h_bd + b_ppm);
  cs->bytes = cs->h_bd + b_bytes;
  cs->nl_perceive = (uint64_t*)(cs->h_bd + b_nlp);
  cs->nl_forward = (uint64_t*)(cs->h_bd + b_nlf);
  cs->p = (float*)(cs->h_out + o_p);
  cs->outs = (float*)(cs->h_out + o_outs);
  cs->stamp = (uint32_t*)(cs->h_out + o_stamp);
  cs->bd_ppm_off = b_ppm;
  cs->committed.assign(S, 0);
  CCHK(hipMalloc((void**)&cs->idx_dev, S * sizeof(uint32_t)));
  {
    std::vector<uint32_t> idn(S);
    for (size_t s = 0; s < S; ++s) idn[s] = (uint32_t)s;
    CCHK(hipMemcpy(cs->idx_dev, idn.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  CCHK(hipMalloc((void**)&cs->ind_latch, S * 64 * 4 * sizeof(uint32_t)));
  CCHK(hipMemset(cs->ind_latch, 0, S * 64 * 4 * sizeof(uint32_t)));
  CCHK(hipHostMalloc((void**)&cs->adam_host, S * 2 * 4 * sizeof(float), hipHostMallocDefault));
  memset(cs->adam_host, 0, S * 2 * 4 * sizeof(float));
  CCHK(hipHostGetDevicePointer((void**)&cs->adam_dev, cs->adam_host, 0));
  CCHK(hipMalloc((void**)&cs->l_pred, S * 8 * sizeof(float)));
  CCHK(hipMalloc((void**)&cs->l_act, S * 8));
  CCHK(hipMalloc((void**)&cs->l_ctx, S * sizeof(uint32_t)));
  cs->pending.assign(S, 0);
  cs->nbits.assign(S, 0);
  cs->acc.assign(S, 0);
  CCHK(cs_capture(cs));
#undef CCHK
  *out = cs;
  return GMX_OK;
}

extern "C" int gmx_chainstep_n_streams(const gmx_chainstep* cs) { return cs ? cs->S : GMX_ERR_INVALID; }
extern "C" float* gmx_chainstep_predictions(gmx_chainstep* cs) { return cs ? cs->pred : nullptr; }
extern "C" uint32_t* gmx_chainstep_active_mask(gmx_chainstep* cs) { return cs ? cs->mask : nullptr; }
extern "C" uint32_t* gmx_chainstep_contexts(gmx_chainstep* cs) { return cs ? cs->ctx : nullptr; }
extern "C" uint32_t* gmx_chainstep_ind_contexts(gmx_chainstep* cs) { return (cs && cs->ib) ? cs->ictx : nullptr; }
extern "C" uint32_t* gmx_chainstep_bit_contexts(gmx_chainstep* cs) { return (cs && (cs->ib || cs->mb)) ? cs->ibc : nullptr; }
extern "C" uint32_t* gmx_chainstep_match_contexts(gmx_chainstep* cs) { return (cs && cs->mb) ? cs->mctx : nullptr; }

// The Match models of every stream step on the device from now on (gmx_match_step.h): their slots of the mixers'
// record, their mask bits and longest_match in the listed gate-context columns are the device's; the host supplies
// match_contexts[s][K] on byte-opening predicts and on a stream's first predict, and bit_contexts[s] on every one.
extern "C" int gmx_chainstep_attach_match(gmx_chainstep* cs, gmx_match* mb, const int32_t* ctx_columns,
                                          int n_ctx_columns) {
  if (!cs || !cs->g || !mb) return GMX_ERR_INVALID;
  if (cs->mb || cs->cb || cs->cb_gone || cs->steps != 0 || cs->in_flight)
    return GMX_ERR_STATE;  // once, before the first step -- and before a context bank, whose routes name its columns
  if (mb->host) return GMX_ERR_STATE;  // (its streams ride in per-bit session waves: gmx_indirect_attach_match)
  gmx_group* g = cs->g;
  const GmxTopoDev& t = g->topo;
  if (mb->S != cs->S || mb->device != g->device || t.mask_words > GMX_MATCH_MAX_MASK_WORDS) return GMX_ERR_INVALID;
  if (n_ctx_columns < 0 || n_ctx_columns > GMX_MATCH_MAX_CTX_COLS || (n_ctx_columns > 0 && !ctx_columns))
    return GMX_ERR_INVALID;
  for (int c = 0; c < n_ctx_columns; ++c)
    if (ctx_columns[c] < 0 || ctx_columns[c] >= t.m) return GMX_ERR_INVALID;
  for (int i = 0; i < mb->dev.k; ++i)
    if (mb->dev.m[i].slot < 0 || mb->dev.m[i].slot >= t.n) return GMX_ERR_INVALID;
  if (cs->up.n >= GMX_STEP_UP_MAX) return GMX_ERR_INVALID;
  HIPCHK(hipSetDevice(g->device));
  HIPCHK(hipStreamSynchronize(mb->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  cs->mb = mb;
  mb->chainsteps.push_back(cs);
  cs->n_mcols = n_ctx_columns;
  for (int c = 0; c < n_ctx_columns; ++c) cs->mcols[c] = ctx_columns[c];
  cs->m_bc.assign(cs->S, 0);
  cs->m_seen.assign(cs->S, 0);
  // the context words join the records of a step: gmx_chainstep_commit and the upload slices move them
  cs->up.off[cs->up.n] = (uint32_t)((const uint8_t*)cs->mctx - cs->h_in);
  cs->up.bps[cs->up.n] = (uint32_t)mb->dev.k * 4u;
  cs->up.n += 1;
  const hipError_t e = cs_capture(cs);
  if (e != hipSuccess) {  // (the object cannot step any more: no graph of it is whole)
    cs->mb = nullptr;
    mb->chainsteps.pop_back();
    cs->up.n -= 1;
    return e == hipErrorOutOfMemory ? GMX_ERR_NOMEM : hip_fail(e, "gmx_chainstep_attach_match: capture");
  }
  return GMX_OK;
}

// Where in its byte every stream's next Predict falls: recent_bits, new_bit and first_prediction head the board, read
// for all streams in one transfer.  At attach, and again before a step when a gmx_ctx_* call between the steps may have
// moved a stream (gmx_ctx_run, _blackboard_set, _copy, _reset).  A stream whose Predict waits for its Learn keeps its
// count: those calls refuse it, and its new_bit means nothing.
static int cs_read_positions(gmx_chainstep* cs, gmx_ctx* cb) {
  gmx_group* g = cs->g;
  std::vector<uint32_t> head((size_t)cs->S * 3);
  uint32_t* head_d = nullptr;
  HIPCHK(hipMalloc((void**)&head_d, head.size() * 4));
  hipError_t eh = gmx_launch_ctx_heads(cb->dev_d, cb->banks, cs->S, head_d, g->stream);
  if (eh == hipSuccess) eh = hipMemcpyAsync(head.data(), head_d, head.size() * 4, hipMemcpyDeviceToHost, g->stream);
  if (eh == hipSuccess) eh = hipStreamSynchronize(g->stream);
  (void)hipFree(head_d);
  HIPCHK(eh);
  for (int s = 0; s < cs->S; ++s) {
    if (cs->pending[s]) continue;
    const uint32_t rb = head[3 * s], nb = head[3 * s + 1], fp = head[3 * s + 2];
    const uint32_t p = fp ? rb : 2u * rb + (nb & 1u);
    int n = 0;
    for (uint32_t q = p; q > 1u; q >>= 1) ++n;  // the bits of the open byte the next Predict has in front of it
    cs->c_pos[s] = (uint8_t)(n & 7);
  }
  return GMX_OK;
}

// The context variables of every stream step on the device from now on (gmx_ctx_step.h): the routed columns of
// contexts / ind_contexts / match_contexts and bit_contexts are the bank's, whatever the staging arrays hold there.
extern "C" int gmx_chainstep_attach_ctx(gmx_chainstep* cs, gmx_ctx* cb, const gmx_ctx_step_routes* routes) {
  if (!cs || !cs->g || !cb || !routes) return GMX_ERR_INVALID;
  if (cs->cb || cs->cb_gone || cs->steps != 0 || cs->in_flight) return GMX_ERR_STATE;  // once, before the first step
  gmx_group* g = cs->g;
  const GmxTopoDev& t = g->topo;
  if (cb->S != cs->S || cb->device != g->device) return GMX_ERR_INVALID;
  const int K = cs->ib ? cs->ib->dev.k : 0, KM = cs->mb ? cs->mb->dev.k : 0;
  if (ctx_route_ok(cb, routes->mixer_route, routes->n_mixer_route, t.m)) return GMX_ERR_INVALID;
  const bool has_ind = routes->ind_route || routes->n_ind_route, has_match = routes->match_route || routes->n_match_route;
  if (has_ind != (K > 0) || has_match != (KM > 0)) return GMX_ERR_INVALID;  // NULL / 0 iff there is no such bank
  if (has_ind && ctx_route_ok(cb, routes->ind_route, routes->n_ind_route, K)) return GMX_ERR_INVALID;
  if (has_match && ctx_route_ok(cb, routes->match_route, routes->n_match_route, KM)) return GMX_ERR_INVALID;
  // a column has one writer on the device
  auto device_owned_mixer = [&](int c) {
    if (c == cs->mixer_ctx_col) return true;
    for (int i = 0; i < cs->n_mcols; ++i)
      if (cs->mcols[i] == c) return true;
    return false;
  };
  for (int c = 0; c < t.m; ++c)
    if (routes->mixer_route[c] >= 0 && device_owned_mixer(c)) return GMX_ERR_INVALID;
  if (has_ind && cs->ind_ctx_col >= 0 && routes->ind_route[cs->ind_ctx_col] >= 0) return GMX_ERR_INVALID;
  if (cb->chainstep) return GMX_ERR_STATE;  // one lock-step object per bank
  if (cb->host) return GMX_ERR_STATE;       // (its streams ride in per-bit session waves: gmx_indirect_attach_ctx)
  HIPCHK(hipSetDevice(g->device));
  for (int s = 0; s < cb->S && cb->n_noted > 0; ++s) {  // a learn gmx_ctx_learn noted: the boards are read below
    const int rcn = ctx_flush_noted(cb, s);
    if (rcn) return rcn;
  }
  HIPCHK(hipStreamSynchronize(cb->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  const GmxStepUpload up_before = cs->up;
  cs->c_pos.assign(cs->S, 0);
  {
    const int rcp = cs_read_positions(cs, cb);
    if (rcp) return rcp;
  }
  cb->moved = false;
  const int32_t* const rt[3] = {routes->mixer_route, has_ind ? routes->ind_route : nullptr,
                                has_match ? routes->match_route : nullptr};
  const int nrt[3] = {t.m, K, KM};
  for (int k = 0; k < 3; ++k) {
    memset(&cs->c_tg[k], 0, sizeof cs->c_tg[k]);
    if (!rt[k]) continue;
    cs->c_tg[k].n_cols = nrt[k];
    cs->c_tg[k].stride = 1;
    memcpy(cs->c_tg[k].route, rt[k], 4 * (size_t)nrt[k]);
  }
  // don't move what nobody reads: bit_contexts, and a record array the caller owns no column of, leave the slices
  {
    bool own_mixer = false, own_ind = false, own_match = false;
    for (int c = 0; c < t.m; ++c) own_mixer = own_mixer || (rt[0][c] < 0 && !device_owned_mixer(c));
    for (int c = 0; c < K; ++c) own_ind = own_ind || (rt[1][c] < 0 && c != cs->ind_ctx_col);
    for (int c = 0; c < KM; ++c) own_match = own_match || rt[2][c] < 0;
    const uint32_t o_ctx = (uint32_t)((const uint8_t*)cs->ctx - cs->h_in), o_ictx = (uint32_t)((const uint8_t*)cs->ictx - cs->h_in),
                   o_ibc = (uint32_t)((const uint8_t*)cs->ibc - cs->h_in), o_mctx = (uint32_t)((const uint8_t*)cs->mctx - cs->h_in);
    GmxStepUpload u = cs->up;
    u.n = 0;
    for (int e = 0; e < cs->up.n; ++e) {
      const uint32_t o = cs->up.off[e];
      if (e >= cs->n_ctl && (o == o_ibc || (o == o_ctx && !own_mixer) || (o == o_ictx && !own_ind) || (o == o_mctx && !own_match)))
        continue;
      u.off[u.n] = o;
      u.bps[u.n] = cs->up.bps[e];
      u.n += 1;
    }
    cs->up = u;
  }
  cs->cb = cb;
  cb->chainstep = cs;
  const hipError_t e = cs_capture(cs);
  if (e != hipSuccess) {  // the object cannot step any more: no graph of it is whole, and its steps say so
    cs->cb = nullptr;
    cb->chainstep = nullptr;
    cs->up = up_before;
    for (GmxCtxTarget& tg : cs->c_tg) memset(&tg, 0, sizeof tg);
    cs->c_pos.clear();
    cs->broken = true;
    return e == hipErrorOutOfMemory ? GMX_ERR_NOMEM : hip_fail(e, "gmx_chainstep_attach_ctx: capture");
  }
  return GMX_OK;
}
extern "C" uint64_t gmx_chainstep_commit_bytes(const gmx_chainstep* cs) {
  uint64_t n = 0;
  if (cs)
    for (int e = cs->n_ctl; e < cs->up.n; ++e) n += cs->up.bps[e];
  return n;
}
extern "C" float* gmx_chainstep_ppm(gmx_chainstep* cs) { return (cs && cs->l) ? cs->ppm : nullptr; }
extern "C" uint8_t* gmx_chainstep_bits(gmx_chainstep* cs) { return cs ? cs->bits : nullptr; }
extern "C" uint8_t* gmx_chainstep_what(gmx_chainstep* cs) { return cs ? cs->what : nullptr; }
extern "C" const float* gmx_chainstep_p(gmx_chainstep* cs) { return cs ? cs->p : nullptr; }
extern "C" const float* gmx_chainstep_outputs(gmx_chainstep* cs) { return cs ? cs->outs : nullptr; }

// The records of stream s for the coming step: from the staging arrays into the device copy that step reads (and the
// PPM distribution of a stream whose Predict opens a byte).  Posted writes; nothing here reads device memory.
static void cs_commit_records(gmx_chainstep* cs, int s) {
  uint8_t* const dst = cs->d_in[cs->steps & 1];
  for (int e = cs->n_ctl; e < cs->up.n; ++e) {
    const size_t at = cs->up.off[e] + (size_t)s * cs->up.bps[e];
    memcpy(dst + at, cs->h_in + at, cs->up.bps[e]);
  }
  if (cs->l) {
    const uint8_t w = cs->what[s];
    if ((w & GMX_STEP_PREDICT) && ((cs->nbits[s] + ((w & GMX_STEP_LEARN) ? 1 : 0)) & 7) == 0) {
      const size_t at = cs->bd_ppm_off + (size_t)s * GMX_L_NI * 4;
      memcpy(cs->d_bd + at, cs->h_bd + at, GMX_L_NI * 4);
    }
  }
}

static std::atomic<uint64_t> g_cs_commit_ns{0}, g_cs_commits{0};  // (GMX_STEP_TRACE)
static bool cs_trace_on();
static double cs_now();

extern "C" int gmx_chainstep_commit(gmx_chainstep* cs, int s) {
  if (!cs || s < 0 || s >= cs->S) return GMX_ERR_INVALID;
  if (cs->in_flight) return GMX_ERR_STATE;  // (the running step's learn reads the copy this would write)
  if (!cs->bar) return GMX_OK;  // (the step's first kernel fetches them)
  const double t0 = cs_trace_on() ? cs_now() : 0.0;
  cs_commit_records(cs, s);
  mb_store_fence();
  cs->committed[s] = 1;
  if (cs_trace_on()) {
    g_cs_commit_ns.fetch_add((uint64_t)((cs_now() - t0) * 1e9), std::memory_order_relaxed);
    g_cs_commits.fetch_add(1, std::memory_order_relaxed);
  }
  return GMX_OK;
}

// The step in two halves, for a caller that has something else to do meanwhile (gmx::LockstepRunner: the files in two
// pools, the host's work on one beside the device's step of the other): launch returns when the step is queued, wait
// when its answers are in p / outputs.  Between the two nothing of this object may be written or committed.
static struct {
  double launch_s = 0, wait_s = 0;
  uint64_t n = 0;
} g_cs_trace;
static bool cs_trace_on() {
  static const bool on = getenv("GMX_STEP_TRACE") != nullptr;  // where a step's host time goes (stderr, every 4096 steps)
  return on;
}
static double cs_now() {
  timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

extern "C" int gmx_chainstep_launch(gmx_chainstep* cs) {
  if (!cs || !cs->g) return GMX_ERR_INVALID;
  if (cs->in_flight || cs->mb_gone || cs->cb_gone || cs->broken) return GMX_ERR_STATE;
  gmx_group* g = cs->g;
  const int S = cs->S;
  bool any = false, opens = false;
  for (int s = 0; s < S; ++s) {
    const uint8_t w = cs->what[s];
    if (w & ~(uint8_t)(GMX_STEP_LEARN | GMX_STEP_PREDICT)) return GMX_ERR_INVALID;
    if ((w & GMX_STEP_LEARN) && (!cs->pending[s] || cs->bits[s] > 1)) return cs->pending[s] ? GMX_ERR_INVALID : GMX_ERR_STATE;
    if ((w & GMX_STEP_PREDICT) && cs->pending[s] && !(w & GMX_STEP_LEARN)) return GMX_ERR_STATE;  // (Predict twice: not a decoder)
    any = any || w != 0;
  }
  if (!any) return GMX_OK;  // (nothing queued: gmx_chainstep_wait returns at once)
  for (int s = 0; s < S; ++s)  // (its record is in the device copy the NEXT step learns from, and only that one)
    if (cs->pending[s] && !(cs->what[s] & GMX_STEP_LEARN)) return GMX_ERR_STATE;
  HIPCHK(hipSetDevice(g->device));
  if (cs->mb) {
    // a history grows by one byte per stream whose Learn completes a byte: the rule of gmx_match_run -- when a bound
    // could pass the capacity the true sizes are fetched, and if it still could nothing is queued
    std::vector<uint64_t> add(S, 0);
    for (int s = 0; s < S; ++s) add[s] = ((cs->what[s] & GMX_STEP_LEARN) && cs->m_bc[s] >= 127u) ? 1 : 0;
    int rc = match_reserve(cs->mb, 0, S, add.data());
    if (rc) return rc;
    if (hipStreamQuery(cs->mb->stream) != hipSuccess) HIPCHK(hipStreamSynchronize(cs->mb->stream));
    (void)hipGetLastError();
  }
  if (cs->cb) {  // whatever gmx_ctx_* calls queued on the bank's own stream between the steps
    if (hipStreamQuery(cs->cb->stream) != hipSuccess) HIPCHK(hipStreamSynchronize(cs->cb->stream));
    (void)hipGetLastError();
    if (cs->cb->moved) {  // ... and where they left the streams in their bytes
      const int rcp = cs_read_positions(cs, cs->cb);
      if (rcp) return rcp;
      cs->cb->moved = false;
    }
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
  if (cs->bar)  // whatever gmx_chainstep_commit has not brought over yet (before the byte counts below move on)
    for (int s = 0; s < S; ++s) {
      if (!cs->committed[s] && cs->what[s]) cs_commit_records(cs, s);
      cs->committed[s] = 0;
    }
  uint64_t at = ~0ull;
  float dv = 0.0f;
  for (int s = 0; s < S; ++s) {
    const uint8_t w = cs->what[s];
    uint8_t wd = w;
    cs->tl_learn[s] = (w & GMX_STEP_LEARN) ? 1 : 0;
    cs->tl_pred[s] = (w & GMX_STEP_PREDICT) ? 1 : 0;
    cs->nl_perceive[s] = 0;
    cs->nl_forward[s] = 0;
    if (w & GMX_STEP_LEARN) {
      if (g->steps[s] != at) {  // float(0.9 / pow(1e-7 * steps_ + 0.8, 0.8)), mixer.cpp:111: one libm call per distinct count
        at = g->steps[s];
        dv = decay_base(at);
      }
      cs->dec[s] = dv;
      cs->acc[s] = (uint8_t)((cs->acc[s] << 1) | cs->bits[s]);
      if (++cs->nbits[s] == 8) {  // the byte is complete: LstmModel::Learn perceives it (lstm-model.cpp:51-60)
        cs->bytes[s] = cs->acc[s];
        cs->nl_perceive[s] = 1;
        cs->nbits[s] = 0;
        cs->acc[s] = 0;
        opens = opens || cs->l != nullptr;
      }
    }
    if ((w & GMX_STEP_PREDICT) && cs->nbits[s] == 0) {
      wd |= 4u;
      cs->nl_forward[s] = 1;
      opens = opens || cs->l != nullptr;
    }
    if (cs->mb && (w & GMX_STEP_PREDICT)) {
      if (!cs->m_seen[s]) wd |= 8u;  // the stream's first Predict here: its context words are read wherever in a byte it is
      cs->m_seen[s] = 1;
      cs->m_bc[s] = cs->cb ? (cs->c_pos[s] == 7 ? 127u : 0u) : cs->ibc[s];  // (only "is it the byte's last bit" is read)
    }
    if (cs->cb && (w & GMX_STEP_PREDICT)) cs->c_pos[s] = (uint8_t)((cs->c_pos[s] + 1) & 7);
    cs->what_dev[s] = wd;
  }
  cs->seq_no += 1;
  for (int s = 0; s < S; ++s) cs->seq[s] = cs->seq_no;
  if (cs->l && opens) {
    // Adam's scalars of the backward passes these Perceives run, and the mirrors that say when passes fall
    lstm_stage_rows(cs->l, 0, S, 1, 1, 4u, cs->nl_perceive, cs->adam_host, 2);
    lstm_stage_rows(cs->l, 0, S, 1, 0, 1u, cs->nl_forward, cs->adam_host, 2);
  }
  if (cs->bar) {
    // the control words of all streams
    uint8_t* const dst = cs->d_in[cs->steps & 1];
    for (int e = 0; e < cs->n_ctl; ++e) memcpy(dst + cs->up.off[e], cs->h_in + cs->up.off[e], (size_t)S * cs->up.bps[e]);
    if (cs->l && opens) {
      const size_t at = (const uint8_t*)cs->bytes - cs->h_bd;  // bytes | nl_perceive | nl_forward, behind the distributions
      memcpy(cs->d_bd + at, cs->h_bd + at, cs->bd_bytes - at);
    }
    mb_store_fence();
  }
  const double ta = cs_trace_on() ? cs_now() : 0.0;
  if (cs->timed) HIPCHK(hipEventRecord(cs->t_ev[0], g->stream));
  HIPCHK(hipGraphLaunch(cs->exec[cs->steps & 1][(cs->l && opens) ? 1 : 0], g->stream));
  cs->bit_launches += 1;
  if (cs->timed) {
    HIPCHK(hipEventRecord(cs->t_ev[1], g->stream));
    cs->timed_ok = true;
  }
  if (cs_trace_on()) g_cs_trace.launch_s += cs_now() - ta;
  cs->in_flight = true;
  for (int s = 0; s < S; ++s) {
    const uint8_t w = cs->what[s];
    if (w & GMX_STEP_LEARN) {
      g->steps[s] += 1;
      cs->pending[s] = 0;
    }
    if (w & GMX_STEP_PREDICT) {
      cs->pending[s] = 1;
      if (cs->dc) cs->dc->via_byte[s] = 0;  // (the bit of its Learn is the caller's to give)
    }
    if (cs->cb && w) cs->cb->outstanding[s] = (w & GMX_STEP_PREDICT) ? 1 : 0;
    if (w) {
      g->fwd_done[s] = 0;
      if (cs->ib) cs->ib->fwd_done[s] = 0;
      if (cs->mb) cs->mb->fwd_done[s] = 0;
      if (cs->l) {
        cs->l->fwd_done[s] = 0;
        cs->l->range_read[s].valid = false;
      }
    }
  }
  for (gmx_lockstep* o : g->locksteps) o->predicted = false;  // the group has ONE latch: it is this object's now
  cs->steps += 1;
  return GMX_OK;
}

extern "C" int gmx_chainstep_wait(gmx_chainstep* cs) {
  if (!cs || !cs->g) return GMX_ERR_INVALID;
  if (!cs->in_flight) return GMX_OK;
  gmx_group* g = cs->g;
  const int S = cs->S;
  const double tb = cs_trace_on() ? cs_now() : 0.0;
  if (cs->stock) {
    // every stream's block stamps the step's number in pinned memory behind its p and outputs: no synchronisation of
    // the stream (which comes back some 12 us later); the stream is only asked, now and then, whether something failed
    const uint32_t want = cs->seq_no;
    uint64_t spins = 0;
    double t_first_look = 0.0;
    for (int s = 0; s < S; ++s) {
      while (__atomic_load_n(cs->stamp + s, __ATOMIC_ACQUIRE) != want) {
        if ((++spins & 0xfff) == 0) {
          // bounded, like the sessions' waits: a step is tens of microseconds
          const double now = cs_now();
          if (t_first_look == 0.0) t_first_look = now;
          if (now - t_first_look > 30.0) {
            g_last_error = "lock-step chain: a step does not end";
            cs->in_flight = false;
            return GMX_ERR_HIP;
          }
          const hipError_t q = hipStreamQuery(g->stream);
          if (q == hipSuccess) {
            if (__atomic_load_n(cs->stamp + s, __ATOMIC_ACQUIRE) == want) break;
            g_last_error = "lock-step chain: a step ended without its stamps";
            cs->in_flight = false;
            return GMX_ERR_HIP;
          }
          if (q != hipErrorNotReady) {
            cs->in_flight = false;
            HIPCHK(q);
          }
          (void)hipGetLastError();
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
    }
  } else {
    cs->in_flight = false;
    HIPCHK(hipStreamSynchronize(g->stream));
  }
  cs->in_flight = false;
  if (cs->dc && cs->dc->in_flight) cs_decoder_answered(cs);
  if (cs_trace_on()) {
    g_cs_trace.wait_s += cs_now() - tb;
    if (++g_cs_trace.n % 4096 == 0) {
      const uint64_t nc = g_cs_commits.exchange(0), ns = g_cs_commit_ns.exchange(0);
      fprintf(stderr, "[gmx step] hipGraphLaunch %.1f us, wait for the step %.1f us per step (%d streams); a commit %.0f ns (%llu of them)\n",
              g_cs_trace.launch_s * 1e6 / 4096, g_cs_trace.wait_s * 1e6 / 4096, S, nc ? (double)ns / (double)nc : 0.0,
              (unsigned long long)nc);
      g_cs_trace.launch_s = g_cs_trace.wait_s = 0;
    }
  }
  return GMX_OK;
}

extern "C" int gmx_chainstep_step(gmx_chainstep* cs) {
  const int rc = gmx_chainstep_launch(cs);
  return rc ? rc : gmx_chainstep_wait(cs);
}

// gmx_chainstep_step with HIP events around the step's graph: what the device spent on it (0 when nothing was queued).
extern "C" int gmx_chainstep_timed_step(gmx_chainstep* cs, float* device_ms) {
  if (!cs || !cs->g || !device_ms) return GMX_ERR_INVALID;
  *device_ms = 0.0f;
  HIPCHK(hipSetDevice(cs->g->device));
  for (hipEvent_t& ev : cs->t_ev)
    if (!ev) HIPCHK(hipEventCreate(&ev));
  cs->timed = true;
  cs->timed_ok = false;
  int rc = gmx_chainstep_launch(cs);
  cs->timed = false;
  if (!rc) rc = gmx_chainstep_wait(cs);
  if (rc || !cs->timed_ok) return rc;
  HIPCHK(hipEventSynchronize(cs->t_ev[1]));
  HIPCHK(hipEventElapsedTime(device_ms, cs->t_ev[0], cs->t_ev[1]));
  return GMX_OK;
}
