// gmx_lstm_ckpt.inc -- gmx_lstm_group_export / gmx_lstm_group_import: the checkpoint of streams [first, first + count)
// of an LSTM group in one call.  Included by gmx_capi.cpp behind gmx_ckpt.inc and gmx_lstm.inc; kernels in
// gmx_lstm_ckpt.hip, the layouts in gmx_lstm_ckpt.h.
//
// An LSTM bank is dense and its sections have one size, so nothing is counted: stream i's section lies at i * stride.
// Export: the host decides per stream how the 12-byte range header comes about (gmx_lstm_export's rules) and sends
// that as a small record; the pack kernel writes whole sections, header and scalars included.  Import: the host
// validates every stream's header and computes the bank's scal[0 .. 6] from the first bytes of its short section as
// gmx_lstm_import does -- the bit prediction with the host's logf, which the device's is not bit for bit --; then the
// banks are cleared on the device and the scatter kernel puts the sections back, rebuilding lin_t and hidden[50].
//
// Staging is gmx_ckpt_stage.h's, through gmx_ckpt.inc's allocations and link: one pass per half, both through the one
// staging set that hangs off the gmx_lstm.  No host copy of a bank exists.

extern "C" {
hipError_t gmx_launch_lstm_ckpt_pack(const GmxLstmCkptArgs* a, hipStream_t stream);
hipError_t gmx_launch_lstm_ckpt_scatter(const GmxLstmCkptArgs* a, hipStream_t stream);
}

struct GmxLstmCkptState {
  GmxLstmCkptLayout lay;
  GmxLstmCkptHalf* half_dev[2] = {nullptr, nullptr};
  uint8_t* rec_dev = nullptr;            // [streams] GmxLstmCkptOut or GmxLstmCkptIn
  size_t rec_cap = 0;                    // bytes
  CkptStaging stage;                     // one slice's packed bytes
};

static void lstm_ckpt_free(gmx_lstm* l) {
  GmxLstmCkptState* c = l->ckpt;
  if (!c) return;
  void* dev[] = {c->half_dev[0], c->half_dev[1], c->rec_dev};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  ckpt_stage_free(c->stage);
  delete c;
  l->ckpt = nullptr;
}

static int lstm_ckpt_state(gmx_lstm* l, GmxLstmCkptState** out) {
  if (!l->ckpt) {
    GmxLstmCkptState* c = new (std::nothrow) GmxLstmCkptState();
    if (!c) return GMX_ERR_NOMEM;
    if (!gmx_lstm_ckpt_layout(l->dev, &c->lay)) {
      delete c;
      return GMX_ERR_STATE;
    }
    l->ckpt = c;  // (from here gmx_lstm_destroy frees whatever exists)
    for (int h = 0; h < 2; ++h) {
      CKPT_ALLOC(hipMalloc((void**)&c->half_dev[h], sizeof(GmxLstmCkptHalf)));
      HIPCHK(hipMemcpy(c->half_dev[h], &c->lay.half[h], sizeof(GmxLstmCkptHalf), hipMemcpyHostToDevice));
    }
  } else if (!l->ckpt->half_dev[1]) {
    return GMX_ERR_NOMEM;  // the first call ran out of memory half way
  }
  *out = l->ckpt;
  return GMX_OK;
}

// Sections of one size: off[i] = i * stride, and the slices of a pass over them.
static bool lstm_ckpt_plan(int count, size_t stride, std::vector<size_t>& off, CkptPlan& plan) {
  try {
    off.resize((size_t)count + 1);
  } catch (const std::bad_alloc&) {
    return false;
  }
  for (int i = 0; i <= count; ++i) off[(size_t)i] = (size_t)i * stride;
  return ckpt_plan(off.data(), count, ckpt_stage_cap(), plan);
}

extern "C" int gmx_lstm_group_export(gmx_lstm* l, int first, int count, void* long_buf, size_t long_cap,
                                     void* short_buf, size_t short_cap, size_t* long_stride, size_t* short_stride) {
  const size_t LB = GMX_LSTM_CKPT_LONG_BYTES, SB = GMX_LSTM_CKPT_SHORT_BYTES;
  if (long_stride) *long_stride = LB;
  if (short_stride) *short_stride = SB;
  if (!l || first < 0 || count < 0 || first > l->S || count > l->S - first) return GMX_ERR_INVALID;
  if (l->any) return GMX_ERR_INVALID;  // the pack / scatter kernels know the stock layout only
  if (count == 0) return GMX_OK;
  if (!long_buf && !short_buf) return GMX_OK;  // sizing only
  if ((long_buf && long_cap < (size_t)count * LB) || (short_buf && short_cap < (size_t)count * SB))
    return GMX_ERR_INVALID;
  std::vector<size_t> off[2];
  CkptPlan plan[2];
  std::vector<GmxLstmCkptOut> rec;
  void* const bufs[2] = {long_buf, short_buf};
  size_t max_slice = 0, n_slices = 0;
  for (int h = 0; h < 2; ++h) {
    if (!bufs[h]) continue;
    if (!lstm_ckpt_plan(count, h == GMX_LCK_LONG ? LB : SB, off[h], plan[h])) return GMX_ERR_NOMEM;
    max_slice = std::max(max_slice, plan[h].max_slice);
    n_slices = std::max(n_slices, plan[h].slices());
  }
  HIPCHK(hipSetDevice(l->device));
  LSTM_CLOSE_SESSIONS(l);
  GmxLstmCkptState* c = nullptr;
  int rc = lstm_ckpt_state(l, &c);
  if (rc) return rc;
  if ((rc = c->stage.grow(max_slice, n_slices, ckpt_grow_dev<uint8_t>, ckpt_grow_host))) return rc;
  if (short_buf) {
    // the range header's source, per stream (gmx_lstm_export's rules; the sessions are closed: fwd_done is final)
    try {
      rec.resize((size_t)count);
    } catch (const std::bad_alloc&) {
      return GMX_ERR_NOMEM;
    }
    for (int i = 0; i < count; ++i) {
      GmxLstmCkptOut& r = rec[(size_t)i];
      const int s = first + i;
      r.fixed = 0;
      r.tmb[0] = 255, r.tmb[1] = 127, r.tmb[2] = 0;
      if (l->range_read[s].valid) {  // nothing has moved since this bank was read from a file
        r.fixed = 1;
        memcpy(r.tmb, l->range_read[s].tmb, sizeof r.tmb);
      } else if (l->fwd_done[s]) {  // between Predict and Perceive: as the forward's own Predict leaves it
        r.fixed = 1;
      }
    }
    if ((rc = ckpt_grow_dev(c->rec_dev, c->rec_cap, rec.size() * sizeof(GmxLstmCkptOut)))) return rc;
    HIPCHK(hipMemcpyAsync(c->rec_dev, rec.data(), rec.size() * sizeof(GmxLstmCkptOut), hipMemcpyHostToDevice,
                          l->stream));
  }
  HIPCHK(hipStreamSynchronize(l->stream));  // the bank's work is done; (pageable source: gone when this returns)
  CkptHipLink link{l->stream, c->stage.dev, nullptr};
  for (int h = 0; h < 2; ++h) {
    if (!bufs[h]) continue;
    GmxLstmCkptArgs a;
    memset(&a, 0, sizeof a);
    a.bank_floats = l->dev.bank_floats;
    a.half = c->half_dev[h];
    a.n_tiles = c->lay.half[h].n_tiles;
    a.buf = c->stage.dev;
    a.stride = c->lay.half[h].bytes;
    rc = ckpt_export_slices(link, plan[h], off[h].data(), bufs[h], c->stage, [&](size_t, int i0, int n) -> int {
      a.banks = (uint32_t*)(l->banks + (size_t)(first + i0) * l->dev.bank_floats);
      a.n_streams = n;
      a.out = h == GMX_LCK_SHORT ? (const GmxLstmCkptOut*)c->rec_dev + i0 : nullptr;
      HIPCHK(gmx_launch_lstm_ckpt_pack(&a, l->stream));
      return GMX_OK;
    });
    if (rc) return rc;
  }
  return GMX_OK;
}

// What gmx_lstm_import derives from a stream's header: validation, scal[0 .. 6], and the host mirrors.  (Restated
// here, not shared: the per-stream call is the yardstick this one is tested against and stays as it is.)
struct LstmCkptHead {
  int32_t tmb[3];
  uint32_t epoch;
  uint32_t steps;
  bool fresh;
};
static int lstm_ckpt_head(const GmxLstmCkptLayout& lay, const uint8_t* sh, LstmCkptHead* hd, GmxLstmCkptIn* in) {
  int32_t tmb[3];
  uint32_t epoch, l_epoch;
  uint64_t steps;
  float probs[GMX_L_NO];
  uint32_t hist[GMX_L_H];
  memcpy(tmb, sh, sizeof tmb);
  memcpy(probs, sh + lay.off_probs, sizeof probs);
  memcpy(hist, sh + lay.off_history, sizeof hist);
  memcpy(&epoch, sh + lay.off_epoch, 4);
  memcpy(&l_epoch, sh + lay.off_layer_epoch, 4);
  memcpy(&steps, sh + lay.off_update_steps, 8);
  // a model nobody has run: the constructor's range and byte distribution (lstm-model.cpp:7-10)
  bool fresh = tmb[0] == 255 && tmb[1] == 127 && tmb[2] == 0;
  for (int i = 0; fresh && i < GMX_L_NO; ++i) fresh = probs[i] == 1.0f / 256;
  // where a byte ends the range is that of its eighth bit; anything else is a checkpoint taken inside a byte
  const bool boundary =
      !fresh && tmb[2] >= 0 && tmb[2] <= 254 && !(tmb[2] & 1) && tmb[1] == tmb[2] && tmb[0] == tmb[2] + 1;
  if (epoch >= (uint32_t)GMX_L_H || l_epoch >= (uint32_t)GMX_L_H || steps > 3000 ||
      !(0 <= tmb[2] && tmb[2] <= tmb[1] && tmb[1] <= tmb[0] && tmb[0] <= 255))
    return GMX_ERR_FORMAT;
  uint32_t last_byte = 0, context = 0;
  float prediction = 0.0f;
  if (!fresh) {
    const uint32_t newest = hist[(epoch + GMX_L_H - (boundary ? 1 : 2)) % GMX_L_H];
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
  memset(in, 0, sizeof *in);
  in->scal[0] = epoch;
  in->scal[1] = l_epoch;
  in->scal[2] = (uint32_t)steps;
  in->scal[3] = last_byte;
  in->scal[4] = context;
  memcpy(&in->scal[5], &prediction, 4);
  in->scal[6] = fresh ? 0u : 1u;
  memcpy(hd->tmb, tmb, sizeof tmb);
  hd->epoch = epoch;
  hd->steps = (uint32_t)steps;
  hd->fresh = fresh;
  return GMX_OK;
}

extern "C" int gmx_lstm_group_import(gmx_lstm* l, int first, int count, const void* long_buf, size_t long_bytes,
                                     const void* short_buf, size_t short_bytes) {
  const size_t LB = GMX_LSTM_CKPT_LONG_BYTES, SB = GMX_LSTM_CKPT_SHORT_BYTES;
  if (!l || first < 0 || count < 0 || first > l->S || count > l->S - first) return GMX_ERR_INVALID;
  if (l->any) return GMX_ERR_INVALID;  // the pack / scatter kernels know the stock layout only
  if (count == 0) return GMX_OK;
  if (!long_buf || !short_buf) return GMX_ERR_INVALID;
  if (long_bytes != (size_t)count * LB || short_bytes != (size_t)count * SB) return GMX_ERR_FORMAT;
  HIPCHK(hipSetDevice(l->device));
  GmxLstmCkptState* c = nullptr;
  int rc = lstm_ckpt_state(l, &c);
  if (rc) return rc;
  // ---- every stream's header is checked before any bank is touched
  std::vector<LstmCkptHead> head;
  std::vector<GmxLstmCkptIn> rec;
  std::vector<size_t> off[2];
  CkptPlan plan[2];
  try {
    head.resize((size_t)count);
    rec.resize((size_t)count);
  } catch (const std::bad_alloc&) {
    return GMX_ERR_NOMEM;
  }
  for (int i = 0; i < count; ++i)
    if ((rc = lstm_ckpt_head(c->lay, (const uint8_t*)short_buf + (size_t)i * SB, &head[(size_t)i], &rec[(size_t)i])))
      return rc;
  if (!lstm_ckpt_plan(count, LB, off[0], plan[0]) || !lstm_ckpt_plan(count, SB, off[1], plan[1])) return GMX_ERR_NOMEM;
  LSTM_CLOSE_SESSIONS(l);
  if ((rc = c->stage.grow(std::max(plan[0].max_slice, plan[1].max_slice), std::max(plan[0].slices(), plan[1].slices()),
                          ckpt_grow_dev<uint8_t>, ckpt_grow_host)))
    return rc;
  if ((rc = ckpt_grow_dev(c->rec_dev, c->rec_cap, rec.size() * sizeof(GmxLstmCkptIn)))) return rc;
  HIPCHK(hipMemcpyAsync(c->rec_dev, rec.data(), rec.size() * sizeof(GmxLstmCkptIn), hipMemcpyHostToDevice, l->stream));
  HIPCHK(hipStreamSynchronize(l->stream));  // the bank's work is done; (pageable source: gone when this returns)
  // ---- from here the banks change: cleared first, as the per-stream import builds its image from zeros
  HIPCHK(hipMemsetAsync(l->banks + (size_t)first * l->dev.bank_floats, 0, (size_t)count * l->dev.bank_floats * 4,
                        l->stream));
  CkptHipLink link{l->stream, c->stage.dev, nullptr};
  const void* const bufs[2] = {long_buf, short_buf};
  for (int h = 0; h < 2; ++h) {
    GmxLstmCkptArgs a;
    memset(&a, 0, sizeof a);
    a.bank_floats = l->dev.bank_floats;
    a.half = c->half_dev[h];
    a.n_tiles = c->lay.half[h].n_tiles;
    a.buf = c->stage.dev;
    a.stride = c->lay.half[h].bytes;
    rc = ckpt_import_slices(link, plan[h], off[h].data(), bufs[h], c->stage, [&](size_t, int i0, int n) -> int {
      a.banks = (uint32_t*)(l->banks + (size_t)(first + i0) * l->dev.bank_floats);
      a.n_streams = n;
      a.in = h == GMX_LCK_SHORT ? (const GmxLstmCkptIn*)c->rec_dev + i0 : nullptr;
      HIPCHK(gmx_launch_lstm_ckpt_scatter(&a, l->stream));
      return GMX_OK;
    });
    if (rc) return rc;
  }
  // the host mirrors, per stream as gmx_lstm_import sets them
  for (int i = 0; i < count; ++i) {
    const LstmCkptHead& hd = head[(size_t)i];
    const int s = first + i;
    l->bytes_seen[s] = hd.epoch;  // only its value mod 100 matters (lstm_launch)
    l->update_steps[s] = hd.steps;
    l->fwd_done[s] = hd.fresh ? 0 : 1;  // the file does not say whether the newest forward has been perceived
    l->range_read[s].valid = true;
    memcpy(l->range_read[s].tmb, hd.tmb, sizeof hd.tmb);
  }
  return GMX_OK;
}
