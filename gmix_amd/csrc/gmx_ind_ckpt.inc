// gmx_ind_ckpt.inc -- gmx_indirect_group_export / gmx_indirect_group_import: the checkpoint of streams
// [first, first + count) of an Indirect group in one call, at the cost of the entries that are alive.  Included by
// gmx_capi.cpp behind gmx_ckpt.inc and gmx_indirect.inc; kernels in gmx_ind_ckpt.hip.
//
// Export: one count launch over all the streams (live entries per chunk of 16 Ki entries), the counts come to the
// host, which per (stream, model) sums them to the header's `cnt`, decides sparse or dense as the file format does
// (cnt < size / 3), and gives every model its byte offset, every chunk the index of its first record and every stream
// its section size -- all a sizing call needs; the pack kernel then writes the sections on the device.
// Import: the host validates every section first (gmx_indirect_import's rules, and the keys of a sparse model strictly
// ascending); then the banks are reset on the device (the image gmx_indirect_import uploads: every entry 0x00ff,
// zeros behind the tables) and the scatter kernel puts entries and logits back.
//
// Staging is gmx_ckpt_stage.h's, through gmx_ckpt.inc's allocations and link.  No second copy of a bank exists on
// either side of the link.

extern "C" {
hipError_t gmx_launch_ind_ckpt_count(const GmxIndCkptArgs* a, hipStream_t stream);
hipError_t gmx_launch_ind_ckpt_pack(const GmxIndCkptArgs* a, hipStream_t stream);
hipError_t gmx_launch_ind_ckpt_scatter(const GmxIndCkptArgs* a, int n_models, unsigned blocks_x, hipStream_t stream);
}

struct GmxIndCkptState {
  std::vector<GmxIndCkptChunk> chunks;   // the bank description's chunk list (one stream's)
  std::vector<uint32_t> model_first;     // [k + 1] first chunk of every model
  GmxIndCkptChunk* chunks_dev = nullptr;
  uint32_t* cnt_dev = nullptr;           // [streams][chunks]
  uint32_t* base_dev = nullptr;          // [streams][chunks]
  uint32_t* mcnt_dev = nullptr;          // [streams][k]
  uint64_t* moff_dev = nullptr;          // [streams][k]
  CkptStaging stage;                     // one slice's packed bytes
  size_t cnt_cap = 0, base_cap = 0, mcnt_cap = 0, moff_cap = 0;  // bytes
};

static void ind_ckpt_free(gmx_indirect* ib) {
  GmxIndCkptState* c = ib->ckpt;
  if (!c) return;
  void* dev[] = {c->chunks_dev, c->cnt_dev, c->base_dev, c->mcnt_dev, c->moff_dev};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  ckpt_stage_free(c->stage);
  delete c;
  ib->ckpt = nullptr;
}

static int ind_ckpt_state(gmx_indirect* ib, GmxIndCkptState** out) {
  if (!ib->ckpt) {
    GmxIndCkptState* c = new (std::nothrow) GmxIndCkptState();
    if (!c) return GMX_ERR_NOMEM;
    const GmxIndDev& d = ib->dev;
    for (int j = 0; j < d.k; ++j) {
      c->model_first.push_back((uint32_t)c->chunks.size());
      for (uint64_t e = 0; e < d.m[j].size; e += GMX_IND_CKPT_CHUNK)
        c->chunks.push_back(GmxIndCkptChunk{(uint32_t)j, (uint32_t)e});
    }
    c->model_first.push_back((uint32_t)c->chunks.size());
    ib->ckpt = c;  // (from here gmx_indirect_destroy frees whatever exists)
    const size_t bytes = c->chunks.size() * sizeof(GmxIndCkptChunk);
    CKPT_ALLOC(hipMalloc((void**)&c->chunks_dev, bytes));
    HIPCHK(hipMemcpy(c->chunks_dev, c->chunks.data(), bytes, hipMemcpyHostToDevice));
  } else if (!ib->ckpt->chunks_dev) {
    return GMX_ERR_NOMEM;  // the first call ran out of memory half way
  }
  *out = ib->ckpt;
  return GMX_OK;
}

// bytes of a model's part of a section behind its u32 cnt and in front of its logits
static inline uint64_t ind_ckpt_body(uint32_t cnt, uint32_t size) { return cnt < size / 3 ? 6ull * cnt : 2ull * size; }

extern "C" int gmx_indirect_group_export(gmx_indirect* ib, int first, int count, void* buf, size_t cap, size_t* off) {
  if (!ib || !off || first < 0 || count < 0 || first > ib->S || count > ib->S - first) return GMX_ERR_INVALID;
  off[0] = 0;
  if (count == 0) return GMX_OK;
  const GmxIndDev& d = ib->dev;
  const size_t k = (size_t)d.k;
  HIPCHK(hipSetDevice(ib->device));
  int rc = ind_sessions_close(ib);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(ib->stream));
  GmxIndCkptState* c = nullptr;
  if ((rc = ind_ckpt_state(ib, &c))) return rc;
  const size_t K = c->chunks.size();
  if ((rc = ckpt_grow_dev(c->cnt_dev, c->cnt_cap, (size_t)count * K * sizeof(uint32_t)))) return rc;
  GmxIndCkptArgs a;
  memset(&a, 0, sizeof a);
  a.dev = ib->dev_d;
  a.chunks = c->chunks_dev;
  a.n_chunks = (uint32_t)K;
  // ---- count, and the scan on the host
  for (int i0 = 0; i0 < count; i0 += kCkptMaxSliceStreams) {
    a.banks = ib->banks + (size_t)(first + i0) * d.bank_bytes;
    a.n_streams = std::min(count - i0, kCkptMaxSliceStreams);
    a.chunk_cnt = c->cnt_dev + (size_t)i0 * K;
    HIPCHK(gmx_launch_ind_ckpt_count(&a, ib->stream));
  }
  std::vector<uint32_t> cnt, mcnt;
  std::vector<uint64_t> moff;
  try {
    cnt.resize((size_t)count * K);  // on the way back: every chunk's first record index
    mcnt.resize((size_t)count * k);
    moff.resize((size_t)count * k);
  } catch (const std::bad_alloc&) {
    return GMX_ERR_NOMEM;
  }
  HIPCHK(hipMemcpyAsync(cnt.data(), c->cnt_dev, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ib->stream));
  HIPCHK(hipStreamSynchronize(ib->stream));
  for (int i = 0; i < count; ++i) {
    uint64_t pos = 0;  // inside the stream's section
    for (size_t j = 0; j < k; ++j) {
      uint32_t live = 0;
      for (uint32_t q = c->model_first[j]; q < c->model_first[j + 1]; ++q) {
        const uint32_t n = cnt[(size_t)i * K + q];
        cnt[(size_t)i * K + q] = live;
        live += n;
      }
      mcnt[(size_t)i * k + j] = live;
      moff[(size_t)i * k + j] = pos;
      pos += 4 + ind_ckpt_body(live, d.m[j].size) + 2048;
    }
    off[i + 1] = off[i] + (size_t)pos;
  }
  if (!buf) return GMX_OK;  // sizing only
  if (cap < off[count]) return GMX_ERR_INVALID;
  // ---- pack, slice by slice
  CkptPlan plan;
  if (!ckpt_plan(off, count, ckpt_stage_cap(), plan)) return GMX_ERR_NOMEM;
  for (int i = 0; i < count; ++i)  // offsets inside the slice's buffer
    for (size_t j = 0; j < k; ++j) moff[(size_t)i * k + j] += plan.shift[i];
  if ((rc = ckpt_grow_dev(c->base_dev, c->base_cap, cnt.size() * sizeof(uint32_t)))) return rc;
  if ((rc = ckpt_grow_dev(c->mcnt_dev, c->mcnt_cap, mcnt.size() * sizeof(uint32_t)))) return rc;
  if ((rc = ckpt_grow_dev(c->moff_dev, c->moff_cap, moff.size() * sizeof(uint64_t)))) return rc;
  if ((rc = ckpt_stage_grow(c->stage, plan))) return rc;
  HIPCHK(hipMemcpyAsync(c->base_dev, cnt.data(), cnt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ib->stream));
  HIPCHK(hipMemcpyAsync(c->mcnt_dev, mcnt.data(), mcnt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ib->stream));
  HIPCHK(hipMemcpyAsync(c->moff_dev, moff.data(), moff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ib->stream));
  HIPCHK(hipStreamSynchronize(ib->stream));  // (pageable sources: gone when this function returns)
  a.buf = c->stage.dev;
  CkptHipLink link{ib->stream, c->stage.dev, nullptr};
  return ckpt_export_slices(link, plan, off, buf, c->stage, [&](size_t, int i0, int n) -> int {
    a.banks = ib->banks + (size_t)(first + i0) * d.bank_bytes;
    a.n_streams = n;
    a.chunk_cnt = c->cnt_dev + (size_t)i0 * K;
    a.chunk_base = c->base_dev + (size_t)i0 * K;
    a.model_cnt = c->mcnt_dev + (size_t)i0 * k;
    a.model_off = c->moff_dev + (size_t)i0 * k;
    HIPCHK(gmx_launch_ind_ckpt_pack(&a, ib->stream));
    return GMX_OK;
  });
}

// gmx_indirect_import's rules over one stream's section, plus: keys of a sparse model strictly ascending.
static int ind_ckpt_validate(const GmxIndDev& d, const uint8_t* p, size_t bytes, uint32_t* mcnt, uint64_t* moff) {
  const uint8_t* const begin = p;
  const uint8_t* const end = p + bytes;
  for (int j = 0; j < d.k; ++j) {
    const uint32_t size = d.m[j].size;
    if (end - p < 4) return GMX_ERR_FORMAT;
    uint32_t cnt;
    memcpy(&cnt, p, 4);
    if (cnt > size) return GMX_ERR_FORMAT;
    mcnt[j] = cnt;
    moff[j] = (uint64_t)(p - begin);
    p += 4;
    if ((uint64_t)(end - p) < ind_ckpt_body(cnt, size)) return GMX_ERR_FORMAT;
    if (cnt < size / 3) {
      uint32_t prev = 0;
      for (uint32_t i = 0; i < cnt; ++i, p += 6) {
        uint32_t key;
        memcpy(&key, p, 4);
        if (key >= size) return GMX_ERR_FORMAT;
        if (i && key <= prev) return GMX_ERR_FORMAT;  // one lane per record: no entry twice
        prev = key;
      }
    } else {
      p += 2ull * size;
    }
    if (end - p < 2048) return GMX_ERR_FORMAT;
    p += 2048;
  }
  return p == end ? GMX_OK : GMX_ERR_FORMAT;
}

extern "C" int gmx_indirect_group_import(gmx_indirect* ib, int first, int count, const void* buf, const size_t* off) {
  if (!ib || !off || first < 0 || count < 0 || first > ib->S || count > ib->S - first) return GMX_ERR_INVALID;
  if (count == 0) return GMX_OK;
  if (!buf) return GMX_ERR_INVALID;
  for (int i = 0; i < count; ++i)
    if (off[i + 1] < off[i]) return GMX_ERR_INVALID;
  const GmxIndDev& d = ib->dev;
  const size_t k = (size_t)d.k;
  // ---- every section is checked before any bank is touched
  std::vector<uint32_t> mcnt;
  std::vector<uint64_t> moff;
  try {
    mcnt.resize((size_t)count * k);
    moff.resize((size_t)count * k);
  } catch (const std::bad_alloc&) {
    return GMX_ERR_NOMEM;
  }
  for (int i = 0; i < count; ++i) {
    int rcv = ind_ckpt_validate(d, (const uint8_t*)buf + off[i], off[i + 1] - off[i], &mcnt[(size_t)i * k],
                                &moff[(size_t)i * k]);
    if (rcv) return rcv;
  }
  CkptPlan plan;
  if (!ckpt_plan(off, count, ckpt_stage_cap(), plan)) return GMX_ERR_NOMEM;
  for (int i = 0; i < count; ++i)
    for (size_t j = 0; j < k; ++j) moff[(size_t)i * k + j] += plan.shift[i];
  HIPCHK(hipSetDevice(ib->device));
  int rc = ind_sessions_close(ib);
  if (rc) return rc;
  GmxIndCkptState* c = nullptr;
  if ((rc = ind_ckpt_state(ib, &c))) return rc;
  if ((rc = ckpt_grow_dev(c->mcnt_dev, c->mcnt_cap, mcnt.size() * sizeof(uint32_t)))) return rc;
  if ((rc = ckpt_grow_dev(c->moff_dev, c->moff_cap, moff.size() * sizeof(uint64_t)))) return rc;
  if ((rc = ckpt_stage_grow(c->stage, plan))) return rc;
  HIPCHK(hipStreamSynchronize(ib->stream));
  // ---- from here the banks change
  for (int i = 0; i < count; ++i) {
    ib->fwd_done[first + i] = 0;
    ind_sessions_drop_forward(ib, first + i);
  }
  HIPCHK(hipMemcpyAsync(c->mcnt_dev, mcnt.data(), mcnt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ib->stream));
  HIPCHK(hipMemcpyAsync(c->moff_dev, moff.data(), moff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ib->stream));
  for (int i0 = 0; i0 < count; i0 += kCkptMaxSliceStreams)
    HIPCHK(gmx_launch_indirect_init(ib->banks + (size_t)(first + i0) * d.bank_bytes, d.bank_bytes, ib->tab_bytes,
                                    std::min(count - i0, kCkptMaxSliceStreams), ib->stream));
  GmxIndCkptArgs a;
  memset(&a, 0, sizeof a);
  a.dev = ib->dev_d;
  a.buf = c->stage.dev;
  CkptHipLink link{ib->stream, c->stage.dev, nullptr};
  return ckpt_import_slices(link, plan, off, buf, c->stage, [&](size_t, int i0, int n) -> int {
    uint32_t most = 0;  // records, or entries of a dense model, of the slice's largest model
    for (size_t q = 0; q < (size_t)n * k; ++q) {
      const uint32_t m = mcnt[(size_t)i0 * k + q], size = d.m[q % k].size;
      most = std::max(most, m < size / 3 ? m : size);
    }
    a.banks = ib->banks + (size_t)(first + i0) * d.bank_bytes;
    a.n_streams = n;
    a.model_cnt = c->mcnt_dev + (size_t)i0 * k;
    a.model_off = c->moff_dev + (size_t)i0 * k;
    HIPCHK(gmx_launch_ind_ckpt_scatter(&a, d.k, std::min(std::max(most / 256u + 1u, 1u), 1024u), ib->stream));
    return GMX_OK;
  });
}
