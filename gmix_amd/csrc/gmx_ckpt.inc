// gmx_ckpt.inc -- gmx_group_export / gmx_group_import: the checkpoint of streams [first, first + count) of a group in
// one call, at the cost of the rows that have been learned.  Included by gmx_capi.cpp; kernels in gmx_ckpt.hip.
//
// Export: one count launch over all the streams (learned rows per chunk of 256 rows), the counts come to the host
// (streams x chunks integers: 1 376 per stream of the reference's topology), the host's exclusive scan gives every
// chunk its byte offset and every stream its section size, and the pack kernel writes the sections on the device.
// Import: the host validates every 12-byte record head of every section first; then the banks are zeroed on the
// device and the scatter kernel puts the records back.
//
// Staging: gmx_ckpt_stage.h -- slices of consecutive streams through one device buffer and two pinned host buffers.
// Here are its allocations and its link to the device, which the Indirect and the context group checkpoints use too.

extern "C" {
hipError_t gmx_launch_ckpt_count(const GmxCkptArgs* a, hipStream_t stream);
hipError_t gmx_launch_ckpt_pack(const GmxCkptArgs* a, hipStream_t stream);
hipError_t gmx_launch_ckpt_scatter(const GmxCkptArgs* a, int n_mixers, unsigned blocks_x, hipStream_t stream);
}

struct GmxCkptState {
  std::vector<GmxCkptChunk> chunks;      // the topology's chunk list (one stream's)
  std::vector<uint32_t> mixer_first;     // [m + 1] first chunk of every mixer
  GmxCkptChunk* chunks_dev = nullptr;
  uint32_t* cnt_dev = nullptr;           // [streams][chunks]
  uint64_t* off_dev = nullptr;           // export: [streams][chunks]; import: [streams][m]
  uint32_t* mcnt_dev = nullptr;          // [streams][m]
  uint32_t* short_dev = nullptr;         // [streams][6 m]
  CkptStaging stage;                     // one slice's packed bytes
  size_t cnt_cap = 0, off_cap = 0, mcnt_cap = 0, short_cap = 0;  // bytes
};

static void ckpt_stage_free(CkptStaging& st) {
  if (st.dev) (void)hipFree(st.dev);
  for (uint8_t* p : st.host)
    if (p) (void)hipHostFree(p);
}

static void ckpt_free(gmx_group* g) {
  GmxCkptState* c = g->ckpt;
  if (!c) return;
  void* dev[] = {c->chunks_dev, c->cnt_dev, c->off_dev, c->mcnt_dev, c->short_dev};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  ckpt_stage_free(c->stage);
  delete c;
  g->ckpt = nullptr;
}

#define CKPT_ALLOC(call)                                                                  \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      int r_ = hip_fail(e_, #call);                                                       \
      return e_ == hipErrorOutOfMemory || e_ == hipErrorMemoryAllocation ? GMX_ERR_NOMEM : r_; \
    }                                                                                     \
  } while (0)

// grow-only buffers: the next checkpoint of the group finds them
template <class T>
static int ckpt_grow_dev(T*& p, size_t& cap, size_t bytes) {
  if (bytes <= cap) return GMX_OK;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  CKPT_ALLOC(hipMalloc((void**)&p, bytes));
  cap = bytes;
  return GMX_OK;
}
static int ckpt_grow_host(uint8_t*& p, size_t& cap, size_t bytes) {
  if (bytes <= cap) return GMX_OK;
  if (p) (void)hipHostFree(p);
  p = nullptr;
  cap = 0;
  CKPT_ALLOC(hipHostMalloc((void**)&p, bytes, hipHostMallocDefault));
  cap = bytes;
  return GMX_OK;
}

static int ckpt_state(gmx_group* g, GmxCkptState** out) {
  if (!g->ckpt) {
    GmxCkptState* c = new (std::nothrow) GmxCkptState();
    if (!c) return GMX_ERR_NOMEM;
    const GmxTopoDev& t = g->topo;
    for (int j = 0; j < t.m; ++j) {
      c->mixer_first.push_back((uint32_t)c->chunks.size());
      for (uint64_t r = 0; r < t.mx[j].table_size; r += GMX_CKPT_CHUNK)
        c->chunks.push_back(GmxCkptChunk{(uint32_t)j, (uint32_t)r});
    }
    c->mixer_first.push_back((uint32_t)c->chunks.size());
    g->ckpt = c;  // (from here gmx_group_destroy frees whatever exists)
    const size_t bytes = c->chunks.size() * sizeof(GmxCkptChunk);
    CKPT_ALLOC(hipMalloc((void**)&c->chunks_dev, bytes));
    HIPCHK(hipMemcpy(c->chunks_dev, c->chunks.data(), bytes, hipMemcpyHostToDevice));
  } else if (!g->ckpt->chunks_dev) {
    return GMX_ERR_NOMEM;  // the first call ran out of memory half way
  }
  *out = g->ckpt;
  return GMX_OK;
}

static int ckpt_stage_grow(CkptStaging& st, const CkptPlan& p) {
  return st.grow(p.max_slice, p.slices(), ckpt_grow_dev<uint8_t>, ckpt_grow_host);
}

// The link of gmx_ckpt_stage.h's pipelines: a bank's stream and its staging device buffer.  `ops` (nullable) counts
// the waits and the transfers, as the callers count their launches.
struct CkptHipLink {
  hipStream_t stream;
  uint8_t* dev;
  int* ops;
  int wait() {
    if (ops) ++*ops;
    HIPCHK(hipStreamSynchronize(stream));
    return GMX_OK;
  }
  int to_host(uint8_t* h, size_t bytes) {
    if (ops) ++*ops;
    HIPCHK(hipMemcpyAsync(h, dev, bytes, hipMemcpyDeviceToHost, stream));
    return GMX_OK;
  }
  int to_device(uint8_t* h, size_t bytes) {
    if (ops) ++*ops;
    HIPCHK(hipMemcpyAsync(dev, h, bytes, hipMemcpyHostToDevice, stream));
    return GMX_OK;
  }
};

extern "C" int gmx_group_export(gmx_group* g, int first, int count, void* long_buf, size_t long_cap,
                                size_t* long_off, void* short_buf) {
  if (!g || !long_off || first < 0 || count < 0 || first > g->S || count > g->S - first) return GMX_ERR_INVALID;
  if ((long_buf == nullptr) != (short_buf == nullptr)) return GMX_ERR_INVALID;
  long_off[0] = 0;
  if (count == 0) return GMX_OK;
  const GmxTopoDev& t = g->topo;
  const size_t m = (size_t)t.m;
  HIPCHK(hipSetDevice(g->device));
  int rc = sessions_close(g, true);
  if (rc) return rc;
  GmxCkptState* c = nullptr;
  rc = ckpt_state(g, &c);
  if (rc) return rc;
  const size_t K = c->chunks.size();
  rc = ckpt_grow_dev(c->cnt_dev, c->cnt_cap, (size_t)count * K * sizeof(uint32_t));
  if (rc) return rc;
  GmxCkptArgs a;
  memset(&a, 0, sizeof a);
  a.topo = g->topo_dev;
  a.chunks = c->chunks_dev;
  a.n_chunks = (uint32_t)K;
  // ---- count, and the scan on the host
  for (int i0 = 0; i0 < count; i0 += kCkptMaxSliceStreams) {
    a.banks = g->banks + (size_t)(first + i0) * t.bank_bytes;
    a.n_streams = std::min(count - i0, kCkptMaxSliceStreams);
    a.chunk_cnt = c->cnt_dev + (size_t)i0 * K;
    HIPCHK(gmx_launch_ckpt_count(&a, g->stream));
  }
  std::vector<uint32_t> cnt, mcnt;
  std::vector<uint64_t> coff;
  try {
    cnt.resize((size_t)count * K);
    mcnt.resize((size_t)count * m);
    coff.resize((size_t)count * K);
  } catch (const std::bad_alloc&) {
    return GMX_ERR_NOMEM;
  }
  HIPCHK(hipMemcpyAsync(cnt.data(), c->cnt_dev, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  for (int i = 0; i < count; ++i) {
    uint64_t pos = 0;  // inside the stream's section
    for (size_t j = 0; j < m; ++j) {
      const uint64_t rec = 12 + 4 * (uint64_t)t.mx[j].weight_size;
      pos += 8;
      uint32_t rows = 0;
      for (uint32_t k = c->mixer_first[j]; k < c->mixer_first[j + 1]; ++k) {
        coff[(size_t)i * K + k] = pos;
        pos += cnt[(size_t)i * K + k] * rec;
        rows += cnt[(size_t)i * K + k];
      }
      mcnt[(size_t)i * m + j] = rows;
    }
    long_off[i + 1] = long_off[i] + (size_t)pos;
  }
  if (!long_buf) return GMX_OK;  // sizing only
  if (long_cap < long_off[count]) return GMX_ERR_INVALID;
  // ---- pack, slice by slice
  CkptPlan plan;
  if (!ckpt_plan(long_off, count, ckpt_stage_cap(), plan)) return GMX_ERR_NOMEM;
  for (int i = 0; i < count; ++i)  // offsets inside the slice's buffer
    for (size_t q = 0; q < K; ++q) coff[(size_t)i * K + q] += plan.shift[i];
  if ((rc = ckpt_grow_dev(c->off_dev, c->off_cap, coff.size() * sizeof(uint64_t)))) return rc;
  if ((rc = ckpt_grow_dev(c->mcnt_dev, c->mcnt_cap, mcnt.size() * sizeof(uint32_t)))) return rc;
  if ((rc = ckpt_grow_dev(c->short_dev, c->short_cap, (size_t)count * 24 * m))) return rc;
  if ((rc = ckpt_stage_grow(c->stage, plan))) return rc;
  HIPCHK(hipMemcpyAsync(c->off_dev, coff.data(), coff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, g->stream));
  HIPCHK(hipMemcpyAsync(c->mcnt_dev, mcnt.data(), mcnt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));  // (pageable sources: gone when this function returns)
  a.long_buf = (uint32_t*)c->stage.dev;
  CkptHipLink link{g->stream, c->stage.dev, nullptr};
  rc = ckpt_export_slices(link, plan, long_off, long_buf, c->stage, [&](size_t, int i0, int n) -> int {
    a.banks = g->banks + (size_t)(first + i0) * t.bank_bytes;
    a.n_streams = n;
    a.chunk_cnt = c->cnt_dev + (size_t)i0 * K;
    a.chunk_off = c->off_dev + (size_t)i0 * K;
    a.mixer_cnt = c->mcnt_dev + (size_t)i0 * m;
    a.short_buf = c->short_dev + (size_t)i0 * 6 * m;
    HIPCHK(gmx_launch_ckpt_pack(&a, g->stream));
    return GMX_OK;
  });
  if (rc) return rc;
  HIPCHK(hipMemcpy(short_buf, c->short_dev, (size_t)count * 24 * m, hipMemcpyDeviceToHost));
  return GMX_OK;
}

// gmx_bank_import's rules over one stream's section, plus: rows of a mixer strictly ascending.
static int ckpt_validate(const GmxTopoDev& t, const uint8_t* p, size_t bytes, const uint8_t* shrt, uint32_t* mcnt,
                         uint64_t* moff) {
  uint64_t s0 = 0;
  for (int j = 0; j < t.m; ++j) {
    uint64_t sj;
    memcpy(&sj, shrt + 24u * (size_t)j, 8);
    if (j == 0) s0 = sj;
    if (sj != s0) return GMX_ERR_FORMAT;  // every Mixer learns on every bit: steps_ agree
  }
  if (bytes % 4) return GMX_ERR_FORMAT;
  const uint8_t* const begin = p;
  const uint8_t* const end = p + bytes;
  for (int j = 0; j < t.m; ++j) {
    const GmxMixerDev& x = t.mx[j];
    if (end - p < 8) return GMX_ERR_FORMAT;
    uint32_t cnt, input_size;
    memcpy(&cnt, p, 4);
    memcpy(&input_size, p + 4, 4);
    p += 8;
    if (cnt > x.table_size || (cnt && input_size != x.weight_size)) return GMX_ERR_FORMAT;
    const size_t rec = 12 + 4 * (size_t)x.weight_size;
    if ((size_t)(end - p) / rec < cnt) return GMX_ERR_FORMAT;
    mcnt[j] = cnt;
    moff[j] = (uint64_t)(p - begin);
    uint32_t prev = 0;
    for (uint32_t i = 0; i < cnt; ++i, p += rec) {
      uint32_t r;
      uint64_t steps;
      memcpy(&r, p, 4);
      memcpy(&steps, p + 4, 8);
      if (r >= x.table_size || steps == 0) return GMX_ERR_FORMAT;  // a stored row has been learned at least once
      if (i && r <= prev) return GMX_ERR_FORMAT;  // one wave per record: no row twice
      prev = r;
    }
  }
  return p == end ? GMX_OK : GMX_ERR_FORMAT;
}

extern "C" int gmx_group_import(gmx_group* g, int first, int count, const void* long_buf, const size_t* long_off,
                                const void* short_buf) {
  if (!g || !long_off || first < 0 || count < 0 || first > g->S || count > g->S - first) return GMX_ERR_INVALID;
  if (count == 0) return GMX_OK;
  if (!long_buf || !short_buf) return GMX_ERR_INVALID;
  for (int i = 0; i < count; ++i)
    if (long_off[i + 1] < long_off[i]) return GMX_ERR_INVALID;
  const GmxTopoDev& t = g->topo;
  const size_t m = (size_t)t.m;
  // ---- every section is checked before any bank is touched
  std::vector<uint32_t> mcnt;
  std::vector<uint64_t> moff;
  try {
    mcnt.resize((size_t)count * m);
    moff.resize((size_t)count * m);
  } catch (const std::bad_alloc&) {
    return GMX_ERR_NOMEM;
  }
  for (int i = 0; i < count; ++i) {
    int rcv = ckpt_validate(t, (const uint8_t*)long_buf + long_off[i], long_off[i + 1] - long_off[i],
                            (const uint8_t*)short_buf + (size_t)i * 24 * m, &mcnt[(size_t)i * m], &moff[(size_t)i * m]);
    if (rcv) return rcv;
  }
  CkptPlan plan;
  if (!ckpt_plan(long_off, count, ckpt_stage_cap(), plan)) return GMX_ERR_NOMEM;
  for (int i = 0; i < count; ++i)
    for (size_t j = 0; j < m; ++j) moff[(size_t)i * m + j] += plan.shift[i];
  HIPCHK(hipSetDevice(g->device));
  int rc = sessions_close(g, true);
  if (rc) return rc;
  GmxCkptState* c = nullptr;
  if ((rc = ckpt_state(g, &c))) return rc;
  if ((rc = ckpt_grow_dev(c->off_dev, c->off_cap, moff.size() * sizeof(uint64_t)))) return rc;
  if ((rc = ckpt_grow_dev(c->mcnt_dev, c->mcnt_cap, mcnt.size() * sizeof(uint32_t)))) return rc;
  if ((rc = ckpt_grow_dev(c->short_dev, c->short_cap, (size_t)count * 24 * m))) return rc;
  if ((rc = ckpt_stage_grow(c->stage, plan))) return rc;
  // ---- from here the banks change
  for (int i = 0; i < count; ++i) {
    const int s = first + i;
    if (s < (int)g->sessions.size() && g->sessions[s]) g->sessions[s]->fwd_live = false;
    memcpy(&g->steps[s], (const uint8_t*)short_buf + (size_t)i * 24 * m, 8);
    g->fwd_done[s] = 0;
  }
  for (gmx_lockstep* ls : g->locksteps) ls->predicted = false;
  HIPCHK(hipMemcpyAsync(c->off_dev, moff.data(), moff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, g->stream));
  HIPCHK(hipMemcpyAsync(c->mcnt_dev, mcnt.data(), mcnt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, g->stream));
  HIPCHK(hipMemcpyAsync(c->short_dev, short_buf, (size_t)count * 24 * m, hipMemcpyHostToDevice, g->stream));
  HIPCHK(hipMemsetAsync(g->banks + (size_t)first * t.bank_bytes, 0, (size_t)count * t.bank_bytes, g->stream));
  GmxCkptArgs a;
  memset(&a, 0, sizeof a);
  a.topo = g->topo_dev;
  a.long_buf = (uint32_t*)c->stage.dev;
  CkptHipLink link{g->stream, c->stage.dev, nullptr};
  return ckpt_import_slices(link, plan, long_off, long_buf, c->stage, [&](size_t, int i0, int n) -> int {
    uint32_t most = 0;
    for (size_t q = 0; q < (size_t)n * m; ++q) most = std::max(most, mcnt[(size_t)i0 * m + q]);
    a.banks = g->banks + (size_t)(first + i0) * t.bank_bytes;
    a.n_streams = n;
    a.mixer_cnt = c->mcnt_dev + (size_t)i0 * m;
    a.mixer_off = c->off_dev + (size_t)i0 * m;
    a.short_buf = c->short_dev + (size_t)i0 * 6 * m;
    HIPCHK(gmx_launch_ckpt_scatter(&a, t.m, std::min(std::max((most + 3u) / 4u, 1u), 1024u), g->stream));
    return GMX_OK;
  });
}
