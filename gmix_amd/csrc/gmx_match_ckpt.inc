// gmx_match_ckpt.inc -- gmx_match_group_export / gmx_match_group_import: the checkpoint of streams
// [first, first + count) of a Match bank in one call.  Included by gmx_capi.cpp behind gmx_match.inc; kernels in
// gmx_match_ckpt.hip.  The per-stream calls of gmx_match.inc keep their own host code; their kernels share the walk
// of gmx_ckpt_walk.h with these (DESIGN 4.12 names the independent witnesses).  This bank keeps its per-call arena
// and is no user of gmx_ckpt_stage.h.
//
// The number of launches, transfers, synchronisations and allocations of a call does not depend on `count`
// (mb->gck_ops counts them: gmx_debug_match_group_ops):
//   export   drain . malloc A . count launch . ONE D2H of A = {counts [count][chunks], states [count]} . wait .
//            host scan . malloc B . ONE H2D of the scan's results . pack launch . history launch . ONE D2H of the image
//            . wait . free x 2                                                        (13; a sizing call: 6)
//   import   host validation . drain . malloc B . H2D of the image . H2D of the tables of offsets . zero launch .
//            scatter launch . restore launch . wait . free                                          (9)
// (The bank's chunk list goes to the device once, at the first checkpoint of any kind: match_ckpt_ready, not counted.)
// The scan is on the host: it is count x chunks additions (1 412 chunks a stream for the stock models, 1.4 MiB of
// counts at 256 streams), the host needs its totals anyway -- long_off[], and the size of the image before it can be
// allocated -- and the states that make the short sections ride in the same transfer.
//
// B = the image, laid out as the caller's buffer: nothing is cut in slices, so a call needs as much free device memory
// as its sections are long (GMX_ERR_NOMEM otherwise; the caller may then ask for fewer streams per call).  Both
// arenas live for one call: a bank that is checkpointed once a generation keeps no staging memory in between.

extern "C" {
hipError_t gmx_launch_match_gck_count(const GmxMatchGckArgs* a, hipStream_t stream);
hipError_t gmx_launch_match_gck_pack(const GmxMatchGckArgs* a, hipStream_t stream);
hipError_t gmx_launch_match_gck_history(const GmxMatchGckArgs* a, hipStream_t stream);
hipError_t gmx_launch_match_gck_restore(const GmxMatchGckArgs* a, hipStream_t stream);
hipError_t gmx_launch_match_gck_zero(const GmxMatchGckArgs* a, hipStream_t stream);
hipError_t gmx_launch_match_gck_scatter(const GmxMatchGckArgs* a, int n_models, hipStream_t stream);
}

// A call's device memory: freed on every way out.
struct GmxMatchGckArena {
  gmx_match* mb;
  uint8_t* p[2] = {nullptr, nullptr};
  explicit GmxMatchGckArena(gmx_match* m) : mb(m) {}
  ~GmxMatchGckArena() {
    for (uint8_t* q : p)
      if (q) {
        (void)hipFree(q);
        ++mb->gck_ops;
      }
  }
  int alloc(int i, size_t bytes) {
    ++mb->gck_ops;
    hipError_t e = hipMalloc((void**)&p[i], bytes ? bytes : 1);
    if (e == hipSuccess) return GMX_OK;
    p[i] = nullptr;
    int r = hip_fail(e, "hipMalloc(match group checkpoint)");
    return e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation ? GMX_ERR_NOMEM : r;
  }
};
#define GCK(call)          \
  do {                     \
    ++mb->gck_ops;         \
    HIPCHK(call);          \
  } while (0)

// blocks of a history / zero launch per stream: 16 bytes a lane and iteration, 1 024 blocks at the most
static uint32_t gck_blocks(uint64_t bytes) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(bytes / 4096u, 1u), 1024u);
}
static bool gck_args_ok(const gmx_match* mb, int first, int count, const size_t* long_off) {
  // (the last condition: the kernels' flat grids -- out of reach of any bank that fits a device's memory)
  return mb && long_off && first >= 0 && count >= 1 && first <= mb->S && count <= mb->S - first &&
         (uint64_t)count * std::max<uint64_t>(mb->chunks.size(), 8u * 1024u) <= 0x7fffffffull;
}

extern "C" int gmx_debug_match_group_ops(gmx_match* mb, uint64_t* ops) {
  if (!mb || !ops) return GMX_ERR_INVALID;
  *ops = mb->gck_ops;
  return GMX_OK;
}

extern "C" int gmx_match_group_export(gmx_match* mb, int first, int count, void* long_buf, size_t long_cap,
                                      size_t* long_off, void* short_buf) {
  if (!gck_args_ok(mb, first, count, long_off)) return GMX_ERR_INVALID;
  if ((long_buf == nullptr) != (short_buf == nullptr)) return GMX_ERR_INVALID;
  const GmxMatchDev& d = mb->dev;
  const size_t K = (size_t)d.k, C = mb->chunks.size(), n = (size_t)count;
  HIPCHK(hipSetDevice(mb->device));
  {
    int rcs = match_settle(mb);  // (hosted streams: no wave steps them, no learn is still noted; not counted)
    if (rcs) return rcs;
  }
  GCK(hipStreamSynchronize(mb->stream));  // (drains the bank's stream, as match_read_states does for gmx_match_export)
  int rc = match_ckpt_ready(mb);
  if (rc) return rc;
  // ---- count; counts and states come back in one transfer
  const size_t cnt_bytes = round_up64(n * C * 4, 16), st_bytes = n * sizeof(GmxMatchGckStates);
  std::vector<uint8_t> back, meta;
  try {
    back.resize(cnt_bytes + st_bytes);
  } catch (const std::bad_alloc&) {
    return GMX_ERR_NOMEM;
  }
  GmxMatchGckArena ar(mb);
  if ((rc = ar.alloc(0, cnt_bytes + st_bytes))) return rc;
  GmxMatchGckArgs a;
  memset(&a, 0, sizeof a);
  a.banks = mb->banks + (size_t)first * d.bank_bytes;
  a.hist = mb->hist + (size_t)first * d.hist_cap;
  a.dev = mb->dev_d;
  a.chunks = mb->chunks_d;
  a.n_chunks = (uint32_t)C;
  a.n_streams = (uint32_t)count;
  a.chunk_cnt = (uint32_t*)ar.p[0];
  a.states = (GmxMatchGckStates*)(ar.p[0] + cnt_bytes);
  GCK(gmx_launch_match_gck_count(&a, mb->stream));
  GCK(hipMemcpyAsync(back.data(), ar.p[0], back.size(), hipMemcpyDeviceToHost, mb->stream));
  GCK(hipStreamSynchronize(mb->stream));
  const uint32_t* const cc = (const uint32_t*)back.data();
  const GmxMatchGckStates* const states = (const GmxMatchGckStates*)(back.data() + cnt_bytes);
  // ---- the scan: per (stream, model) the count, the branch and the offset; per chunk its first record
  const size_t st_off = 0, md_off = n * sizeof(GmxMatchGckStream), base_off = md_off + n * K * sizeof(GmxMatchGckModel);
  try {
    meta.assign(base_off + n * C * 4, 0);
  } catch (const std::bad_alloc&) {
    return GMX_ERR_NOMEM;
  }
  GmxMatchGckStream* const st = (GmxMatchGckStream*)(meta.data() + st_off);
  GmxMatchGckModel* const md = (GmxMatchGckModel*)(meta.data() + md_off);
  uint32_t* const base = (uint32_t*)(meta.data() + base_off);
  uint64_t max_hs = 0;
  long_off[0] = 0;
  for (size_t i = 0; i < n; ++i) {
    uint32_t cnt[GMX_MATCH_MAX_MODELS] = {};
    for (size_t c = 0; c < C; ++c) {
      base[i * C + c] = cnt[mb->chunks[c].model];
      cnt[mb->chunks[c].model] += cc[i * C + c];
    }
    const uint64_t hs = states[i].s.hist_size;
    mb->hist_bound[first + i] = hs;
    max_hs = std::max(max_hs, hs);
    st[i].sec_off = long_off[i];
    st[i].hist_size = (uint32_t)hs;
    uint64_t pos = long_off[i] + 8 + hs;
    for (size_t j = 0; j < K; ++j) {
      GmxMatchGckModel& m = md[i * K + j];
      m.off = pos;
      m.cnt = cnt[j];
      m.dense = match_is_dense(cnt[j], d.m[j].table_size) ? 1 : 0;
      pos += 4 + (m.dense ? 5ull * d.m[j].table_size : 9ull * cnt[j]) + 2048;
    }
    long_off[i + 1] = (size_t)pos;
  }
  if (!long_buf) return GMX_OK;  // sizing only
  const size_t need = long_off[count];
  if (long_cap < need) return GMX_ERR_INVALID;
  // ---- assemble every section on the device, then one transfer
  const size_t img_bytes = round_up64(need, 16);
  if ((rc = ar.alloc(1, img_bytes + meta.size()))) return rc;
  uint8_t* const meta_d = ar.p[1] + img_bytes;
  a.image = ar.p[1];
  a.st = (const GmxMatchGckStream*)(meta_d + st_off);
  a.md = (const GmxMatchGckModel*)(meta_d + md_off);
  a.chunk_base = (const uint32_t*)(meta_d + base_off);
  a.blocks = gck_blocks(max_hs);
  GCK(hipMemcpyAsync(meta_d, meta.data(), meta.size(), hipMemcpyHostToDevice, mb->stream));
  GCK(gmx_launch_match_gck_pack(&a, mb->stream));
  GCK(gmx_launch_match_gck_history(&a, mb->stream));
  GCK(hipMemcpyAsync(long_buf, ar.p[1], need, hipMemcpyDeviceToHost, mb->stream));
  GCK(hipStreamSynchronize(mb->stream));  // (`meta` is pageable: it lives until here)
  // ---- the short sections: Match::WriteToDisk x K (match.cpp:111-116)
  uint8_t* o = (uint8_t*)short_buf;
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < K; ++j, o += 11) {
      const GmxMatchModelState& m = states[i].m[j];
      const uint64_t cm = m.cur_match;
      memcpy(o, &cm, 8);
      o[8] = m.cur_byte;
      o[9] = m.bit_pos;
      o[10] = m.match_length;
    }
  return GMX_OK;
}

extern "C" int gmx_match_group_import(gmx_match* mb, int first, int count, const void* long_buf,
                                      const size_t* long_off, const void* short_buf) {
  if (!gck_args_ok(mb, first, count, long_off) || !long_buf || !short_buf) return GMX_ERR_INVALID;
  for (int i = 0; i < count; ++i)
    if (long_off[i + 1] < long_off[i]) return GMX_ERR_INVALID;
  const GmxMatchDev& d = mb->dev;
  const size_t K = (size_t)d.k, n = (size_t)count;
  const uint8_t* const lb = (const uint8_t*)long_buf;
  const uint8_t* const sb = (const uint8_t*)short_buf;
  // ---- every section is checked before any bank is touched
  const size_t md_off = n * sizeof(GmxMatchGckStream);
  std::vector<uint8_t> meta;
  try {
    meta.assign(md_off + n * K * sizeof(GmxMatchGckModel), 0);
  } catch (const std::bad_alloc&) {
    return GMX_ERR_NOMEM;
  }
  GmxMatchGckStream* const st = (GmxMatchGckStream*)meta.data();
  GmxMatchGckModel* const md = (GmxMatchGckModel*)(meta.data() + md_off);
  uint64_t max_hs = 0;
  uint32_t most = 0;  // records, or entries of a dense model, of the call's largest model
  for (size_t i = 0; i < n; ++i) {
    GmxMatchSection sec;
    const uint8_t* const sp = sb + i * 11 * K;
    int rcv = match_validate_section(d, lb + long_off[i], long_off[i + 1] - long_off[i], sp, 11 * K, &sec);
    if (rcv) return rcv;
    st[i].sec_off = long_off[i] - long_off[0];
    st[i].hist_size = (uint32_t)sec.hs;
    max_hs = std::max(max_hs, sec.hs);
    for (size_t j = 0; j < K; ++j) {
      GmxMatchGckModel& m = md[i * K + j];
      m.off = st[i].sec_off + sec.moff[j] - 4;
      m.cnt = sec.cnt[j];
      m.dense = sec.dense[j];
      m.cur_match = (uint32_t)sec.cms[j];
      m.cur_byte = sp[11 * j + 8];
      m.bit_pos = sp[11 * j + 9];
      m.match_length = sp[11 * j + 10];
      most = std::max(most, m.dense ? d.m[j].table_size : m.cnt);
    }
  }
  const size_t bytes = long_off[count] - long_off[0], img_bytes = round_up64(bytes, 16);
  HIPCHK(hipSetDevice(mb->device));
  {
    int rcs = match_settle(mb);
    if (rcs) return rcs;
  }
  GCK(hipStreamSynchronize(mb->stream));  // (drains the bank's stream, as gmx_match_import does)
  int rc = match_ckpt_ready(mb);
  if (rc) return rc;
  GmxMatchGckArena ar(mb);
  if ((rc = ar.alloc(1, img_bytes + meta.size()))) return rc;
  uint8_t* const meta_d = ar.p[1] + img_bytes;
  GmxMatchGckArgs a;
  memset(&a, 0, sizeof a);
  a.banks = mb->banks + (size_t)first * d.bank_bytes;
  a.hist = mb->hist + (size_t)first * d.hist_cap;
  a.dev = mb->dev_d;
  a.n_streams = (uint32_t)count;
  a.image = ar.p[1];
  a.st = (const GmxMatchGckStream*)meta_d;
  a.md = (const GmxMatchGckModel*)(meta_d + md_off);
  GCK(hipMemcpyAsync(ar.p[1], lb + long_off[0], bytes, hipMemcpyHostToDevice, mb->stream));
  GCK(hipMemcpyAsync(meta_d, meta.data(), meta.size(), hipMemcpyHostToDevice, mb->stream));
  // ---- from here the banks change
  for (int i = 0; i < count; ++i) {
    mb->fwd_done[first + i] = 0;
    mb->hist_bound[first + i] = st[i].hist_size;
  }
  a.blocks = gck_blocks(d.tab_bytes);
  GCK(gmx_launch_match_gck_zero(&a, mb->stream));
  a.blocks = std::min(most / 256u + 1u, 1024u);
  GCK(gmx_launch_match_gck_scatter(&a, d.k, mb->stream));
  a.blocks = gck_blocks(max_hs);
  GCK(gmx_launch_match_gck_restore(&a, mb->stream));
  GCK(hipStreamSynchronize(mb->stream));  // (`meta` and the caller's buffer are pageable: read by now)
  return GMX_OK;
}
#undef GCK
