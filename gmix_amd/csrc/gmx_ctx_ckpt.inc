// gmx_ctx_ckpt.inc -- gmx_ctx_group_export / _import and gmx_ctx_group_blackboard_get / _set: the checkpoint of streams
// [first, first + count) of a context bank in one call.  Included by gmx_capi.cpp behind gmx_ckpt.inc and gmx_ctx.inc;
// kernels in gmx_ctx_ckpt.hip.  The per-stream calls of gmx_ctx.inc keep their own host code (but for
// ctx_validate_section, which both imports call); their kernels share the walk of gmx_ckpt_walk.h with these.
//
// Staging is gmx_ckpt_stage.h's, through gmx_ckpt.inc's allocations and link, which counts its waits and transfers
// in cb->gck_ops as GCK counts the calls made here.  A stock stream's sections approach its 201 MB of tables once
// they are dense: an image of a whole group would not fit beside the banks.  The buffers grow only and stay with the
// bank (freed by gmx_ctx_destroy): a bank that is checkpointed every generation allocates at its first checkpoint.
//
// Round trips of a call -- launches, transfers and waits, counted in cb->gck_ops (gmx_debug_ctx_group_ops); they
// depend on the number of slices, never on `count`:
//   export   drain . count launch . ONE D2H of {counts [count][chunks], hash states [count][16]} . wait . host scan
//            (a sizing call ends here: 4) . ONE H2D of the scan's results . per slice: pack launch . D2H of the slice's
//            image . wait                                                                      (5 + 3 x slices)
//   import   host validation . drain . ONE H2D of the tables' offsets and counts . zero launch . per slice: wait (the
//            device buffer is free) . H2D of the slice's image . scatter launch . then one wait       (4 + 3 x slices)
//   boards   get: drain . gather launch . ONE D2H . wait (4).  set: host validation . drain . ONE H2D . scatter launch .
//            wait (4)
// A bank without hash variables: export and import launch and copy nothing (0).  Not counted: growing a staging buffer
// and the bank's chunk list going to the device, which happen at a bank's first checkpoint (of that size).
// The scan is on the host: count x chunks additions (3 087 chunks a stream for the stock bank), and the host needs its
// totals anyway -- off[], var_off[] and the slices.

extern "C" {
hipError_t gmx_launch_ctx_gck_count(const GmxCtxGckArgs* a, hipStream_t stream);
hipError_t gmx_launch_ctx_gck_pack(const GmxCtxGckArgs* a, hipStream_t stream);
hipError_t gmx_launch_ctx_gck_zero(const GmxCtxGckArgs* a, int n_hash, hipStream_t stream);
hipError_t gmx_launch_ctx_gck_scatter(const GmxCtxGckArgs* a, int n_hash, hipStream_t stream);
hipError_t gmx_launch_ctx_gck_board_gather(const GmxCtxGckArgs* a, hipStream_t stream);
hipError_t gmx_launch_ctx_gck_board_scatter(const GmxCtxGckArgs* a, hipStream_t stream);
}

static_assert(sizeof(GmxCtxGckBoard) == sizeof(gmx_ctx_blackboard) &&
                  offsetof(GmxCtxGckBoard, rotating_history) == offsetof(gmx_ctx_blackboard, rotating_history) &&
                  offsetof(GmxCtxGckBoard, values) == offsetof(gmx_ctx_blackboard, values),
              "the board kernels' record is gmx_ctx_blackboard");

struct GmxCtxGckState {
  uint8_t* back_dev = nullptr;   // count's results: counts [streams][chunks], hash states [streams][16]
  uint8_t* meta_dev = nullptr;   // the scan's results: tables [streams][h], chunk bases [streams][chunks]
  uint8_t* board_dev = nullptr;  // [streams] gmx_ctx_blackboard
  CkptStaging img;               // one slice's sections
  size_t back_cap = 0, meta_cap = 0, board_cap = 0;  // bytes
};

static void ctx_gck_free(gmx_ctx* cb) {
  GmxCtxGckState* c = cb->gck;
  if (!c) return;
  void* dev[] = {c->back_dev, c->meta_dev, c->board_dev};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  ckpt_stage_free(c->img);
  delete c;
  cb->gck = nullptr;
}
static int ctx_gck_state(gmx_ctx* cb, GmxCtxGckState** out) {
  if (!cb->gck && !(cb->gck = new (std::nothrow) GmxCtxGckState())) return GMX_ERR_NOMEM;
  *out = cb->gck;
  return GMX_OK;
}

#define GCK(call)          \
  do {                     \
    ++cb->gck_ops;         \
    HIPCHK(call);          \
  } while (0)

static bool ctx_gck_window_ok(const gmx_ctx* cb, int first, int count) {
  // (the last condition: the kernels' flat grids -- out of reach of any bank that fits a device's memory)
  return cb && first >= 0 && count >= 1 && first <= cb->S && count <= cb->S - first &&
         (uint64_t)count * std::max<uint64_t>(cb->chunks.size(), (uint64_t)GMX_CTX_MAX_HASH * 1024u) <= 0x7fffffffull;
}
// blocks per (stream, table) of a zero / scatter launch: 256 lanes, up to 1 024 blocks
static uint32_t ctx_gck_blocks(uint64_t items) { return (uint32_t)std::min<uint64_t>(items / 256u + 1u, 1024u); }

extern "C" int gmx_debug_ctx_group_ops(const gmx_ctx* cb) { return cb ? cb->gck_ops : GMX_ERR_INVALID; }

// The slices of the window; tb[].off becomes an offset inside the table's slice.
static bool ctx_gck_plan(const size_t* off, int count, size_t H, GmxCtxGckTable* tb, CkptPlan& plan) {
  if (!ckpt_plan(off, count, ckpt_stage_cap(), plan)) return false;
  for (int i = 0; i < count; ++i)
    for (size_t j = 0; j < H; ++j) tb[(size_t)i * H + j].off += plan.shift[i];
  return true;
}

extern "C" int gmx_ctx_group_export(gmx_ctx* cb, int first, int count, void* buf, size_t cap, size_t* off,
                                    size_t* var_off) {
  if (!ctx_gck_window_ok(cb, first, count) || !off) return GMX_ERR_INVALID;
  const GmxCtxDev& d = cb->dev;
  const size_t H = (size_t)d.h, C = cb->chunks.size(), n = (size_t)count;
  cb->gck_ops = 0;
  HIPCHK(hipSetDevice(cb->device));
  {
    int rcs = ctx_settle(cb);
    if (rcs) return rcs;
  }
  if (H == 0) {  // every section is empty: nothing to read
    std::fill(off, off + n + 1, (size_t)0);
    if (var_off) std::fill(var_off, var_off + n, (size_t)0);
    return GMX_OK;
  }
  GCK(hipStreamSynchronize(cb->stream));  // (drains the bank's stream, as gmx_ctx_export does)
  int rc = ctx_ckpt_ready(cb);
  if (rc) return rc;
  GmxCtxGckState* c = nullptr;
  if ((rc = ctx_gck_state(cb, &c))) return rc;
  // ---- count; counts and hash states come back in one transfer
  const size_t cnt_bytes = round_up64(n * C * 4, 16), st_bytes = n * GMX_CTX_MAX_HASH * sizeof(GmxCtxHashState);
  const size_t tb_bytes = n * H * sizeof(GmxCtxGckTable);
  std::vector<uint8_t> back, meta;
  CkptPlan plan;
  try {
    back.resize(cnt_bytes + st_bytes);
    meta.assign(tb_bytes + n * C * 4, 0);
  } catch (const std::bad_alloc&) {
    return GMX_ERR_NOMEM;
  }
  if ((rc = ckpt_grow_dev(c->back_dev, c->back_cap, back.size()))) return rc;
  GmxCtxGckArgs a;
  memset(&a, 0, sizeof a);
  a.banks = cb->banks + (size_t)first * d.bank_bytes;
  a.dev = cb->dev_d;
  a.chunks = cb->chunks_d;
  a.n_chunks = (uint32_t)C;
  a.n_streams = (uint32_t)count;
  a.chunk_cnt = (uint32_t*)c->back_dev;
  a.states = (GmxCtxHashState*)(c->back_dev + cnt_bytes);
  GCK(gmx_launch_ctx_gck_count(&a, cb->stream));
  GCK(hipMemcpyAsync(back.data(), c->back_dev, back.size(), hipMemcpyDeviceToHost, cb->stream));
  GCK(hipStreamSynchronize(cb->stream));
  const uint32_t* const cc = (const uint32_t*)back.data();
  // ---- the scan: per (stream, table) the count, the branch and the offset; per chunk its first pair
  GmxCtxGckTable* const tb = (GmxCtxGckTable*)meta.data();
  uint32_t* const base = (uint32_t*)(meta.data() + tb_bytes);
  off[0] = 0;
  for (size_t i = 0; i < n; ++i) {
    uint32_t cnt[GMX_CTX_MAX_HASH] = {};
    for (size_t q = 0; q < C; ++q) {
      base[i * C + q] = cnt[cb->chunks[q].hash];
      cnt[cb->chunks[q].hash] += cc[i * C + q];
    }
    uint64_t pos = 0;  // inside the stream's section
    for (size_t j = 0; j < H; ++j) {
      GmxCtxGckTable& t = tb[i * H + j];
      t.off = pos;
      t.cnt = cnt[j];
      t.dense = ctx_is_dense(cnt[j], d.hash[j].table_size) ? 1u : 0u;
      if (var_off) var_off[i * (H + 1) + j] = (size_t)pos;
      pos += 4 + (t.dense ? 4ull * d.hash[j].table_size : 8ull * cnt[j]) + 12;
    }
    if (var_off) var_off[i * (H + 1) + H] = (size_t)pos;
    off[i + 1] = off[i] + (size_t)pos;
  }
  if (!buf) return GMX_OK;  // sizing only
  if (cap < off[count]) return GMX_ERR_INVALID;
  // ---- pack, slice by slice
  if (!ctx_gck_plan(off, count, H, tb, plan)) return GMX_ERR_NOMEM;
  if ((rc = ckpt_grow_dev(c->meta_dev, c->meta_cap, meta.size()))) return rc;
  if ((rc = ckpt_stage_grow(c->img, plan))) return rc;
  GCK(hipMemcpyAsync(c->meta_dev, meta.data(), meta.size(), hipMemcpyHostToDevice, cb->stream));
  a.image = c->img.dev;
  CkptHipLink link{cb->stream, c->img.dev, &cb->gck_ops};
  // (`meta` is pageable: read by the first slice's wait)
  return ckpt_export_slices(link, plan, off, buf, c->img, [&](size_t, int s0, int ns) -> int {
    const size_t i0 = (size_t)s0;
    a.banks = cb->banks + ((size_t)first + i0) * d.bank_bytes;
    a.n_streams = (uint32_t)ns;
    a.chunk_cnt = (uint32_t*)c->back_dev + i0 * C;
    a.tb = (const GmxCtxGckTable*)c->meta_dev + i0 * H;
    a.chunk_base = (const uint32_t*)(c->meta_dev + tb_bytes) + i0 * C;
    GCK(gmx_launch_ctx_gck_pack(&a, cb->stream));
    return GMX_OK;
  });
}

extern "C" int gmx_ctx_group_import(gmx_ctx* cb, int first, int count, const void* buf, const size_t* off) {
  if (!ctx_gck_window_ok(cb, first, count) || !off) return GMX_ERR_INVALID;
  for (int i = 0; i < count; ++i)
    if (off[i + 1] < off[i]) return GMX_ERR_INVALID;
  if (!buf && off[count] != off[0]) return GMX_ERR_INVALID;
  const GmxCtxDev& d = cb->dev;
  const size_t H = (size_t)d.h, n = (size_t)count;
  const uint8_t* const lb = (const uint8_t*)buf;
  cb->gck_ops = 0;
  // ---- every section is checked before any bank is touched
  std::vector<GmxCtxGckTable> tb;
  CkptPlan plan;
  try {
    tb.resize(n * H + 1);
  } catch (const std::bad_alloc&) {
    return GMX_ERR_NOMEM;
  }
  uint64_t most = 0, room = 0;  // pairs, or entries of a dense table, of the call's largest table; its largest sparse table
  for (size_t i = 0; i < n; ++i) {
    GmxCtxSection sec;
    const uint8_t* const sp = lb ? lb + off[i] : nullptr;
    int rcv = ctx_validate_section(d, sp, off[i + 1] - off[i], &sec);
    if (rcv) return rcv;
    for (size_t j = 0; j < H; ++j) {
      GmxCtxGckTable& t = tb[i * H + j];
      t.off = (uint64_t)(sec.body[j] - sp) - 4;
      t.cnt = sec.cnt[j];
      t.dense = sec.dense[j];
      most = std::max<uint64_t>(most, t.dense ? d.hash[j].table_size : t.cnt);
      if (!t.dense) room = std::max<uint64_t>(room, d.hash[j].table_size);
    }
  }
  if (H == 0) return GMX_OK;
  if (!ctx_gck_plan(off, count, H, tb.data(), plan)) return GMX_ERR_NOMEM;
  HIPCHK(hipSetDevice(cb->device));
  {
    int rcs = ctx_settle(cb);
    if (rcs) return rcs;
  }
  GmxCtxGckState* c = nullptr;
  int rc = ctx_gck_state(cb, &c);
  if (rc) return rc;
  const size_t tb_bytes = n * H * sizeof(GmxCtxGckTable);
  if ((rc = ckpt_grow_dev(c->meta_dev, c->meta_cap, tb_bytes))) return rc;
  if ((rc = ckpt_stage_grow(c->img, plan))) return rc;
  GCK(hipStreamSynchronize(cb->stream));  // (drains the bank's stream, as gmx_ctx_import does)
  // ---- from here the banks change
  GmxCtxGckArgs a;
  memset(&a, 0, sizeof a);
  a.banks = cb->banks + (size_t)first * d.bank_bytes;
  a.dev = cb->dev_d;
  a.n_streams = (uint32_t)count;
  a.tb = (const GmxCtxGckTable*)c->meta_dev;
  a.image = c->img.dev;
  GCK(hipMemcpyAsync(c->meta_dev, tb.data(), tb_bytes, hipMemcpyHostToDevice, cb->stream));
  a.blocks = ctx_gck_blocks(room / 4);  // 16 bytes a lane
  GCK(gmx_launch_ctx_gck_zero(&a, d.h, cb->stream));
  a.blocks = ctx_gck_blocks(most);
  CkptHipLink link{cb->stream, c->img.dev, &cb->gck_ops};
  // (`tb` is pageable: read by the first slice's wait)
  return ckpt_import_slices(link, plan, off, lb, c->img, [&](size_t, int s0, int ns) -> int {
    a.banks = cb->banks + ((size_t)first + (size_t)s0) * d.bank_bytes;
    a.n_streams = (uint32_t)ns;
    a.tb = (const GmxCtxGckTable*)c->meta_dev + (size_t)s0 * H;
    GCK(gmx_launch_ctx_gck_scatter(&a, d.h, cb->stream));
    return GMX_OK;
  });
}

// ---- the blackboards -------------------------------------------------------------------------------
static int ctx_gck_boards(gmx_ctx* cb, int count, GmxCtxGckState** c) {
  int rc = ctx_gck_state(cb, c);
  if (rc) return rc;
  return ckpt_grow_dev((*c)->board_dev, (*c)->board_cap, (size_t)count * sizeof(gmx_ctx_blackboard));
}

extern "C" int gmx_ctx_group_blackboard_get(gmx_ctx* cb, int first, int count, gmx_ctx_blackboard* out) {
  if (!ctx_gck_window_ok(cb, first, count) || !out) return GMX_ERR_INVALID;
  for (int i = 0; i < count; ++i)
    if (cb->outstanding[first + i]) return GMX_ERR_STATE;
  cb->gck_ops = 0;
  HIPCHK(hipSetDevice(cb->device));
  {
    int rcs = ctx_settle(cb);
    if (rcs) return rcs;
  }
  GmxCtxGckState* c = nullptr;
  int rc = ctx_gck_boards(cb, count, &c);
  if (rc) return rc;
  GCK(hipStreamSynchronize(cb->stream));
  GmxCtxGckArgs a;
  memset(&a, 0, sizeof a);
  a.banks = cb->banks + (size_t)first * cb->dev.bank_bytes;
  a.dev = cb->dev_d;
  a.n_streams = (uint32_t)count;
  a.boards = (GmxCtxGckBoard*)c->board_dev;
  GCK(gmx_launch_ctx_gck_board_gather(&a, cb->stream));
  GCK(hipMemcpyAsync(out, c->board_dev, (size_t)count * sizeof(gmx_ctx_blackboard), hipMemcpyDeviceToHost,
                     cb->stream));
  GCK(hipStreamSynchronize(cb->stream));
  return GMX_OK;
}

extern "C" int gmx_ctx_group_blackboard_set(gmx_ctx* cb, int first, int count, const gmx_ctx_blackboard* in) {
  if (!ctx_gck_window_ok(cb, first, count) || !in) return GMX_ERR_INVALID;
  for (int i = 0; i < count; ++i) {  // gmx_ctx_blackboard_set's rules, for every board before any is written
    const gmx_ctx_blackboard& b = in[i];
    if (b.recent_bits < 1 || b.recent_bits > 255 || (b.new_bit != 0 && b.new_bit != 1) ||
        b.rotating_history_pos >= GMX_CTX_RING || (b.first_prediction && b.recent_bits != 1))
      return GMX_ERR_INVALID;
    for (int k = 0; k < 10; ++k)
      if (b.recent_bytes[k] != b.rotating_history[(b.rotating_history_pos + GMX_CTX_RING - k) % GMX_CTX_RING])
        return GMX_ERR_INVALID;
    if (b.last_byte != b.recent_bytes[0]) return GMX_ERR_INVALID;
  }
  cb->gck_ops = 0;
  HIPCHK(hipSetDevice(cb->device));
  {
    int rcs = GMX_OK;
    for (int s = first; s < first + count && !rcs; ++s) rcs = ctx_board_moves(cb, s);
    if (!rcs) rcs = ctx_settle(cb);
    if (rcs) return rcs;
  }
  GmxCtxGckState* c = nullptr;
  int rc = ctx_gck_boards(cb, count, &c);
  if (rc) return rc;
  GCK(hipStreamSynchronize(cb->stream));
  GmxCtxGckArgs a;
  memset(&a, 0, sizeof a);
  a.banks = cb->banks + (size_t)first * cb->dev.bank_bytes;
  a.dev = cb->dev_d;
  a.n_streams = (uint32_t)count;
  a.boards = (GmxCtxGckBoard*)c->board_dev;
  GCK(hipMemcpyAsync(c->board_dev, in, (size_t)count * sizeof(gmx_ctx_blackboard), hipMemcpyHostToDevice, cb->stream));
  GCK(gmx_launch_ctx_gck_board_scatter(&a, cb->stream));
  GCK(hipStreamSynchronize(cb->stream));
  for (int i = 0; i < count; ++i) cb->outstanding[first + i] = 0;
  cb->moved = true;
  return GMX_OK;
}
#undef GCK
