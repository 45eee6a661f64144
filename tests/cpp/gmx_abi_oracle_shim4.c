/* gmx_abi_oracle_shim4.c -- TEST INFRASTRUCTURE, CPU only (see gmx_abi_oracle_shim.c): the gmx_ctx_* entry points
 * gmx_model_adapter.h calls for gmx::GpuCtxBank, answered by tests/helpers/ctx_ref.c (pinned to the reference by
 * tests/golden/ctx_*.npz, tests/test_ctx_ref.py), so that the host logic of the *_dev drop-in can be run inside the real
 * reference without a GPU (oracle/_ref/shim/*_dev*_shim, tests/test_dev_cpu.py).  Never shipped, never a fallback.
 *
 * The state rules of include/gmxmix.h that the adapter can break are kept: a second forward without a learn, and a run,
 * a blackboard_get or a copy from a stream that stands between a forward and its learn, return GMX_ERR_STATE.
 *
 * Run-ahead: gmx_ctx_run_ragged writes the routed context columns, bit_contexts and bits into the other stand-ins'
 * batches through their public accessors.  Those have no max_bits accessor for the Indirect batch, so every target
 * must have the context batch's max_bits (MixerPool makes them so); anything else is GMX_ERR_INVALID.
 *
 * Lock step: the *_dev*_shim binaries are linked with -Wl,--wrap= for gmx_chainstep_create / _destroy / _step /
 * _launch like the *_full*_shim ones, but gmx_abi_oracle_shim3.c is compiled a second time with its wrappers of
 * _destroy / _step / _launch renamed on the command line (dropin/Makefile: abi_shim3_chained.o); the wrappers here own
 * the names and run the context stage -- the step's learn and one record per predicting stream, into the object's own
 * records -- in front of the Match stage, which runs in front of gmx_abi_oracle_shim2.c's step. */
#include "../helpers/ctx_ref.c"

#include <pthread.h>

#include "../../include/gmxmix.h"

struct gmx_ctx {
  int S, V, H;
  gmx_ctx_desc d[64];
  cref** st;
  uint8_t* fwd; /* [S] a forward (or a lock-step Predict) waits for its learn */
};
#define CST(cb, s) ((cb) && (s) >= 0 && (s) < (cb)->S ? (cb)->st[s] : 0)

static int desc_ok(const gmx_ctx_desc* d) {
  switch (d->kind) {
    case GMX_CTX_ZERO:
    case GMX_CTX_BIT_CONTEXT: return 1;
    case GMX_CTX_RECENT_BYTE:
    case GMX_CTX_BYTE_PLUS_RECENT: return d->index >= 0 && d->index <= 9;
    case GMX_CTX_INTERVAL: return d->num_bits >= 1 && d->num_bits <= 31;
    case GMX_CTX_SKIP:
      if (d->n_bytes < 1 || d->n_bytes > 8) return 0;
      for (int i = 0; i < d->n_bytes; ++i)
        if (d->bytes_to_use[i] > 15) return 0;
      return 1;
    case GMX_CTX_INDIRECT_HASH:
      return d->outer_order >= 1 && d->outer_order <= 4 && d->inner_order >= 1 && d->inner_order <= 4 && d->table_size >= 1;
  }
  return 0;
}

int gmx_ctx_create(gmx_ctx** out, const gmx_ctx_desc* descs, int n_vars, int n_streams, int device) {
  (void)device;
  if (!out || !descs || n_vars < 1 || n_vars > 64 || n_streams < 1) return GMX_ERR_INVALID;
  int H = 0;
  for (int v = 0; v < n_vars; ++v) {
    if (!desc_ok(&descs[v])) return GMX_ERR_INVALID;
    H += descs[v].kind == GMX_CTX_INDIRECT_HASH;
  }
  if (H > 16) return GMX_ERR_INVALID;
  gmx_ctx* cb = (gmx_ctx*)calloc(1, sizeof *cb);
  cb->S = n_streams;
  cb->V = n_vars;
  cb->H = H;
  memcpy(cb->d, descs, (size_t)n_vars * sizeof *descs);
  cb->st = (cref**)calloc((size_t)n_streams, sizeof(cref*));
  cb->fwd = (uint8_t*)calloc((size_t)n_streams, 1);
  for (int s = 0; s < n_streams; ++s) cb->st[s] = cref_create(n_vars, (const cref_desc*)descs);
  *out = cb;
  return GMX_OK;
}

static void note_forget_bank(gmx_ctx* cb);
void gmx_ctx_destroy(gmx_ctx* cb) {
  if (!cb) return;
  note_forget_bank(cb);
  for (int s = 0; s < cb->S; ++s) cref_destroy(cb->st[s]);
  free(cb->st);
  free(cb->fwd);
  free(cb);
}
int gmx_ctx_n_streams(const gmx_ctx* cb) { return cb ? cb->S : GMX_ERR_INVALID; }
int gmx_ctx_n_vars(const gmx_ctx* cb) { return cb ? cb->V : GMX_ERR_INVALID; }

int gmx_ctx_learn(gmx_ctx* cb, int stream, int bit) {
  cref* c = CST(cb, stream);
  if (!c || (bit != 0 && bit != 1)) return GMX_ERR_INVALID;
  c->b.new_bit = bit;
  cb->fwd[stream] = 0;
  return GMX_OK;
}
int gmx_ctx_forward(gmx_ctx* cb, int stream, uint32_t* values, uint32_t* bit_context) {
  cref* c = CST(cb, stream);
  if (!c) return GMX_ERR_INVALID;
  if (cb->fwd[stream]) return GMX_ERR_STATE;
  step(c, c->b.new_bit); /* one record; the board's new_bit stays what the learn made it */
  cb->fwd[stream] = 1;
  if (values) memcpy(values, c->b.values, (size_t)cb->V * 4);
  if (bit_context) *bit_context = (uint32_t)c->b.recent_bits - 1;
  return GMX_OK;
}

int gmx_ctx_blackboard_get(gmx_ctx* cb, int stream, gmx_ctx_blackboard* out) {
  cref* c = CST(cb, stream);
  if (!c || !out) return GMX_ERR_INVALID;
  if (cb->fwd[stream]) return GMX_ERR_STATE;
  memcpy(out, &c->b, sizeof *out);
  return GMX_OK;
}
int gmx_ctx_blackboard_set(gmx_ctx* cb, int stream, const gmx_ctx_blackboard* in) {
  cref* c = CST(cb, stream);
  if (!c || !in) return GMX_ERR_INVALID;
  if (in->recent_bits < 1 || in->recent_bits > 255 || in->rotating_history_pos >= 1000u || (in->new_bit != 0 && in->new_bit != 1))
    return GMX_ERR_INVALID;
  if (in->first_prediction && in->recent_bits != 1) return GMX_ERR_INVALID;
  cref_board b;
  memcpy(&b, in, sizeof b);
  if (b.last_byte != recent_byte(&b, 0)) return GMX_ERR_INVALID;
  for (int i = 0; i < 10; ++i)
    if (b.recent_bytes[i] != recent_byte(&b, i)) return GMX_ERR_INVALID;
  c->b = b;
  cb->fwd[stream] = 0;
  return GMX_OK;
}

int gmx_ctx_export(gmx_ctx* cb, int stream, void* buf, size_t* bytes, size_t* offsets) {
  cref* c = CST(cb, stream);
  if (!c || !bytes) return GMX_ERR_INVALID;
  uint64_t off[17];
  const size_t need = (size_t)cref_export(c, 0, off);
  const int fits = !buf || *bytes >= need;
  *bytes = need;
  if (offsets)
    for (int h = 0; h <= cb->H; ++h) offsets[h] = (size_t)off[h];
  if (!buf) return GMX_OK;
  if (!fits) return GMX_ERR_INVALID;
  cref_export(c, (uint8_t*)buf, 0);
  return GMX_OK;
}
int gmx_ctx_import(gmx_ctx* cb, int stream, const void* buf, size_t bytes) {
  cref* c = CST(cb, stream);
  if (!c || (!buf && bytes)) return GMX_ERR_INVALID;
  /* validated on a scratch object first: a bad section leaves the bank as it was */
  cref* fresh = cref_create(cb->V, (const cref_desc*)cb->d);
  if (cref_import(fresh, (const uint8_t*)buf, bytes)) {
    cref_destroy(fresh);
    return GMX_ERR_FORMAT;
  }
  fresh->b = c->b; /* (the blackboard is left alone) */
  cref_destroy(c);
  cb->st[stream] = fresh;
  return GMX_OK;
}
int gmx_ctx_copy(gmx_ctx* dst, int ds, gmx_ctx* src, int ss) {
  cref *d = CST(dst, ds), *s = CST(src, ss);
  if (!d || !s || dst->V != src->V || memcmp(dst->d, src->d, (size_t)dst->V * sizeof(gmx_ctx_desc))) return GMX_ERR_INVALID;
  if (src->fwd[ss]) return GMX_ERR_STATE;
  if (d == s) return GMX_OK;
  for (int v = 0; v < dst->V; ++v) {
    if (dst->d[v].kind == GMX_CTX_INDIRECT_HASH) memcpy(d->table[v], s->table[v], 4ull * dst->d[v].table_size);
    d->outer_context[v] = s->outer_context[v];
    d->outer_hash[v] = s->outer_hash[v];
  }
  d->b = s->b;
  dst->fwd[ds] = 0;
  return GMX_OK;
}
int gmx_ctx_memory_usage(gmx_ctx* cb, int var, uint64_t* bytes) {
  if (!cb || var < 0 || var >= cb->V || !bytes) return GMX_ERR_INVALID;
  const gmx_ctx_desc* d = &cb->d[var];
  *bytes = d->kind == GMX_CTX_INDIRECT_HASH ? 36 + 4ull * d->table_size
           : d->kind == GMX_CTX_INTERVAL    ? 256 * 4 + 8 + 4
           : d->kind == GMX_CTX_SKIP        ? 4ull * (uint64_t)d->n_bytes + 4
                                            : 0;
  return GMX_OK;
}

/* ---- the batched surface the run-ahead compressor uses (MixerPool::Lead) ---- */
struct gmx_ctx_batch {
  gmx_ctx* cb;
  uint64_t T;
  uint8_t* bits;
  uint32_t* values; /* NULL without GMX_CTX_BATCH_VALUES */
};
int gmx_ctx_batch_create(gmx_ctx_batch** out, gmx_ctx* cb, uint64_t max_bits, unsigned flags) {
  if (!out || !cb || !max_bits || max_bits > (1ull << 30)) return GMX_ERR_INVALID;
  gmx_ctx_batch* b = (gmx_ctx_batch*)calloc(1, sizeof *b);
  b->cb = cb;
  b->T = max_bits;
  b->bits = (uint8_t*)calloc((size_t)cb->S * max_bits, 1);
  if (flags & GMX_CTX_BATCH_VALUES) b->values = (uint32_t*)calloc((size_t)cb->S * max_bits * cb->V, 4);
  *out = b;
  return GMX_OK;
}
void gmx_ctx_batch_destroy(gmx_ctx_batch* b) {
  if (!b) return;
  free(b->bits);
  free(b->values);
  free(b);
}
uint64_t gmx_ctx_batch_max_bits(const gmx_ctx_batch* b) { return b ? b->T : 0; }
uint8_t* gmx_ctx_batch_bits(gmx_ctx_batch* b) { return b->bits; }
const uint32_t* gmx_ctx_batch_values(gmx_ctx_batch* b) { return b->values; }
int gmx_ctx_batch_upload(gmx_ctx_batch* b, uint64_t n) { return (b && n <= b->T) ? GMX_OK : GMX_ERR_INVALID; }
int gmx_ctx_batch_download(gmx_ctx_batch* b, uint64_t n) { return (b && n <= b->T) ? GMX_OK : GMX_ERR_INVALID; }
int gmx_ctx_batch_wait(gmx_ctx_batch* b) { return b ? GMX_OK : GMX_ERR_INVALID; }

/* the other stand-ins' batches (gmx_abi_oracle_shim.c, _shim2.c, _shim3.c) */
extern uint32_t* gmx_batch_contexts(gmx_batch* b);
extern uint64_t gmx_batch_max_bits(const gmx_batch* b);
extern int gmx_shim_batch_m(const gmx_batch* b);
extern uint32_t* gmx_ind_batch_contexts(gmx_ind_batch* b);
extern uint32_t* gmx_ind_batch_bit_contexts(gmx_ind_batch* b);
extern uint8_t* gmx_ind_batch_bits(gmx_ind_batch* b);
extern int gmx_ind_batch_upload(gmx_ind_batch* b, uint64_t n);
extern uint32_t* gmx_match_batch_contexts(gmx_match_batch* b);
extern uint32_t* gmx_match_batch_bit_contexts(gmx_match_batch* b);
extern uint8_t* gmx_match_batch_bits(gmx_match_batch* b);
extern uint64_t gmx_match_batch_max_bits(const gmx_match_batch* b);

static int route_ok(const int32_t* r, int n, int V) {
  if (!r || n < 1 || n > 128) return 0;
  for (int i = 0; i < n; ++i)
    if (r[i] < -1 || r[i] >= V) return 0;
  return 1;
}

int gmx_ctx_run_ragged(gmx_ctx* cb, gmx_ctx_batch* b, const uint64_t* n_bits, const gmx_ctx_targets* tg) {
  if (!cb || !b || b->cb != cb || !n_bits) return GMX_ERR_INVALID;
  const int V = cb->V;
  if (tg) {
    if (tg->mixers && (!route_ok(tg->mixer_route, tg->n_mixer_route, V) || tg->n_mixer_route != gmx_shim_batch_m(tg->mixers) ||
                       gmx_batch_max_bits(tg->mixers) != b->T))
      return GMX_ERR_INVALID;
    if (tg->indirect && (!route_ok(tg->ind_route, tg->n_ind_route, V) || gmx_ind_batch_upload(tg->indirect, b->T) != GMX_OK ||
                         gmx_ind_batch_upload(tg->indirect, b->T + 1) == GMX_OK))
      return GMX_ERR_INVALID;
    if (tg->match && (!route_ok(tg->match_route, tg->n_match_route, V) || gmx_match_batch_max_bits(tg->match) != b->T))
      return GMX_ERR_INVALID;
  }
  for (int s = 0; s < cb->S; ++s) {
    if (n_bits[s] > b->T) return GMX_ERR_INVALID;
    if (n_bits[s] && cb->fwd[s]) return GMX_ERR_STATE;
  }
  for (int s = 0; s < cb->S; ++s) {
    cref* c = cb->st[s];
    for (uint64_t t = 0; t < n_bits[s]; ++t) {
      const size_t r = (size_t)s * b->T + t;
      const int bit = b->bits[r] ? 1 : 0;
      step(c, bit);
      const uint32_t* val = c->b.values;
      const uint32_t bc = (uint32_t)c->b.recent_bits - 1;
      if (b->values) memcpy(b->values + r * (size_t)V, val, (size_t)V * 4);
      if (!tg) continue;
      if (tg->mixers) {
        uint32_t* mc = gmx_batch_contexts(tg->mixers) + r * (size_t)tg->n_mixer_route;
        for (int j = 0; j < tg->n_mixer_route; ++j)
          if (tg->mixer_route[j] >= 0) mc[j] = val[tg->mixer_route[j]];
      }
      if (tg->indirect) {
        uint32_t* ic = gmx_ind_batch_contexts(tg->indirect) + r * (size_t)tg->n_ind_route;
        for (int j = 0; j < tg->n_ind_route; ++j)
          if (tg->ind_route[j] >= 0) ic[j] = val[tg->ind_route[j]];
        gmx_ind_batch_bit_contexts(tg->indirect)[r] = bc;
        gmx_ind_batch_bits(tg->indirect)[r] = (uint8_t)bit;
      }
      if (tg->match) {
        uint32_t* xc = gmx_match_batch_contexts(tg->match) + r * (size_t)tg->n_match_route;
        for (int j = 0; j < tg->n_match_route; ++j)
          if (tg->match_route[j] >= 0) xc[j] = val[tg->match_route[j]];
        gmx_match_batch_bit_contexts(tg->match)[r] = bc;
        gmx_match_batch_bits(tg->match)[r] = (uint8_t)bit;
      }
    }
  }
  return GMX_OK;
}

/* ---- lock step ---- */
#ifdef GMX_SHIM4_NO_LOCKSTEP
/* The shim binaries whose Predictor has no device context objects: gmx_model_adapter.h names the call, nothing makes it. */
static void note_forget_bank(gmx_ctx* cb) { (void)cb; }
int gmx_chainstep_attach_ctx(gmx_chainstep* cs, gmx_ctx* cb, const gmx_ctx_step_routes* routes) {
  (void)cs, (void)cb, (void)routes;
  return GMX_ERR_INVALID;
}
#else
/* gmx_abi_oracle_shim3.c's wrappers under the names dropin/Makefile gives them in abi_shim3_chained.o */
void gmx_shim3_chainstep_destroy(gmx_chainstep* cs);
int gmx_shim3_chainstep_step(gmx_chainstep* cs);
int gmx_shim3_chainstep_launch(gmx_chainstep* cs);

typedef struct ctx_note {
  gmx_chainstep* cs;
  gmx_ctx* cb;
  int32_t mixer[128], ind[128], match[128];
  int n_mixer, n_ind, n_match;
} ctx_note;
enum { kCtxNotes = 64 };
static ctx_note g_ctx_notes[kCtxNotes];
static pthread_mutex_t g_ctx_notes_mu = PTHREAD_MUTEX_INITIALIZER;
static ctx_note* ctx_note_of(gmx_chainstep* cs) {
  ctx_note* n = 0;
  pthread_mutex_lock(&g_ctx_notes_mu);
  for (int i = 0; i < kCtxNotes; ++i)
    if (g_ctx_notes[i].cs == cs) n = &g_ctx_notes[i];
  pthread_mutex_unlock(&g_ctx_notes_mu);
  return n;
}
static void note_forget_bank(gmx_ctx* cb) { /* (after the bank is destroyed the object's steps return GMX_ERR_STATE) */
  pthread_mutex_lock(&g_ctx_notes_mu);
  for (int i = 0; i < kCtxNotes; ++i)
    if (g_ctx_notes[i].cs && g_ctx_notes[i].cb == cb) g_ctx_notes[i].cb = 0;
  pthread_mutex_unlock(&g_ctx_notes_mu);
}

int gmx_chainstep_attach_ctx(gmx_chainstep* cs, gmx_ctx* cb, const gmx_ctx_step_routes* r) {
  if (!cs || !cb || !r) return GMX_ERR_INVALID;
  if (ctx_note_of(cs)) return GMX_ERR_STATE;
  if (cb->S != gmx_chainstep_n_streams(cs) || !route_ok(r->mixer_route, r->n_mixer_route, cb->V)) return GMX_ERR_INVALID;
  const int has_ind = gmx_chainstep_ind_contexts(cs) != 0, has_match = gmx_chainstep_match_contexts(cs) != 0;
  if (has_ind != (r->ind_route != 0) || has_match != (r->match_route != 0)) return GMX_ERR_INVALID;
  if (has_ind && !route_ok(r->ind_route, r->n_ind_route, cb->V)) return GMX_ERR_INVALID;
  if (has_match && !route_ok(r->match_route, r->n_match_route, cb->V)) return GMX_ERR_INVALID;
  ctx_note* n = ctx_note_of(0);
  if (!n) return GMX_ERR_NOMEM;
  memset(n, 0, sizeof *n);
  n->cb = cb;
  n->n_mixer = r->n_mixer_route;
  memcpy(n->mixer, r->mixer_route, (size_t)n->n_mixer * 4);
  if (has_ind) {
    n->n_ind = r->n_ind_route;
    memcpy(n->ind, r->ind_route, (size_t)n->n_ind * 4);
  }
  if (has_match) {
    n->n_match = r->n_match_route;
    memcpy(n->match, r->match_route, (size_t)n->n_match * 4);
  }
  n->cs = cs;
  return GMX_OK;
}

static int ctx_stage(gmx_chainstep* cs) {
  ctx_note* n = cs ? ctx_note_of(cs) : 0;
  if (!n) return GMX_OK;
  gmx_ctx* cb = n->cb;
  if (!cb) return GMX_ERR_STATE;
  const uint8_t* what = gmx_chainstep_what(cs);
  for (int s = 0; s < cb->S; ++s) {
    cref* c = cb->st[s];
    if (what[s] & GMX_STEP_LEARN) {
      c->b.new_bit = gmx_chainstep_bits(cs)[s] ? 1 : 0;
      cb->fwd[s] = 0;
    }
    if (!(what[s] & GMX_STEP_PREDICT)) continue;
    step(c, c->b.new_bit);
    cb->fwd[s] = 1;
    const uint32_t* val = c->b.values;
    uint32_t* mc = gmx_chainstep_contexts(cs) + (size_t)s * n->n_mixer;
    for (int j = 0; j < n->n_mixer; ++j)
      if (n->mixer[j] >= 0) mc[j] = val[n->mixer[j]];
    if (n->n_ind) {
      uint32_t* ic = gmx_chainstep_ind_contexts(cs) + (size_t)s * n->n_ind;
      for (int j = 0; j < n->n_ind; ++j)
        if (n->ind[j] >= 0) ic[j] = val[n->ind[j]];
    }
    if (n->n_match) {
      uint32_t* xc = gmx_chainstep_match_contexts(cs) + (size_t)s * n->n_match;
      for (int j = 0; j < n->n_match; ++j)
        if (n->match[j] >= 0) xc[j] = val[n->match[j]];
    }
    if (gmx_chainstep_bit_contexts(cs)) gmx_chainstep_bit_contexts(cs)[s] = (uint32_t)c->b.recent_bits - 1;
  }
  return GMX_OK;
}
void __wrap_gmx_chainstep_destroy(gmx_chainstep* cs) {
  ctx_note* n = cs ? ctx_note_of(cs) : 0;
  if (n) {
    pthread_mutex_lock(&g_ctx_notes_mu);
    memset(n, 0, sizeof *n);
    pthread_mutex_unlock(&g_ctx_notes_mu);
  }
  gmx_shim3_chainstep_destroy(cs);
}
int __wrap_gmx_chainstep_step(gmx_chainstep* cs) {
  const int rc = ctx_stage(cs);
  return rc ? rc : gmx_shim3_chainstep_step(cs);
}
int __wrap_gmx_chainstep_launch(gmx_chainstep* cs) {
  const int rc = ctx_stage(cs);
  return rc ? rc : gmx_shim3_chainstep_launch(cs);
}
#endif /* GMX_SHIM4_NO_LOCKSTEP */
