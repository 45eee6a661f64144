/* gmx_abi_oracle_shim3.c -- TEST INFRASTRUCTURE, CPU only (see gmx_abi_oracle_shim.c): the gmx_match_* entry points
 * gmx_model_adapter.h calls for gmx::GpuMatch, answered by tests/helpers/match_ref.c (pinned to the reference by
 * tests/golden/match_*.npz, tests/test_match_ref.py), so that the host logic of the full drop-in can be run inside the
 * real reference without a GPU (oracle/_ref/shim/*_full*_shim, tests/test_full_cpu.py).  Never shipped, never a fallback.
 *
 * Lock step: gmx_chainstep_* live in gmx_abi_oracle_shim2.c, which knows nothing of a Match bank.  The *_full*_shim
 * binaries are linked with -Wl,--wrap= for gmx_chainstep_create / _destroy / _step / _launch (dropin/Makefile): the
 * wrappers here note each object's group, and run the Match stage of a step -- the history push and K x Match::Learn,
 * then K x Match::Predict into the object's own pinned records -- in front of shim2's step. */
#include "../helpers/match_ref.c"

#include <pthread.h>

#include "../../include/gmxmix.h"

typedef struct mstream {
  mref* r;
  uint32_t ctx[8]; /* the contexts of the byte that is open */
  uint32_t bc;
  unsigned lm;     /* longest_match of the pending forward */
  int fwd;         /* a forward waits for its learn */
} mstream;
struct gmx_match {
  int S, K;
  gmx_match_desc d[8];
  uint64_t cap;
  mstream* st;
};
#define MST(mb, s) ((mb) && (s) >= 0 && (s) < (mb)->S ? &(mb)->st[s] : 0)

static mref* m_fresh(const gmx_match* mb) {
  uint32_t ts[8];
  int lim[8];
  for (int k = 0; k < mb->K; ++k) {
    ts[k] = mb->d[k].table_size;
    lim[k] = mb->d[k].limit;
  }
  return mref_create(mb->K, ts, lim);
}

int gmx_match_create(gmx_match** out, const gmx_match_desc* models, int n_models, uint64_t history_capacity, int n_streams,
                     int device) {
  (void)device;
  if (!out || !models || n_models < 1 || n_models > 8 || n_streams < 1 || !history_capacity || history_capacity >> 32)
    return GMX_ERR_INVALID;
  gmx_match* mb = (gmx_match*)calloc(1, sizeof *mb);
  mb->S = n_streams;
  mb->K = n_models;
  mb->cap = history_capacity;
  memcpy(mb->d, models, (size_t)n_models * sizeof *models);
  mb->st = (mstream*)calloc((size_t)n_streams, sizeof(mstream));
  for (int s = 0; s < n_streams; ++s) mb->st[s].r = m_fresh(mb);
  *out = mb;
  return GMX_OK;
}
void gmx_match_destroy(gmx_match* mb) {
  if (!mb) return;
  for (int s = 0; s < mb->S; ++s) mref_destroy(mb->st[s].r);
  free(mb->st);
  free(mb);
}
int gmx_match_n_models(const gmx_match* mb) { return mb ? mb->K : GMX_ERR_INVALID; }
int gmx_match_n_streams(const gmx_match* mb) { return mb ? mb->S : GMX_ERR_INVALID; }

/* K x Match::Predict with the contexts given (match.cpp:25-74) */
static void m_predict(gmx_match* mb, mstream* st, const uint32_t* ctx, uint32_t bc, float* pred, uint8_t* act, uint32_t* longest) {
  unsigned lm = 0;
  for (int k = 0; k < mb->K; ++k) {
    const int a = mref_predict(st->r, &st->r->m[k], ctx[k], bc, &lm);
    if (pred) pred[k] = st->r->m[k].slot;
    if (act) act[k] = (uint8_t)a;
  }
  memcpy(st->ctx, ctx, (size_t)mb->K * 4);
  st->bc = bc;
  st->lm = lm;
  st->fwd = 1;
  if (longest) *longest = lm;
}
/* the history push of BasicContexts::Learn (basic-contexts.cpp:44-53) + K x Match::Learn (match.cpp:76-109) */
static void m_learn(gmx_match* mb, mstream* st, int bit) {
  mref* r = st->r;
  r->new_bit = bit;
  const int current_byte = (int)(st->bc + 1) * 2 + bit;
  if (current_byte >= 256 && st->lm < 2) {
    if (r->hist_size == r->hist_cap) {
      r->hist_cap *= 2;
      r->history = (uint8_t*)realloc(r->history, r->hist_cap);
    }
    r->history[r->hist_size++] = (uint8_t)current_byte;
  }
  for (int k = 0; k < mb->K; ++k) mref_learn(r, &r->m[k], st->ctx[k], st->bc, st->lm);
  st->fwd = 0;
}

int gmx_match_forward(gmx_match* mb, int stream, const uint32_t* contexts, uint32_t bit_context, float* predictions,
                      uint8_t* active, uint32_t* longest_match) {
  mstream* st = MST(mb, stream);
  if (!st || !contexts || bit_context > 254u) return GMX_ERR_INVALID;
  if (st->fwd) return GMX_ERR_STATE;
  m_predict(mb, st, contexts, bit_context, predictions, active, longest_match);
  return GMX_OK;
}
int gmx_match_learn(gmx_match* mb, int stream, int bit) {
  mstream* st = MST(mb, stream);
  if (!st || (bit != 0 && bit != 1)) return GMX_ERR_INVALID;
  if (!st->fwd) return GMX_ERR_STATE;
  if (st->bc >= 127u && st->r->hist_size + 1 > mb->cap) return GMX_ERR_INVALID;
  m_learn(mb, st, bit);
  return GMX_OK;
}
int gmx_match_slots_get(gmx_match* mb, int stream, float* values, int* new_bit) {
  mstream* st = MST(mb, stream);
  if (!st || (!values && !new_bit)) return GMX_ERR_INVALID;
  float v[8];
  int nb;
  mref_slots_get(st->r, v, &nb);
  if (values) memcpy(values, v, (size_t)mb->K * 4);
  if (new_bit) *new_bit = nb;
  return GMX_OK;
}
int gmx_match_slots_set(gmx_match* mb, int stream, const float* values, int new_bit) {
  mstream* st = MST(mb, stream);
  if (!st || !values || (new_bit != 0 && new_bit != 1)) return GMX_ERR_INVALID;
  mref_slots_set(st->r, values, new_bit);
  st->fwd = 0; /* (a new blackboard drops a pending forward: gmxmix.h) */
  return GMX_OK;
}
int gmx_match_history_size(gmx_match* mb, int stream, uint64_t* size) {
  mstream* st = MST(mb, stream);
  if (!st || !size) return GMX_ERR_INVALID;
  *size = mref_history_size(st->r);
  return GMX_OK;
}
int gmx_match_export(gmx_match* mb, int stream, void* long_buf, size_t* long_bytes, void* short_buf, size_t* short_bytes) {
  mstream* st = MST(mb, stream);
  if (!st || !long_bytes || !short_bytes) return GMX_ERR_INVALID;
  const size_t need = (size_t)mref_export_long(st->r, 0), need_short = 11 * (size_t)mb->K;
  const int fits = (!long_buf || *long_bytes >= need) && (!short_buf || *short_bytes >= need_short);
  *long_bytes = need;
  *short_bytes = need_short;
  if (!long_buf && !short_buf) return GMX_OK;
  if (!fits) return GMX_ERR_INVALID;
  if (short_buf) mref_export_short(st->r, (uint8_t*)short_buf);
  if (long_buf) mref_export_long(st->r, (uint8_t*)long_buf);
  return GMX_OK;
}
int gmx_match_import(gmx_match* mb, int stream, const void* long_buf, size_t long_bytes, const void* short_buf,
                     size_t short_bytes) {
  mstream* st = MST(mb, stream);
  if (!st || !long_buf || !short_buf) return GMX_ERR_INVALID;
  if (long_bytes >= 8) {
    unsigned long long hs;
    memcpy(&hs, long_buf, 8);
    if (hs > mb->cap) return GMX_ERR_FORMAT;
  }
  /* mref_import fills a freshly created object; the slot values and new_bit are not the checkpoint's (gmxmix.h) */
  mref* fresh = m_fresh(mb);
  if (mref_import(fresh, (const uint8_t*)long_buf, long_bytes, (const uint8_t*)short_buf, short_bytes)) {
    mref_destroy(fresh);
    return GMX_ERR_FORMAT;
  }
  float v[8];
  int nb;
  mref_slots_get(st->r, v, &nb);
  mref_slots_set(fresh, v, nb);
  mref_destroy(st->r);
  st->r = fresh;
  st->fwd = 0;
  return GMX_OK;
}
int gmx_match_copy(gmx_match* dst, int ds, gmx_match* src, int ss) {
  mstream *d = MST(dst, ds), *s = MST(src, ss);
  if (!d || !s || dst->K != src->K) return GMX_ERR_INVALID;
  for (int k = 0; k < dst->K; ++k)
    if (dst->d[k].table_size != src->d[k].table_size || dst->d[k].limit != src->d[k].limit || dst->d[k].slot != src->d[k].slot)
      return GMX_ERR_INVALID;
  if (d == s) return GMX_OK;
  if (mref_history_size(s->r) > dst->cap) return GMX_ERR_INVALID;
  const size_t nl = (size_t)mref_export_long(s->r, 0);
  uint8_t* l = (uint8_t*)malloc(nl ? nl : 1);
  uint8_t sh[11 * 8];
  mref_export_long(s->r, l);
  mref_export_short(s->r, sh);
  mref* fresh = m_fresh(dst);
  const int bad = mref_import(fresh, l, nl, sh, 11 * (size_t)dst->K);
  free(l);
  if (bad) {
    mref_destroy(fresh);
    return GMX_ERR_FORMAT;
  }
  float v[8];
  int nb;
  mref_slots_get(s->r, v, &nb);
  mref_slots_set(fresh, v, nb);
  mref_destroy(d->r);
  d->r = fresh;
  memcpy(d->ctx, s->ctx, sizeof d->ctx);
  d->bc = s->bc;
  d->lm = s->lm;
  d->fwd = 0; /* (as the product: a copy drops the pending forward) */
  return GMX_OK;
}
int gmx_match_memory_usage(gmx_match* mb, int model, uint64_t* bytes) {
  if (!mb || model < 0 || model >= mb->K || !bytes) return GMX_ERR_INVALID;
  *bytes = mref_memory_usage(mb->st[0].r, model);
  return GMX_OK;
}

/* ---- the batched surface the run-ahead compressor uses (MixerPool::Lead): plain host arrays, the "device work" done
 * when the run call is made ---- */
struct gmx_match_batch {
  gmx_match* mb;
  uint64_t T;
  uint32_t *ctx, *bc, *lng;
  uint8_t *bits, *act;
  float* pred;
};
int gmx_match_batch_create(gmx_match_batch** out, gmx_match* mb, uint64_t max_bits) {
  if (!out || !mb || !max_bits) return GMX_ERR_INVALID;
  gmx_match_batch* b = (gmx_match_batch*)calloc(1, sizeof *b);
  const size_t R = (size_t)mb->S * max_bits;
  b->mb = mb;
  b->T = max_bits;
  b->ctx = (uint32_t*)calloc(R * mb->K, 4);
  b->bc = (uint32_t*)calloc(R, 4);
  b->bits = (uint8_t*)calloc(R, 1);
  b->pred = (float*)calloc(R * mb->K, 4);
  b->act = (uint8_t*)calloc(R * mb->K, 1);
  b->lng = (uint32_t*)calloc(R, 4);
  *out = b;
  return GMX_OK;
}
void gmx_match_batch_destroy(gmx_match_batch* b) {
  if (!b) return;
  free(b->ctx);
  free(b->bc);
  free(b->bits);
  free(b->pred);
  free(b->act);
  free(b->lng);
  free(b);
}
uint64_t gmx_match_batch_max_bits(const gmx_match_batch* b) { return b ? b->T : 0; }
uint32_t* gmx_match_batch_contexts(gmx_match_batch* b) { return b->ctx; }
uint32_t* gmx_match_batch_bit_contexts(gmx_match_batch* b) { return b->bc; }
uint8_t* gmx_match_batch_bits(gmx_match_batch* b) { return b->bits; }
const float* gmx_match_batch_predictions(gmx_match_batch* b) { return b->pred; }
const uint8_t* gmx_match_batch_active(gmx_match_batch* b) { return b->act; }
const uint32_t* gmx_match_batch_longest(gmx_match_batch* b) { return b->lng; }
int gmx_match_batch_upload(gmx_match_batch* b, uint64_t n) { return (b && n <= b->T) ? GMX_OK : GMX_ERR_INVALID; }
int gmx_match_batch_download(gmx_match_batch* b, uint64_t n) { return (b && n <= b->T) ? GMX_OK : GMX_ERR_INVALID; }
int gmx_match_batch_wait(gmx_match_batch* b) { return b ? GMX_OK : GMX_ERR_INVALID; }

/* the mixer batch's arrays (gmx_abi_oracle_shim.c) */
extern float* gmx_batch_predictions(gmx_batch* b);
extern uint32_t* gmx_batch_active_mask(gmx_batch* b);
extern uint32_t* gmx_batch_contexts(gmx_batch* b);
extern int gmx_batch_n_pad(const gmx_batch* b);
extern int gmx_batch_mask_words(const gmx_batch* b);
extern uint64_t gmx_batch_max_bits(const gmx_batch* b);
extern int gmx_shim_batch_m(const gmx_batch* b);

/* what a Predict leaves in one record of the mixers: the slots, their active bits, longest_match in the gate columns */
static void m_into(const gmx_match* mb, const float* pred, const uint8_t* act, uint32_t lm, float* mp, uint32_t* mm,
                   uint32_t* mc, const int32_t* cols, int n_cols) {
  for (int k = 0; k < mb->K; ++k) {
    const int slot = mb->d[k].slot;
    mp[slot] = pred[k];
    if (act[k])
      mm[slot >> 5] |= 1u << (slot & 31);
    else
      mm[slot >> 5] &= ~(1u << (slot & 31));
  }
  for (int c = 0; c < n_cols; ++c) mc[cols[c]] = lm;
}

int gmx_match_run_ragged(gmx_match* mb, gmx_match_batch* b, const uint64_t* n_bits, gmx_batch* into, const int32_t* ctx_columns,
                         int n_ctx_columns) {
  if (!mb || !b || b->mb != mb || !n_bits || n_ctx_columns < 0 || n_ctx_columns > 8 || (!into && n_ctx_columns)) return GMX_ERR_INVALID;
  const int K = mb->K;
  for (int s = 0; s < mb->S; ++s) {
    if (n_bits[s] > b->T || (into && n_bits[s] > gmx_batch_max_bits(into))) return GMX_ERR_INVALID;
    if (mref_history_size(mb->st[s].r) + (n_bits[s] + 7) / 8 > mb->cap) return GMX_ERR_INVALID; /* before anything runs */
  }
  for (int s = 0; s < mb->S; ++s) {
    mstream* st = &mb->st[s];
    const size_t r0 = (size_t)s * b->T;
    for (uint64_t t = 0; t < n_bits[s]; ++t) {
      const size_t r = r0 + t;
      m_predict(mb, st, b->ctx + r * K, b->bc[r], b->pred + r * K, b->act + r * K, &b->lng[r]);
      if (into) {
        const uint64_t MT = gmx_batch_max_bits(into);
        const size_t q = (size_t)s * MT + t;
        m_into(mb, b->pred + r * K, b->act + r * K, b->lng[r], gmx_batch_predictions(into) + q * gmx_batch_n_pad(into),
               gmx_batch_active_mask(into) + q * gmx_batch_mask_words(into),
               gmx_batch_contexts(into) + q * gmx_shim_batch_m(into), ctx_columns, n_ctx_columns);
      }
      m_learn(mb, st, b->bits[r] ? 1 : 0);
    }
  }
  return GMX_OK;
}

#ifdef GMX_SHIM3_NO_LOCKSTEP
/* The shim binaries whose Predictor has no gmx::GpuMatch: gmx_model_adapter.h names these calls, nothing makes them. */
int gmx_chainstep_attach_match(gmx_chainstep* cs, gmx_match* mb, const int32_t* ctx_columns, int n_ctx_columns) {
  (void)cs, (void)mb, (void)ctx_columns, (void)n_ctx_columns;
  return GMX_ERR_INVALID;
}
uint32_t* gmx_chainstep_match_contexts(gmx_chainstep* cs) {
  (void)cs;
  return 0;
}
#else
/* ---- lock step: the Match stage in front of gmx_abi_oracle_shim2.c's step ---- */
extern int gmx_group_n_mixers(const gmx_group* g);
extern int gmx_group_n_inputs(const gmx_group* g);
extern int gmx_group_n_streams(const gmx_group* g);
int __real_gmx_chainstep_create(gmx_chainstep** out, gmx_group* g, gmx_indirect* ib, gmx_lstm* l, int lstm_slot, int mixer_ctx_col,
                                int ind_ctx_col);
void __real_gmx_chainstep_destroy(gmx_chainstep* cs);
int __real_gmx_chainstep_step(gmx_chainstep* cs);
int __real_gmx_chainstep_launch(gmx_chainstep* cs);

typedef struct cs_note {
  gmx_chainstep* cs;
  gmx_group* g;
  gmx_match* mb;
  int32_t cols[8];
  int n_cols, stepped;
  uint32_t* mctx;   /* [S][K] the caller's records */
  uint8_t* started; /* [S] the stream has predicted through this object */
} cs_note;
enum { kNotes = 64 };
static cs_note g_notes[kNotes];
static pthread_mutex_t g_notes_mu = PTHREAD_MUTEX_INITIALIZER;
static cs_note* note_of(gmx_chainstep* cs) {
  cs_note* n = 0;
  pthread_mutex_lock(&g_notes_mu);
  for (int i = 0; i < kNotes; ++i)
    if (g_notes[i].cs == cs) n = &g_notes[i];
  pthread_mutex_unlock(&g_notes_mu);
  return n;
}

int __wrap_gmx_chainstep_create(gmx_chainstep** out, gmx_group* g, gmx_indirect* ib, gmx_lstm* l, int lstm_slot, int mixer_ctx_col,
                                int ind_ctx_col) {
  const int rc = __real_gmx_chainstep_create(out, g, ib, l, lstm_slot, mixer_ctx_col, ind_ctx_col);
  if (rc != GMX_OK) return rc;
  cs_note* n = note_of(0);
  if (!n) {
    __real_gmx_chainstep_destroy(*out);
    return GMX_ERR_NOMEM;
  }
  memset(n, 0, sizeof *n);
  n->g = g;
  n->cs = *out;
  return GMX_OK;
}
void __wrap_gmx_chainstep_destroy(gmx_chainstep* cs) {
  cs_note* n = cs ? note_of(cs) : 0;
  if (n) {
    free(n->mctx);
    free(n->started);
    pthread_mutex_lock(&g_notes_mu);
    memset(n, 0, sizeof *n);
    pthread_mutex_unlock(&g_notes_mu);
  }
  __real_gmx_chainstep_destroy(cs);
}
int gmx_chainstep_attach_match(gmx_chainstep* cs, gmx_match* mb, const int32_t* ctx_columns, int n_ctx_columns) {
  cs_note* n = cs ? note_of(cs) : 0;
  if (!n || !mb || n_ctx_columns < 0 || n_ctx_columns > 8 || (n_ctx_columns && !ctx_columns)) return GMX_ERR_INVALID;
  if (n->mb || n->stepped) return GMX_ERR_STATE;
  if (mb->S != gmx_group_n_streams(n->g) || !gmx_chainstep_bit_contexts(cs)) return GMX_ERR_INVALID;
  for (int k = 0; k < mb->K; ++k)
    if (mb->d[k].slot < 0 || mb->d[k].slot >= gmx_group_n_inputs(n->g)) return GMX_ERR_INVALID;
  for (int c = 0; c < n_ctx_columns; ++c) {
    if (ctx_columns[c] < 0 || ctx_columns[c] >= gmx_group_n_mixers(n->g)) return GMX_ERR_INVALID;
    n->cols[c] = ctx_columns[c];
  }
  n->n_cols = n_ctx_columns;
  n->mctx = (uint32_t*)calloc((size_t)mb->S * mb->K, 4);
  n->started = (uint8_t*)calloc((size_t)mb->S, 1);
  n->mb = mb;
  return GMX_OK;
}
uint32_t* gmx_chainstep_match_contexts(gmx_chainstep* cs) {
  cs_note* n = cs ? note_of(cs) : 0;
  return n ? n->mctx : 0;
}
static int match_stage(gmx_chainstep* cs) {
  cs_note* n = cs ? note_of(cs) : 0;
  if (!n) return GMX_OK;
  n->stepped = 1;
  gmx_match* mb = n->mb;
  if (!mb) return GMX_OK;
  const int N = gmx_group_n_inputs(n->g), M = gmx_group_n_mixers(n->g);
  const int n_pad = (N + 3) / 4 * 4, mw = (N + 31) / 32;
  const uint8_t* what = gmx_chainstep_what(cs);
  for (int s = 0; s < mb->S; ++s) /* the capacity rule: refused before anything runs */
    if ((what[s] & GMX_STEP_LEARN) && mb->st[s].fwd && mb->st[s].bc >= 127u && mref_history_size(mb->st[s].r) + 1 > mb->cap)
      return GMX_ERR_INVALID;
  for (int s = 0; s < mb->S; ++s) {
    mstream* st = &mb->st[s];
    if ((what[s] & GMX_STEP_LEARN) && st->fwd) m_learn(mb, st, gmx_chainstep_bits(cs)[s] ? 1 : 0);
    if (what[s] & GMX_STEP_PREDICT) {
      const uint32_t bc = gmx_chainstep_bit_contexts(cs)[s];
      uint32_t ctx[8];
      memcpy(ctx, st->ctx, sizeof ctx);
      if (bc == 0 || !n->started[s]) memcpy(ctx, n->mctx + (size_t)s * mb->K, (size_t)mb->K * 4);
      n->started[s] = 1;
      float pred[8];
      uint8_t act[8];
      uint32_t lm = 0;
      st->fwd = 0; /* (a forward left pending outside the object is dropped by a step) */
      m_predict(mb, st, ctx, bc, pred, act, &lm);
      m_into(mb, pred, act, lm, gmx_chainstep_predictions(cs) + (size_t)s * n_pad, gmx_chainstep_active_mask(cs) + (size_t)s * mw,
             gmx_chainstep_contexts(cs) + (size_t)s * M, n->cols, n->n_cols);
    }
  }
  return GMX_OK;
}
int __wrap_gmx_chainstep_step(gmx_chainstep* cs) {
  const int rc = match_stage(cs);
  return rc ? rc : __real_gmx_chainstep_step(cs);
}
int __wrap_gmx_chainstep_launch(gmx_chainstep* cs) {
  const int rc = match_stage(cs);
  return rc ? rc : __real_gmx_chainstep_launch(cs);
}
#endif /* GMX_SHIM3_NO_LOCKSTEP */
