// gmx_ppmd.h -- the reference's PPMd byte model (models/mod_ppmd.cpp: PPMd var.I with SEE, inheritance, rescale and
// the cutOff model flush, as ModPPMD drives it) restated as pure functions for host and device alike (GMX_HD, as
// gmx_coder.h).  No HIP in here: tests/cpp/test_ppmd.cpp builds it for the host, where it is the checker of the GPU
// tests; gmx_ppmd.hip hosts it in the bank's kernel.  DESIGN.md section 4.24.
//
// A stream is {GmxPpmdState, arena}.  The arena is the model's heap: `size` bytes, zero at create and at reset (the
// model reads units it never wrote), addressed by 32-bit offsets from its base only, so it stays below 4 GiB.  Every
// link of the model is such an offset; 0 is "none" (offset 0 is the first text byte, never a unit).  The packed
// layouts are the reference's, byte for byte:
//   context (12): NumStats u8, Flags u8, SummFreq u16, iStats u32, iSuffix u32; a binary context keeps its one state
//                 over SummFreq/iStats, at +2
//   state    (6): Symbol u8, Freq u8, iSuccessor u32 at +2 -- 2-byte aligned only in every other state of a table
//   free block  : Stamp u32, Next u32, NU u32
// Units lie at multiples of 4 (the arena's size is a multiple of 2^20, the unit area a multiple of 12 from its end),
// so context and block fields are aligned 32-bit accesses and a state's successor goes as two 16-bit halves.
//
// The free lists' heads are not heap units but are walked with the same links: a "node" is a heap offset, or
// GMX_PPMD_HEAD + 8k for head k of the state block.  No arena reaches GMX_PPMD_HEAD (4095 MiB = 0xfff00000).
//
// The recursions of the reference are explicit stacks in the state block: cutOff's frames (depth order + 2) and
// CreateSuccessors' list of states (order + 1).  So nothing here needs a stack of its own on the device.
#ifndef GMX_PPMD_H_
#define GMX_PPMD_H_

#include "gmx_math.h"

#define GMX_PPMD_MIN_ORDER 2
#define GMX_PPMD_MAX_ORDER 64
#define GMX_PPMD_MAX_ARENA_MB 4095
#define GMX_PPMD_N_INDEXES 38
#define GMX_PPMD_HEAD 0xfffffe00u
#define GMX_PPMD_UNIT 12u
#define GMX_PPMD_MAX_FREQ 124
#define GMX_PPMD_O_BOUND 9
#define GMX_PPMD_FAR (128u * 1024u)

#if defined(GMX_PPMD_CENSUS) && !defined(__HIP_DEVICE_COMPILE__)
enum {
  GMX_PC_RESTORE, GMX_PC_CUTOFF, GMX_PC_CUT_FREE, GMX_PC_CUT_FOLD, GMX_PC_CUT_RESCALE, GMX_PC_CUT_BIN_FREE,
  GMX_PC_MOVE_UP, GMX_PC_GLUE, GMX_PC_RARE_NULL, GMX_PC_SPLIT, GMX_PC_SHIFT_RARE, GMX_PC_RESCALE, GMX_PC_RESCALE_ZERO,
  GMX_PC_RESCALE_FOLD, GMX_PC_FULL_ORDER, GMX_PC_BIN_UPDATE, GMX_PC_REDUCE_ORDER, GMX_PC_EXPAND, GMX_PC_BIN_TO_TWO,
  GMX_PC_TEXT_FULL, GMX_PC_COUNT
};
static uint64_t gmx_ppmd_census[GMX_PC_COUNT];
static uint64_t gmx_ppmd_census_ns[257];  // contexts scanned, by their number of symbols
#define GMX_PPMD_HIT(k) (++gmx_ppmd_census[k])
#define GMX_PPMD_SCAN(n) (++gmx_ppmd_census_ns[n])
#else
#define GMX_PPMD_HIT(k) ((void)0)
#define GMX_PPMD_SCAN(n) ((void)0)
#endif

struct GmxPpmdSee {
  uint16_t summ;
  uint8_t shift, count;
};

struct GmxPpmdFrame {
  uint32_t q, p0;
  int32_t i, pi;
};

struct GmxPpmdState {
  uint32_t blist[GMX_PPMD_N_INDEXES + 2][2];  // {Stamp, Next}; [N_INDEXES] is the far list, the last is the glue's own
  uint32_t glue_count, glue_count1;
  uint64_t size;
  uint32_t text, units_start, lo, hi, aux;
  uint32_t found, max_ctx, saved_pc;
  int32_t order_fall, max_order, run_length, init_rl, num_masked, prev_success, bsumm;
  uint32_t esc_count;
  uint32_t restores;  // model flushes since create / reset
  // the bank's records (gmx_ppmd_record): the byte the next record's UpdateByte takes, and whether it is still owed
  uint8_t last_byte, pending, pad_[2];
  uint16_t bin_summ[25][64];
  GmxPpmdSee see2[23][32];
  GmxPpmdSee dummy_see;
  uint32_t char_mask[256];
  uint32_t sqp[256];
  uint32_t count[GMX_PPMD_N_INDEXES];
  uint32_t ps[GMX_PPMD_MAX_ORDER + 2];
  GmxPpmdFrame frame[GMX_PPMD_MAX_ORDER + 2];
  uint8_t indx2units[GMX_PPMD_N_INDEXES];
  uint8_t units2indx[128];
  uint8_t ns2bs[256];
  uint8_t qtable[260];
};

// ---- arena access ----
GMX_HD uint32_t gmx_pp_ld8(const uint8_t* a, uint32_t o) { return a[o]; }
GMX_HD void gmx_pp_st8(uint8_t* a, uint32_t o, uint32_t v) { a[o] = (uint8_t)v; }
GMX_HD uint32_t gmx_pp_ld16(const uint8_t* a, uint32_t o) { return *(const uint16_t*)(a + o); }
GMX_HD void gmx_pp_st16(uint8_t* a, uint32_t o, uint32_t v) { *(uint16_t*)(a + o) = (uint16_t)v; }
GMX_HD uint32_t gmx_pp_ld32(const uint8_t* a, uint32_t o) { return *(const uint32_t*)(a + o); }
GMX_HD void gmx_pp_st32(uint8_t* a, uint32_t o, uint32_t v) { *(uint32_t*)(a + o) = v; }
// a state's successor: two halves
GMX_HD uint32_t gmx_pp_succ(const uint8_t* a, uint32_t p) {
  return gmx_pp_ld16(a, p + 2) | (gmx_pp_ld16(a, p + 4) << 16);
}
GMX_HD void gmx_pp_set_succ(uint8_t* a, uint32_t p, uint32_t v) {
  gmx_pp_st16(a, p + 2, v & 0xffffu);
  gmx_pp_st16(a, p + 4, v >> 16);
}
GMX_HD void gmx_pp_copy_state(uint8_t* a, uint32_t dst, uint32_t src) {
  const uint32_t w0 = gmx_pp_ld16(a, src), w1 = gmx_pp_ld16(a, src + 2), w2 = gmx_pp_ld16(a, src + 4);
  gmx_pp_st16(a, dst, w0);
  gmx_pp_st16(a, dst + 2, w1);
  gmx_pp_st16(a, dst + 4, w2);
}
GMX_HD void gmx_pp_swap_states(uint8_t* a, uint32_t x, uint32_t y) {
  for (uint32_t k = 0; k < 6; k += 2) {
    const uint32_t t = gmx_pp_ld16(a, x + k);
    gmx_pp_st16(a, x + k, gmx_pp_ld16(a, y + k));
    gmx_pp_st16(a, y + k, t);
  }
}
GMX_HD void gmx_pp_copy_units(uint8_t* a, uint32_t dst, uint32_t src, uint32_t nu) {
  for (uint32_t k = 0; k < 3 * nu; ++k) gmx_pp_st32(a, dst + 4 * k, gmx_pp_ld32(a, src + 4 * k));
}
// context fields
#define GMX_PP_NS(a, c) gmx_pp_ld8(a, c)
#define GMX_PP_FLAGS(a, c) gmx_pp_ld8(a, (c) + 1)
#define GMX_PP_SUMM(a, c) gmx_pp_ld16(a, (c) + 2)
#define GMX_PP_STATS(a, c) gmx_pp_ld32(a, (c) + 4)
#define GMX_PP_SUFFIX(a, c) gmx_pp_ld32(a, (c) + 8)

// ---- nodes of the free lists ----
GMX_HD uint32_t gmx_pp_head(uint32_t k) { return GMX_PPMD_HEAD + 8u * k; }
GMX_HD uint32_t gmx_pp_node_next(const GmxPpmdState* s, const uint8_t* a, uint32_t n) {
  return n >= GMX_PPMD_HEAD ? s->blist[(n - GMX_PPMD_HEAD) >> 3][1] : gmx_pp_ld32(a, n + 4);
}
GMX_HD void gmx_pp_node_set_next(GmxPpmdState* s, uint8_t* a, uint32_t n, uint32_t v) {
  if (n >= GMX_PPMD_HEAD)
    s->blist[(n - GMX_PPMD_HEAD) >> 3][1] = v;
  else
    gmx_pp_st32(a, n + 4, v);
}
// the head's own list operations
GMX_HD uint32_t gmx_pp_list_pop(GmxPpmdState* s, const uint8_t* a, uint32_t k) {
  const uint32_t p = s->blist[k][1];
  s->blist[k][1] = gmx_pp_ld32(a, p + 4);
  s->blist[k][0]--;
  return p;
}
GMX_HD void gmx_pp_list_push(GmxPpmdState* s, uint8_t* a, uint32_t k, uint32_t p, uint32_t nu) {
  gmx_pp_st32(a, p + 4, s->blist[k][1]);
  s->blist[k][1] = p;
  gmx_pp_st32(a, p, 0xffffffffu);
  gmx_pp_st32(a, p + 8, nu);
  s->blist[k][0]++;
}

// ---- the sub-allocator ----
GMX_HD void gmx_ppmd_init_allocator(GmxPpmdState* s) {
  for (int k = 0; k < GMX_PPMD_N_INDEXES + 2; ++k) s->blist[k][0] = s->blist[k][1] = 0;
  s->text = 0;
  s->hi = (uint32_t)s->size;
  const uint64_t units = s->size / 8 / GMX_PPMD_UNIT * 7 * GMX_PPMD_UNIT;
  s->lo = s->units_start = (uint32_t)(s->size - units);
  s->glue_count = s->glue_count1 = 0;
}

GMX_HD uint64_t gmx_ppmd_used_memory(const GmxPpmdState* s) {
  uint64_t r = s->size - (uint64_t)(s->hi - s->lo) - (uint64_t)(s->units_start - s->text);
  for (int k = 0; k < GMX_PPMD_N_INDEXES; ++k) r -= (uint64_t)((uint32_t)s->indx2units[k] * s->blist[k][0]) * 12u;
  return r;
}

GMX_HD void gmx_pp_glue(GmxPpmdState* s, uint8_t* a) {
  GMX_PPMD_HIT(GMX_PC_GLUE);
  const uint32_t own = GMX_PPMD_N_INDEXES + 1;
  if (s->lo != s->hi) gmx_pp_st8(a, s->lo, 0);
  s->blist[own][1] = 0;
  uint32_t tail = gmx_pp_head(own);
  for (uint32_t k = 0; k <= GMX_PPMD_N_INDEXES; ++k) {
    while (s->blist[k][1]) {
      const uint32_t p = gmx_pp_list_pop(s, a, k);
      if (gmx_pp_ld32(a, p + 8)) {
        for (;;) {
          const uint32_t p1 = p + GMX_PPMD_UNIT * gmx_pp_ld32(a, p + 8);
          if (gmx_pp_ld32(a, p1) != 0xffffffffu) break;
          gmx_pp_st32(a, p + 8, gmx_pp_ld32(a, p + 8) + gmx_pp_ld32(a, p1 + 8));
          gmx_pp_st32(a, p1 + 8, 0);
        }
        gmx_pp_st32(a, p + 4, gmx_pp_node_next(s, a, tail));
        gmx_pp_node_set_next(s, a, tail, p);
        tail = p;
      }
    }
  }
  while (s->blist[own][1]) {
    uint32_t p = gmx_pp_list_pop(s, a, own);
    uint32_t sz = gmx_pp_ld32(a, p + 8);
    if (sz) {
      for (; sz > 128; sz -= 128, p += 128 * GMX_PPMD_UNIT) gmx_pp_list_push(s, a, GMX_PPMD_N_INDEXES - 1, p, 128);
      uint32_t i = s->units2indx[sz - 1];
      if (s->indx2units[i] != sz) {
        const uint32_t k = sz - s->indx2units[--i];
        gmx_pp_list_push(s, a, k - 1, p + (sz - k) * GMX_PPMD_UNIT, k);
      }
      gmx_pp_list_push(s, a, i, p, s->indx2units[i]);
    }
  }
  s->glue_count = 1u << (13 + s->glue_count1++);
}

GMX_HD void gmx_pp_split(GmxPpmdState* s, uint8_t* a, uint32_t pv, uint32_t old_i, uint32_t new_i) {
  GMX_PPMD_HIT(GMX_PC_SPLIT);
  uint32_t diff = (uint32_t)s->indx2units[old_i] - s->indx2units[new_i];
  uint32_t p = pv + GMX_PPMD_UNIT * s->indx2units[new_i];
  uint32_t i = s->units2indx[diff - 1];
  if (s->indx2units[i] != diff) {
    const uint32_t k = s->indx2units[--i];
    gmx_pp_list_push(s, a, i, p, k);
    p += GMX_PPMD_UNIT * k;
    diff -= k;
  }
  gmx_pp_list_push(s, a, s->units2indx[diff - 1], p, diff);
}

// 0 when nothing is left
GMX_HD uint32_t gmx_pp_alloc_rare(GmxPpmdState* s, uint8_t* a, uint32_t indx) {
  uint32_t i = indx;
  do {
    if (++i == GMX_PPMD_N_INDEXES) {
      if (!s->glue_count--) {
        gmx_pp_glue(s, a);
        i = indx;
        if (s->blist[i][1]) return gmx_pp_list_pop(s, a, i);
      } else {
        const uint32_t bytes = GMX_PPMD_UNIT * s->indx2units[indx];
        if ((int64_t)s->units_start - (int64_t)s->text > (int64_t)bytes) {
          s->units_start -= bytes;
          return s->units_start;
        }
        GMX_PPMD_HIT(GMX_PC_RARE_NULL);
        return 0;
      }
    }
  } while (!s->blist[i][1]);
  const uint32_t r = gmx_pp_list_pop(s, a, i);
  gmx_pp_split(s, a, r, i, indx);
  return r;
}

GMX_HD uint32_t gmx_pp_alloc_units(GmxPpmdState* s, uint8_t* a, uint32_t nu) {
  const uint32_t indx = s->units2indx[nu - 1];
  if (s->blist[indx][1]) return gmx_pp_list_pop(s, a, indx);
  const uint32_t bytes = GMX_PPMD_UNIT * s->indx2units[indx];
  if ((uint64_t)s->lo + bytes <= (uint64_t)s->hi) {
    const uint32_t r = s->lo;
    s->lo += bytes;
    return r;
  }
  return gmx_pp_alloc_rare(s, a, indx);
}

GMX_HD uint32_t gmx_pp_alloc_context(GmxPpmdState* s, uint8_t* a) {
  if (s->hi != s->lo) return s->hi -= GMX_PPMD_UNIT;
  return s->blist[0][1] ? gmx_pp_list_pop(s, a, 0) : gmx_pp_alloc_rare(s, a, 0);
}

GMX_HD void gmx_pp_free_units(GmxPpmdState* s, uint8_t* a, uint32_t p, uint32_t nu) {
  const uint32_t indx = s->units2indx[nu - 1];
  gmx_pp_list_push(s, a, indx, p, s->indx2units[indx]);
}

GMX_HD void gmx_pp_free_unit(GmxPpmdState* s, uint8_t* a, uint32_t p) {
  const uint32_t k = (uint64_t)p > (uint64_t)s->units_start + GMX_PPMD_FAR ? 0u : (uint32_t)GMX_PPMD_N_INDEXES;
  gmx_pp_list_push(s, a, k, p, 1);
}

GMX_HD uint32_t gmx_pp_expand_units(GmxPpmdState* s, uint8_t* a, uint32_t old, uint32_t old_nu) {
  const uint32_t i0 = s->units2indx[old_nu - 1], i1 = s->units2indx[old_nu];
  if (i0 == i1) return old;
  GMX_PPMD_HIT(GMX_PC_EXPAND);
  const uint32_t p = gmx_pp_alloc_units(s, a, old_nu + 1);
  if (p) {
    gmx_pp_copy_units(a, p, old, old_nu);
    gmx_pp_list_push(s, a, i0, old, old_nu);
  }
  return p;
}

GMX_HD uint32_t gmx_pp_shrink_units(GmxPpmdState* s, uint8_t* a, uint32_t old, uint32_t old_nu, uint32_t new_nu) {
  const uint32_t i0 = s->units2indx[old_nu - 1], i1 = s->units2indx[new_nu - 1];
  if (i0 == i1) return old;
  if (s->blist[i1][1]) {
    const uint32_t p = gmx_pp_list_pop(s, a, i1);
    gmx_pp_copy_units(a, p, old, new_nu);
    gmx_pp_list_push(s, a, i0, old, s->indx2units[i0]);
    return p;
  }
  gmx_pp_split(s, a, old, i0, i1);
  return old;
}

GMX_HD uint32_t gmx_pp_move_up(GmxPpmdState* s, uint8_t* a, uint32_t old, uint32_t nu) {
  const uint32_t indx = s->units2indx[nu - 1];
  if ((uint64_t)old > (uint64_t)s->units_start + GMX_PPMD_FAR || old > s->blist[indx][1]) return old;
  GMX_PPMD_HIT(GMX_PC_MOVE_UP);
  const uint32_t p = gmx_pp_list_pop(s, a, indx);
  gmx_pp_copy_units(a, p, old, nu);
  gmx_pp_list_push(s, a, GMX_PPMD_N_INDEXES, old, s->indx2units[indx]);
  return p;
}

GMX_HD void gmx_pp_prepare_text(GmxPpmdState* s, uint8_t* a) {
  s->aux = gmx_pp_alloc_context(s, a);
  if (!s->aux)
    s->aux = s->units_start;
  else if (s->aux == s->units_start)
    s->aux = (s->units_start += GMX_PPMD_UNIT);
}

GMX_HD void gmx_pp_expand_text(GmxPpmdState* s, uint8_t* a) {
  uint32_t n = 0;
  for (int k = 0; k < GMX_PPMD_N_INDEXES; ++k) s->count[k] = 0;
  if (s->aux != s->units_start) {
    if (gmx_pp_ld32(a, s->aux) != 0xffffffffu)
      s->units_start += GMX_PPMD_UNIT;
    else
      gmx_pp_list_push(s, a, 0, s->aux, 1);
  }
  while (gmx_pp_ld32(a, s->units_start) == 0xffffffffu) {
    const uint32_t b = s->units_start, nu = gmx_pp_ld32(a, b + 8);
    s->units_start = b + GMX_PPMD_UNIT * nu;
    s->count[s->units2indx[nu - 1]]++;
    n++;
    gmx_pp_st32(a, b, 0);
  }
  if (!n) return;
  for (uint32_t p = gmx_pp_head(GMX_PPMD_N_INDEXES); gmx_pp_node_next(s, a, p); p = gmx_pp_node_next(s, a, p)) {
    for (;;) {
      const uint32_t nx = gmx_pp_node_next(s, a, p);
      if (!nx || gmx_pp_ld32(a, nx) != 0) break;
      s->count[s->units2indx[gmx_pp_ld32(a, nx + 8) - 1]]--;
      gmx_pp_node_set_next(s, a, p, gmx_pp_ld32(a, nx + 4));
      s->blist[GMX_PPMD_N_INDEXES][0]--;
    }
    if (!gmx_pp_node_next(s, a, p)) break;
  }
  for (uint32_t k = 0; k < GMX_PPMD_N_INDEXES; ++k) {
    for (uint32_t p = gmx_pp_head(k); s->count[k] != 0; p = gmx_pp_node_next(s, a, p)) {
      for (;;) {
        const uint32_t nx = gmx_pp_node_next(s, a, p);
        if (gmx_pp_ld32(a, nx) != 0) break;
        gmx_pp_node_set_next(s, a, p, gmx_pp_ld32(a, nx + 4));
        s->blist[k][0]--;
        if (!--s->count[k]) break;
      }
    }
  }
}

// ---- the model ----
GMX_HD void gmx_ppmd_tables(GmxPpmdState* s) {
  int i = 0, k = 1;
  for (; i < 4; ++i, k += 1) s->indx2units[i] = (uint8_t)k;
  for (++k; i < 8; ++i, k += 2) s->indx2units[i] = (uint8_t)k;
  for (++k; i < 12; ++i, k += 3) s->indx2units[i] = (uint8_t)k;
  for (++k; i < GMX_PPMD_N_INDEXES; ++i, k += 4) s->indx2units[i] = (uint8_t)k;
  for (k = 0, i = 0; k < 128; ++k) {
    i += s->indx2units[i] < k + 1;
    s->units2indx[k] = (uint8_t)i;
  }
  for (k = 0; k < 256; ++k) s->ns2bs[k] = (uint8_t)(k == 0 ? 0 : k < 3 ? 2 : k < 29 ? 4 : 6);
  for (i = 0; i < 5; ++i) s->qtable[i] = (uint8_t)i;
  int m = 5, step = 1;
  for (k = 1; i < 260; ++i) {
    s->qtable[i] = (uint8_t)m;
    if (!--k) {
      k = ++step;
      m++;
    }
  }
}

GMX_HD void gmx_pp_start_model(GmxPpmdState* s, uint8_t* a) {
  const int esc_coef[12] = {16, -10, 1, 51, 14, 89, 23, 35, 64, 26, -42, 43};
  for (int i = 0; i < 256; ++i) s->char_mask[i] = 0;
  s->esc_count = 1;
  s->order_fall = s->max_order;
  gmx_ppmd_init_allocator(s);
  s->init_rl = -(s->max_order < 13 ? s->max_order : 13);
  s->run_length = s->init_rl;
  const uint32_t c = gmx_pp_alloc_context(s, a);
  s->max_ctx = c;
  const uint32_t st = gmx_pp_alloc_units(s, a, 128);
  gmx_pp_st8(a, c, 255);
  gmx_pp_st8(a, c + 1, 0);
  gmx_pp_st16(a, c + 2, 257);
  gmx_pp_st32(a, c + 4, st);
  gmx_pp_st32(a, c + 8, 0);
  s->prev_success = 0;
  for (uint32_t i = 0; i < 256; ++i) {
    gmx_pp_st8(a, st + 6 * i, i);
    gmx_pp_st8(a, st + 6 * i + 1, 1);
    gmx_pp_set_succ(a, st + 6 * i, 0);
  }
  // the frequency each quantised level starts at, then the binary and the masked SEE contexts
  int k = 0;
  for (int i = 0; i < 25; ++i) {
    while (s->qtable[k] == i) k++;
    const int f = k + 1;
    for (int b = 0; b < 64; ++b) {
      int v = 0;
      for (int j = 0; j < 6; ++j) v += esc_coef[2 * j + ((b >> j) & 1)];
      v = 128 * (v < 32 ? 32 : v > 224 ? 224 : v);
      s->bin_summ[i][b] = (uint16_t)(16384 - v / f);
    }
  }
  for (int i = 0; i < 23; ++i)
    for (int b = 0; b < 32; ++b) {
      s->see2[i][b].shift = 3;
      s->see2[i][b].summ = (uint16_t)((8 * i + 5) << 3);
      s->see2[i][b].count = 7;
    }
}

// A stream as the reference's Init leaves it.  The arena must be zero.
GMX_HD void gmx_ppmd_init(GmxPpmdState* s, uint8_t* a, int order, uint64_t arena_bytes) {
  s->max_order = order;
  s->size = arena_bytes;
  s->found = s->saved_pc = s->aux = 0;
  s->num_masked = s->bsumm = 0;
  s->restores = 0;
  s->last_byte = 0;
  s->pending = 1;
  s->pad_[0] = s->pad_[1] = 0;
  s->dummy_see.summ = 0;
  s->dummy_see.shift = s->dummy_see.count = 0;
  for (int i = 0; i < 256; ++i) s->sqp[i] = 0;
  gmx_ppmd_tables(s);
  gmx_pp_start_model(s, a);
}

GMX_HD void gmx_pp_see_update(GmxPpmdSee* e) {
  if (--e->count == 0) {
    GMX_PPMD_HIT(GMX_PC_SHIFT_RARE);
    uint32_t i = (uint32_t)e->summ >> e->shift;
    i = 7u - (i > 40) - (i > 280) - (i > 1020);
    if (i < e->shift) {
      e->summ = (uint16_t)(e->summ >> 1);
      e->shift--;
    } else if (i > e->shift) {
      e->summ = (uint16_t)(e->summ << 1);
      e->shift++;
    }
    e->count = (uint8_t)(5u << e->shift);
  }
}

// Halves the table of context q with the found state moved to the front; returns the found state's new place.
GMX_HD uint32_t gmx_pp_rescale(GmxPpmdState* s, uint8_t* a, uint32_t q, int order_fall, uint32_t found) {
  GMX_PPMD_HIT(GMX_PC_RESCALE);
  gmx_pp_st8(a, q + 1, GMX_PP_FLAGS(a, q) & 0x14);
  uint32_t flags = GMX_PP_FLAGS(a, q);
  const uint32_t tab = GMX_PP_STATS(a, q);
  {
    const uint32_t t0 = gmx_pp_ld16(a, found), t1 = gmx_pp_ld16(a, found + 2), t2 = gmx_pp_ld16(a, found + 4);
    for (uint32_t p = found; p != tab; p -= 6) gmx_pp_copy_state(a, p, p - 6);
    gmx_pp_st16(a, tab, t0);
    gmx_pp_st16(a, tab + 2, t1);
    gmx_pp_st16(a, tab + 4, t2);
  }
  const int of = order_fall != 0;
  uint32_t p = tab;
  const int f0 = (int)gmx_pp_ld8(a, p + 1);
  int sf = (int)GMX_PP_SUMM(a, q);
  int esc = sf - f0;
  int ns = (int)GMX_PP_NS(a, q);
  int summ = (f0 + of) >> 1;
  gmx_pp_st8(a, p + 1, summ);
  for (int i = 0; i < ns; ++i) {
    p += 6;
    int f = (int)gmx_pp_ld8(a, p + 1);
    esc -= f;
    f = (f + of) >> 1;
    gmx_pp_st8(a, p + 1, f);
    summ += f;
    if (f) flags |= 0x08u * (gmx_pp_ld8(a, p) >= 0x40);
    if (f > (int)gmx_pp_ld8(a, p - 6 + 1)) {
      const uint32_t t0 = gmx_pp_ld16(a, p), t1 = gmx_pp_ld16(a, p + 2), t2 = gmx_pp_ld16(a, p + 4);
      uint32_t p1 = p;
      for (; f > (int)gmx_pp_ld8(a, p1 - 6 + 1); p1 -= 6) gmx_pp_copy_state(a, p1, p1 - 6);
      gmx_pp_st16(a, p1, t0);
      gmx_pp_st16(a, p1 + 2, t1);
      gmx_pp_st16(a, p1 + 4, t2);
    }
  }
  summ &= 0xffff;
  if (gmx_pp_ld8(a, p + 1) == 0) {
    GMX_PPMD_HIT(GMX_PC_RESCALE_ZERO);
    int z = 0;
    for (; gmx_pp_ld8(a, p + 1) == 0; ++z, p -= 6) {
    }
    esc += z;
    const uint32_t old_nu = (uint32_t)(ns + 2) >> 1;
    ns -= z;
    gmx_pp_st8(a, q, ns);
    if (ns == 0) {
      GMX_PPMD_HIT(GMX_PC_RESCALE_FOLD);
      const uint32_t sym = gmx_pp_ld8(a, tab), succ = gmx_pp_succ(a, tab);
      int f = (2 * (int)gmx_pp_ld8(a, tab + 1) + esc - 1) / esc;
      if (f > GMX_PPMD_MAX_FREQ / 3) f = GMX_PPMD_MAX_FREQ / 3;
      gmx_pp_st8(a, q + 1, flags & 0x18);
      gmx_pp_free_units(s, a, tab, old_nu);
      gmx_pp_st8(a, q + 2, sym);
      gmx_pp_st8(a, q + 3, f);
      gmx_pp_st32(a, q + 4, succ);
      return q + 2;
    }
    gmx_pp_st32(a, q + 4, gmx_pp_shrink_units(s, a, tab, old_nu, (uint32_t)(ns + 2) >> 1));
  }
  summ = (summ + ((esc + 1) >> 1)) & 0xffff;
  const uint32_t nt = GMX_PP_STATS(a, q);
  int add;
  if (order_fall || (flags & 0x04) == 0) {
    sf -= esc;
    const int d = sf - f0;
    uint32_t v = (uint32_t)((f0 * summ - sf * (int)gmx_pp_ld8(a, nt + 1) + d - 1) / d);
    add = (int)(v >= 2u ? (v <= GMX_PPMD_MAX_FREQ / 2u - 18u ? v : GMX_PPMD_MAX_FREQ / 2u - 18u) : 2u);
  } else {
    add = 2;
  }
  gmx_pp_st8(a, nt + 1, gmx_pp_ld8(a, nt + 1) + add);
  gmx_pp_st16(a, q + 2, summ + add);
  gmx_pp_st8(a, q + 1, flags | 0x04);
  return nt;
}

// What is left of a frame of the cut once its successors are done.
GMX_HD uint32_t gmx_pp_cut_tail(GmxPpmdState* s, uint8_t* a, uint32_t q) {
  if (q == s->units_start) {
    gmx_pp_copy_units(a, s->aux, q, 1);
    return s->aux;
  }
  if (GMX_PP_SUFFIX(a, q) == s->units_start) gmx_pp_st32(a, q + 8, s->aux);
  return q;
}
GMX_HD uint32_t gmx_pp_cut_binary(GmxPpmdState* s, uint8_t* a, uint32_t q, int order, bool went) {
  bool drop = true;
  if (went && (gmx_pp_ld32(a, q + 4) || order < GMX_PPMD_O_BOUND)) drop = false;
  if (drop) {
    GMX_PPMD_HIT(GMX_PC_CUT_BIN_FREE);
    gmx_pp_free_unit(s, a, q);
    return 0;
  }
  return gmx_pp_cut_tail(s, a, q);
}
GMX_HD uint32_t gmx_pp_cut_table(GmxPpmdState* s, uint8_t* a, uint32_t q, int order, uint32_t p0, int i) {
  int ns = (int)GMX_PP_NS(a, q);
  const uint32_t nu = (uint32_t)(ns + 2) >> 1;
  if (i != ns && order > 0) {
    gmx_pp_st8(a, q, (uint32_t)i);
    if (i < 0) {
      GMX_PPMD_HIT(GMX_PC_CUT_FREE);
      gmx_pp_free_units(s, a, p0, nu);
      gmx_pp_free_unit(s, a, q);
      return 0;
    }
    if (i == 0) {
      GMX_PPMD_HIT(GMX_PC_CUT_FOLD);
      const uint32_t sym = gmx_pp_ld8(a, p0), succ = gmx_pp_succ(a, p0);
      const int f = (int)gmx_pp_ld8(a, p0 + 1);
      gmx_pp_st8(a, q + 1, (GMX_PP_FLAGS(a, q) & 0x10) + 0x08u * (sym >= 0x40));
      const int nf = 1 + (2 * (f - 1)) / ((int)GMX_PP_SUMM(a, q) - f);
      gmx_pp_st8(a, q + 2, sym);
      gmx_pp_st8(a, q + 3, nf);
      gmx_pp_st32(a, q + 4, succ);
      // (the reference stores the new frequency in the table first; the table is freed next)
      gmx_pp_st8(a, p0 + 1, nf);
      gmx_pp_free_units(s, a, p0, nu);
    } else {
      const uint32_t p = gmx_pp_shrink_units(s, a, p0, nu, (uint32_t)(i + 2) >> 1);
      gmx_pp_st32(a, q + 4, p);
      const int summ0 = (int)GMX_PP_SUMM(a, q);
      const int scale = summ0 > 16 * i;
      uint32_t flags = GMX_PP_FLAGS(a, q) & (0x10u + 0x04u * (uint32_t)scale);
      if (scale) {
        GMX_PPMD_HIT(GMX_PC_CUT_RESCALE);
        int esc = summ0, summ = 0;
        for (int k = 0; k <= i; ++k) {
          int f = (int)gmx_pp_ld8(a, p + 6 * k + 1);
          esc -= f;
          f = (f + 1) >> 1;
          gmx_pp_st8(a, p + 6 * k + 1, f);
          summ += f;
          flags |= 0x08u * (gmx_pp_ld8(a, p + 6 * k) >= 0x40);
        }
        esc = (esc + 1) >> 1;
        gmx_pp_st16(a, q + 2, summ + esc);
      } else {
        for (int k = 0; k <= i; ++k) flags |= 0x08u * (gmx_pp_ld8(a, p + 6 * k) >= 0x40);
      }
      gmx_pp_st8(a, q + 1, flags);
    }
  }
  return gmx_pp_cut_tail(s, a, q);
}

// cutOff from the root: drops every branch that still points into the text, down to the model's order.  The
// reference's recursion is the frame stack; a frame's order is its depth.
GMX_HD uint32_t gmx_pp_cut_off(GmxPpmdState* s, uint8_t* a, uint32_t root) {
  int d = 0;
  uint32_t r = 0;
  s->frame[0].q = root;
  bool enter = true;
  for (;;) {
    bool done = false;  // frame d has its value in r
    if (enter) {
      GMX_PPMD_HIT(GMX_PC_CUTOFF);
      const uint32_t q = s->frame[d].q;
      const uint32_t ns = GMX_PP_NS(a, q);
      if (ns == 0) {
        const uint32_t succ = gmx_pp_ld32(a, q + 4);
        if (succ >= s->units_start) {
          if (d < s->max_order) {
            s->frame[d].pi = -1;
            s->frame[++d].q = succ;
            continue;
          }
          gmx_pp_st32(a, q + 4, 0);
          r = gmx_pp_cut_binary(s, a, q, d, true);
        } else {
          r = gmx_pp_cut_binary(s, a, q, d, false);
        }
        done = true;
      } else {
        const uint32_t p0 = gmx_pp_move_up(s, a, GMX_PP_STATS(a, q), (ns + 2) >> 1);
        gmx_pp_st32(a, q + 4, p0);
        s->frame[d].p0 = p0;
        s->frame[d].i = (int32_t)ns;
        s->frame[d].pi = (int32_t)ns;
      }
    }
    if (!done) {
      // the table of frame d, from its last state down
      const uint32_t q = s->frame[d].q, p0 = s->frame[d].p0;
      int i = s->frame[d].i, pi = s->frame[d].pi;
      bool down = false;
      while (pi >= 0) {
        const uint32_t p = p0 + 6u * (uint32_t)pi;
        const uint32_t succ = gmx_pp_succ(a, p);
        if (succ < s->units_start) {
          gmx_pp_set_succ(a, p, 0);
          gmx_pp_swap_states(a, p, p0 + 6u * (uint32_t)i);
          i--;
        } else if (d < s->max_order) {
          s->frame[d].i = i;
          s->frame[d].pi = pi;
          s->frame[++d].q = succ;
          down = true;
          break;
        } else {
          gmx_pp_set_succ(a, p, 0);
        }
        pi--;
      }
      if (down) {
        enter = true;
        continue;
      }
      r = gmx_pp_cut_table(s, a, q, d, p0, i);
    }
    // frame d returns r to the frame below
    for (;;) {
      if (d == 0) return r;
      --d;
      const uint32_t q = s->frame[d].q;
      if (s->frame[d].pi != -1) break;
      gmx_pp_st32(a, q + 4, r);
      r = gmx_pp_cut_binary(s, a, q, d, true);
    }
    gmx_pp_set_succ(a, s->frame[d].p0 + 6u * (uint32_t)s->frame[d].pi, r);
    s->frame[d].pi--;
    enter = false;
  }
}

// The model flush: the arena is full.
GMX_HD void gmx_pp_restore_model(GmxPpmdState* s, uint8_t* a) {
  GMX_PPMD_HIT(GMX_PC_RESTORE);
  s->restores++;
  s->text = 0;
  for (;; s->max_ctx = GMX_PP_SUFFIX(a, s->max_ctx)) {
    const uint32_t c = s->max_ctx;
    if (GMX_PP_NS(a, c) != 1 || c == s->saved_pc) break;
    const uint32_t p = GMX_PP_STATS(a, c);
    if (gmx_pp_succ(a, p + 6) >= s->units_start) break;
    const uint32_t sym = gmx_pp_ld8(a, p), f = (gmx_pp_ld8(a, p + 1) + 1) >> 1, succ = gmx_pp_succ(a, p);
    gmx_pp_st8(a, c + 1, (GMX_PP_FLAGS(a, c) & 0x10) + 0x08u * (sym >= 0x40));
    gmx_pp_st8(a, p + 1, f);
    gmx_pp_st8(a, c + 2, sym);
    gmx_pp_st8(a, c + 3, f);
    gmx_pp_st32(a, c + 4, succ);
    gmx_pp_st8(a, c, 0);
    gmx_pp_free_units(s, a, p, 1);
  }
  while (GMX_PP_SUFFIX(a, s->max_ctx)) s->max_ctx = GMX_PP_SUFFIX(a, s->max_ctx);
  s->aux = s->units_start;
  gmx_pp_expand_text(s, a);
  do {
    gmx_pp_prepare_text(s, a);
    gmx_pp_cut_off(s, a, s->max_ctx);
    gmx_pp_expand_text(s, a);
  } while (gmx_ppmd_used_memory(s) > 3 * (s->size >> 2));
  s->glue_count = s->glue_count1 = 0;
  s->order_fall = s->max_order;
}

// The state of `sym` in the table of context c (it is there).
GMX_HD uint32_t gmx_pp_find(const uint8_t* a, uint32_t c, uint32_t sym) {
  GMX_PPMD_SCAN(GMX_PP_NS(a, c) + 1);
  uint32_t p = GMX_PP_STATS(a, c);
  while (gmx_pp_ld8(a, p) != sym) p += 6;
  return p;
}

// New contexts for the found state's text branch, one per order from pc up.  0 when the arena is full.
GMX_HD uint32_t gmx_pp_create_successors(GmxPpmdState* s, uint8_t* a, bool skip, uint32_t p, uint32_t pc) {
  int n = 0;
  uint32_t sym = gmx_pp_ld8(a, s->found);
  const uint32_t up_branch = gmx_pp_succ(a, s->found);
  bool walk = true;
  if (!skip) {
    s->ps[n++] = s->found;
    if (!GMX_PP_SUFFIX(a, pc)) walk = false;
  }
  if (walk) {
    bool entry = false;
    if (p) {
      pc = GMX_PP_SUFFIX(a, pc);
      entry = true;
    }
    do {
      if (!entry) {
        pc = GMX_PP_SUFFIX(a, pc);
        if (GMX_PP_NS(a, pc)) {
          p = gmx_pp_find(a, pc, sym);
          const uint32_t f = gmx_pp_ld8(a, p + 1);
          const uint32_t t = 2u * (f < GMX_PPMD_MAX_FREQ - 1);
          gmx_pp_st8(a, p + 1, f + t);
          gmx_pp_st16(a, pc + 2, GMX_PP_SUMM(a, pc) + t);
        } else {
          p = pc + 2;
          const uint32_t f = gmx_pp_ld8(a, p + 1);
          gmx_pp_st8(a, p + 1, f + ((GMX_PP_NS(a, GMX_PP_SUFFIX(a, pc)) == 0) & (f < 16)));
        }
      }
      entry = false;
      if (gmx_pp_succ(a, p) != up_branch) {
        pc = gmx_pp_succ(a, p);
        break;
      }
      s->ps[n++] = p;
    } while (GMX_PP_SUFFIX(a, pc));
  }
  if (n == 0) return pc;
  // the symbol that follows in the text
  uint32_t flags = 0x10u * (sym >= 0x40);
  sym = gmx_pp_ld8(a, up_branch);
  flags |= 0x08u * (sym >= 0x40);
  uint32_t freq;
  if (GMX_PP_NS(a, pc)) {
    const uint32_t q = gmx_pp_find(a, pc, sym);
    uint32_t cf = gmx_pp_ld8(a, q + 1) - 1;
    const uint32_t s0 = GMX_PP_SUMM(a, pc) - GMX_PP_NS(a, pc) - cf;
    cf = 1 + ((2 * cf < s0) ? (uint32_t)(12 * cf > s0) : 2 + cf / s0);
    freq = cf < 7 ? cf : 7;
  } else {
    freq = gmx_pp_ld8(a, pc + 3);
  }
  const uint32_t w0 = (flags << 8) | (sym << 16) | (freq << 24);
  do {
    const uint32_t c = gmx_pp_alloc_context(s, a);
    if (!c) return 0;
    gmx_pp_st32(a, c, w0);
    gmx_pp_st32(a, c + 4, up_branch + 1);
    gmx_pp_st32(a, c + 8, pc);
    pc = c;
    gmx_pp_set_succ(a, s->ps[--n], pc);
  } while (n != 0);
  return pc;
}

GMX_HD uint32_t gmx_pp_reduce_order(GmxPpmdState* s, uint8_t* a, uint32_t p, uint32_t pc) {
  GMX_PPMD_HIT(GMX_PC_REDUCE_ORDER);
  const uint32_t pc1 = pc;
  gmx_pp_set_succ(a, s->found, s->text);
  const uint32_t sym = gmx_pp_ld8(a, s->found);
  const uint32_t up_branch = s->text;
  s->order_fall++;
  bool entry = false;
  if (p) {
    pc = GMX_PP_SUFFIX(a, pc);
    entry = true;
  }
  for (;;) {
    if (!entry) {
      if (!GMX_PP_SUFFIX(a, pc)) return pc;
      pc = GMX_PP_SUFFIX(a, pc);
      if (GMX_PP_NS(a, pc)) {
        p = gmx_pp_find(a, pc, sym);
        const uint32_t f = gmx_pp_ld8(a, p + 1);
        const uint32_t t = 2u * (f < GMX_PPMD_MAX_FREQ - 3);
        gmx_pp_st8(a, p + 1, f + t);
        gmx_pp_st16(a, pc + 2, GMX_PP_SUMM(a, pc) + t);
      } else {
        p = pc + 2;
        const uint32_t f = gmx_pp_ld8(a, p + 1);
        gmx_pp_st8(a, p + 1, f + (f < 11));
      }
    }
    entry = false;
    if (gmx_pp_succ(a, p)) break;
    gmx_pp_set_succ(a, p, up_branch);
    s->order_fall++;
  }
  if (gmx_pp_succ(a, p) <= up_branch) {
    const uint32_t keep = s->found;
    s->found = p;
    const uint32_t r = gmx_pp_create_successors(s, a, false, 0, pc);
    gmx_pp_set_succ(a, p, r);
    s->found = keep;
  }
  if (s->order_fall == 1 && pc1 == s->max_ctx) {
    gmx_pp_set_succ(a, s->found, gmx_pp_succ(a, p));
    s->text--;
  }
  return gmx_pp_succ(a, p);
}

// UpdateModel: returns the new MaxContext, or 0 with saved_pc set when the arena is full.
GMX_HD uint32_t gmx_pp_update_model(GmxPpmdState* s, uint8_t* a, uint32_t min_ctx) {
  const uint32_t fsym = gmx_pp_ld8(a, s->found), ffreq = gmx_pp_ld8(a, s->found + 1);
  uint32_t fsucc = gmx_pp_succ(a, s->found);
  uint32_t p = 0;
  uint32_t pc;
  if (GMX_PP_SUFFIX(a, min_ctx)) {
    pc = GMX_PP_SUFFIX(a, min_ctx);
    if (GMX_PP_NS(a, pc)) {
      GMX_PPMD_SCAN(GMX_PP_NS(a, pc) + 1);
      p = GMX_PP_STATS(a, pc);
      if (gmx_pp_ld8(a, p) != fsym) {
        for (p += 6; gmx_pp_ld8(a, p) != fsym; p += 6) {
        }
        if (gmx_pp_ld8(a, p + 1) >= gmx_pp_ld8(a, p - 6 + 1)) {
          gmx_pp_swap_states(a, p, p - 6);
          p -= 6;
        }
      }
      const uint32_t f = gmx_pp_ld8(a, p + 1);
      if (f < GMX_PPMD_MAX_FREQ - 3) {
        const uint32_t cf = 2 + (ffreq < 28);
        gmx_pp_st8(a, p + 1, f + cf);
        gmx_pp_st16(a, pc + 2, GMX_PP_SUMM(a, pc) + cf);
      }
    } else {
      p = pc + 2;
      const uint32_t f = gmx_pp_ld8(a, p + 1);
      gmx_pp_st8(a, p + 1, f + (f < 14));
    }
  }
  pc = s->max_ctx;
  bool full_order = !s->order_fall && fsucc;
  if (!full_order) {
    gmx_pp_st8(a, s->text++, fsym);
    if (s->text >= s->units_start) {
      GMX_PPMD_HIT(GMX_PC_TEXT_FULL);
      s->saved_pc = pc;
      return 0;
    }
  } else {
    GMX_PPMD_HIT(GMX_PC_FULL_ORDER);
  }
  uint32_t succ = s->text;
  if (fsucc) {
    if (full_order || fsucc < s->units_start) {
      const uint32_t r = gmx_pp_create_successors(s, a, full_order, p, min_ctx);
      if (full_order) {
        gmx_pp_set_succ(a, s->found, r);
        if (!r) {
          s->saved_pc = pc;
          return 0;
        }
        s->max_ctx = r;
        return r;
      }
      fsucc = r;
    }
  } else {
    fsucc = gmx_pp_reduce_order(s, a, p, min_ctx);
  }
  if (!fsucc) {
    s->saved_pc = pc;
    return 0;
  }
  if (!--s->order_fall) {
    succ = fsucc;
    s->text -= (s->max_ctx != min_ctx);
  }
  const uint32_t s0 = GMX_PP_SUMM(a, min_ctx) - ffreq;
  const uint32_t ns = GMX_PP_NS(a, min_ctx);
  const uint32_t flag = 0x08u * (fsym >= 0x40);
  for (pc = s->max_ctx; pc != min_ctx; pc = GMX_PP_SUFFIX(a, pc)) {
    const uint32_t ns1 = GMX_PP_NS(a, pc);
    uint32_t summ;
    if (ns1) {
      if (ns1 & 1) {
        p = gmx_pp_expand_units(s, a, GMX_PP_STATS(a, pc), (ns1 + 1) >> 1);
        if (!p) {
          s->saved_pc = pc;
          return 0;
        }
        gmx_pp_st32(a, pc + 4, p);
      }
      summ = GMX_PP_SUMM(a, pc) + (s->qtable[ns + 4] >> 3);
    } else {
      GMX_PPMD_HIT(GMX_PC_BIN_TO_TWO);
      p = gmx_pp_alloc_units(s, a, 1);
      if (!p) {
        s->saved_pc = pc;
        return 0;
      }
      const uint32_t sym = gmx_pp_ld8(a, pc + 2), sc = gmx_pp_ld32(a, pc + 4);
      uint32_t f = gmx_pp_ld8(a, pc + 3);
      f = f <= GMX_PPMD_MAX_FREQ / 3 ? 2 * f - 1 : GMX_PPMD_MAX_FREQ - 15;
      gmx_pp_st8(a, p, sym);
      gmx_pp_st8(a, p + 1, f);
      gmx_pp_set_succ(a, p, sc);
      gmx_pp_st32(a, pc + 4, p);
      const uint8_t exp_escape[16] = {51, 43, 18, 12, 11, 9, 8, 7, 6, 5, 4, 3, 3, 2, 2, 2};
      summ = f + (ns > 1) + exp_escape[s->qtable[s->bsumm >> 8]];
    }
    summ &= 0xffffu;
    uint32_t cf = (ffreq - 1) * (5 + summ);
    const uint32_t sf = s0 + summ;
    if (cf <= 3 * sf) {
      cf = 1 + (2 * cf > sf) + (2 * cf > 3 * sf);
      summ += 4;
    } else {
      cf = 5 + (cf > 5 * sf) + (cf > 6 * sf) + (cf > 8 * sf) + (cf > 10 * sf) + (cf > 12 * sf);
      summ += cf;
    }
    gmx_pp_st16(a, pc + 2, summ);
    const uint32_t nn = ns1 + 1;
    gmx_pp_st8(a, pc, nn);
    p = GMX_PP_STATS(a, pc) + 6 * nn;
    gmx_pp_set_succ(a, p, succ);
    gmx_pp_st8(a, p, fsym);
    gmx_pp_st8(a, p + 1, cf);
    gmx_pp_st8(a, pc + 1, GMX_PP_FLAGS(a, pc) | flag);
  }
  s->max_ctx = fsucc;
  return fsucc;
}

GMX_HD uint16_t* gmx_pp_bin_slot(GmxPpmdState* s, const uint8_t* a, uint32_t q) {
  const uint32_t i = s->ns2bs[GMX_PP_NS(a, GMX_PP_SUFFIX(a, q))] + (uint32_t)s->prev_success + GMX_PP_FLAGS(a, q) +
                     (((uint32_t)s->run_length >> 26) & 0x20u);
  return &s->bin_summ[s->qtable[gmx_pp_ld8(a, q + 3) - 1]][i];
}

GMX_HD GmxPpmdSee* gmx_pp_see_of(GmxPpmdState* s, const uint8_t* a, uint32_t q, int* see_freq) {
  const uint32_t cnum = GMX_PP_NS(a, q);
  if (cnum == 0xff) {
    *see_freq = 1;
    return &s->dummy_see;
  }
  GmxPpmdSee* e = s->see2[s->qtable[cnum + 3] - 4];
  e += (GMX_PP_SUMM(a, q) > 10 * (cnum + 1));
  e += 2 * (2 * cnum < GMX_PP_NS(a, GMX_PP_SUFFIX(a, q)) + (uint32_t)s->num_masked) + GMX_PP_FLAGS(a, q);
  *see_freq = (int)((uint32_t)e->summ >> e->shift) + 1;
  return e;
}

// ppmd_UpdateByte: the model learns byte c.
GMX_HD void gmx_ppmd_update_byte(GmxPpmdState* s, uint8_t* a, uint32_t c) {
  uint32_t mc = s->max_ctx;
  if (GMX_PP_NS(a, mc)) {
    // the unmasked context
    const uint32_t cnum = GMX_PP_NS(a, mc);
    GMX_PPMD_SCAN(cnum + 1);
    const uint32_t tab = GMX_PP_STATS(a, mc);
    s->prev_success = 0;
    uint32_t p = 0;
    if (gmx_pp_ld8(a, tab) == c) {
      gmx_pp_st8(a, tab + 1, gmx_pp_ld8(a, tab + 1) + 4);
      gmx_pp_st16(a, mc + 2, GMX_PP_SUMM(a, mc) + 4);
      p = tab;
    } else {
      uint32_t i = 1;
      for (; i <= cnum; ++i)
        if (gmx_pp_ld8(a, tab + 6 * i) == c) break;
      if (i <= cnum) {
        p = tab + 6 * i;
        gmx_pp_st8(a, p + 1, gmx_pp_ld8(a, p + 1) + 4);
        gmx_pp_st16(a, mc + 2, GMX_PP_SUMM(a, mc) + 4);
        if (gmx_pp_ld8(a, p + 1) > gmx_pp_ld8(a, p - 6 + 1)) {
          gmx_pp_swap_states(a, p, p - 6);
          p -= 6;
        }
      } else {
        s->num_masked = (int32_t)cnum;
        for (i = 0; i <= cnum; ++i) s->char_mask[gmx_pp_ld8(a, tab + 6 * i)] = s->esc_count;
      }
    }
    s->found = p;
    if (p && gmx_pp_ld8(a, p + 1) > GMX_PPMD_MAX_FREQ) s->found = gmx_pp_rescale(s, a, mc, s->order_fall, p);
  } else {
    GMX_PPMD_HIT(GMX_PC_BIN_UPDATE);
    uint16_t* bs = gmx_pp_bin_slot(s, a, mc);
    s->bsumm = *bs;
    *bs = (uint16_t)(*bs - ((s->bsumm + 64) >> 7));
    const uint32_t sym = gmx_pp_ld8(a, mc + 2);
    if (sym != c) {
      s->char_mask[sym] = s->esc_count;
      s->num_masked = 0;
      s->prev_success = 0;
      s->found = 0;
    } else {
      *bs = (uint16_t)(*bs + 128);
      const uint32_t f = gmx_pp_ld8(a, mc + 3);
      gmx_pp_st8(a, mc + 3, f + (f < 196));
      s->run_length++;
      s->prev_success = 1;
      s->found = mc + 2;
    }
  }
  while (!s->found) {
    do {
      s->order_fall++;
      mc = GMX_PP_SUFFIX(a, mc);
    } while ((int32_t)GMX_PP_NS(a, mc) == s->num_masked);
    // a masked context
    const uint32_t cnum = GMX_PP_NS(a, mc);
    GMX_PPMD_SCAN(cnum + 1);
    int see_freq;
    GmxPpmdSee* e = gmx_pp_see_of(s, a, mc, &see_freq);
    const uint32_t tab = GMX_PP_STATS(a, mc);
    int low = 0;
    uint32_t hit = 0;
    for (uint32_t i = 0; i <= cnum; ++i) {
      const uint32_t sym = gmx_pp_ld8(a, tab + 6 * i);
      if (s->char_mask[sym] != s->esc_count) {
        s->char_mask[sym] = s->esc_count;
        low += (int)gmx_pp_ld8(a, tab + 6 * i + 1);
        if (sym == c) hit = tab + 6 * i;
      }
    }
    const int total = see_freq + low;
    if (hit) {
      if (see_freq > 2) e->summ = (uint16_t)(e->summ - see_freq);
      gmx_pp_see_update(e);
      s->found = hit;
      gmx_pp_st8(a, hit + 1, gmx_pp_ld8(a, hit + 1) + 4);
      gmx_pp_st16(a, mc + 2, GMX_PP_SUMM(a, mc) + 4);
      if (gmx_pp_ld8(a, hit + 1) > GMX_PPMD_MAX_FREQ) s->found = gmx_pp_rescale(s, a, mc, s->order_fall, hit);
      s->run_length = s->init_rl;
      s->esc_count++;
    } else {
      s->num_masked = (int32_t)cnum;
      e->summ = (uint16_t)(e->summ + (total - see_freq));
    }
  }
  uint32_t next;
  if (s->order_fall != 0 || gmx_pp_succ(a, s->found) < s->units_start) {
    next = gmx_pp_update_model(s, a, mc);
    if (next) s->max_ctx = next;
  } else {
    next = s->max_ctx = gmx_pp_succ(a, s->found);
  }
  if (!next) gmx_pp_restore_model(s, a);
}

GMX_HD uint32_t gmx_pp_scale(uint32_t cum, uint32_t freq, uint32_t total) {
  return (uint32_t)(((uint64_t)cum * (uint64_t)(freq & 0xffffu)) / (uint64_t)(total & 0xffffu));
}

// ppmd_PrepareByte with ConvertSQ's sqp: the model itself stays as it is.  A context's symbols all scale by the cum
// its predecessors' escapes left; the escape is the context's last entry.
GMX_HD void gmx_ppmd_prepare_byte(GmxPpmdState* s, const uint8_t* a) {
  for (int i = 0; i < 256; ++i) s->sqp[i] = 0;
  uint32_t cum = 0xffffff00u;
  s->num_masked = 0;
  uint32_t mc = s->max_ctx;
  if (GMX_PP_NS(a, mc)) {
    const uint32_t cnum = GMX_PP_NS(a, mc), tab = GMX_PP_STATS(a, mc), total = GMX_PP_SUMM(a, mc);
    uint32_t low = 0;
    for (uint32_t i = 0; i <= cnum; ++i) {
      const uint32_t sym = gmx_pp_ld8(a, tab + 6 * i), f = gmx_pp_ld8(a, tab + 6 * i + 1);
      s->sqp[sym] = gmx_pp_scale(cum, f, total) + 1;
      low += f;
      s->char_mask[sym] = s->esc_count;
    }
    s->num_masked = (int32_t)cnum;
    cum = gmx_pp_scale(cum, total - low, total);
  } else {
    s->bsumm = *gmx_pp_bin_slot(s, a, mc);
    const uint32_t sym = gmx_pp_ld8(a, mc + 2), b2 = (uint32_t)(s->bsumm + s->bsumm);
    s->sqp[sym] = gmx_pp_scale(cum, b2, 32768u) + 1;
    cum = gmx_pp_scale(cum, 32768u - b2, 32768u);
    s->char_mask[sym] = s->esc_count;
    s->num_masked = 0;
  }
  for (;;) {
    bool end = false;
    do {
      if (!GMX_PP_SUFFIX(a, mc)) {
        end = true;
        break;
      }
      mc = GMX_PP_SUFFIX(a, mc);
    } while ((int32_t)GMX_PP_NS(a, mc) == s->num_masked);
    if (end) break;
    int see_freq;
    (void)gmx_pp_see_of(s, a, mc, &see_freq);
    const uint32_t cnum = GMX_PP_NS(a, mc), tab = GMX_PP_STATS(a, mc);
    uint32_t low = 0;
    for (uint32_t i = 0; i <= cnum; ++i)
      if (s->char_mask[gmx_pp_ld8(a, tab + 6 * i)] != s->esc_count) low += gmx_pp_ld8(a, tab + 6 * i + 1);
    const uint32_t total = (uint32_t)see_freq + low;
    for (uint32_t i = 0; i <= cnum; ++i) {
      const uint32_t sym = gmx_pp_ld8(a, tab + 6 * i);
      if (s->char_mask[sym] != s->esc_count) {
        s->sqp[sym] = gmx_pp_scale(cum, gmx_pp_ld8(a, tab + 6 * i + 1), total) + 1;
        s->char_mask[sym] = s->esc_count;
      }
    }
    cum = gmx_pp_scale(cum, (uint32_t)see_freq, total);
    s->num_masked = (int32_t)cnum;
  }
  s->esc_count++;
  s->num_masked = 0;
}

// ModPPMD::Predict's byte distribution out of sqp: float(max(sqp, 1)), a left-to-right float sum from 0, one true
// division per element.
GMX_HD float gmx_ppmd_weight(uint32_t sqp) {
  const float f = (float)sqp;
  return f < 1.0f ? 1.0f : f;
}
GMX_HD void gmx_ppmd_normalise(const uint32_t* sqp, float* ppm) {
  float sum = 0.0f;
  for (int i = 0; i < 256; ++i) sum += gmx_ppmd_weight(sqp[i]);
  for (int i = 0; i < 256; ++i) ppm[i] = gmx_ppmd_weight(sqp[i]) / sum;
}

// One byte of ModPPMD::Predict at a byte boundary: the byte coded last is handed in (the bank's per-byte surface,
// gmx_ppmd_step).  The model is then ahead of the bank's records: the next record owes no update.
GMX_HD void gmx_ppmd_byte(GmxPpmdState* s, uint8_t* a, uint32_t last_byte, float* ppm) {
  gmx_ppmd_update_byte(s, a, last_byte);
  gmx_ppmd_prepare_byte(s, a);
  gmx_ppmd_normalise(s->sqp, ppm);
  s->pending = 0;
}

// One record of the bank's batches: `byte` is the byte being CODED under the distribution asked for, as in the LSTM
// bank's records.  The update the model still owes is that of the byte before it -- 0 for a new model, as a new
// Predictor's first Predict hands in; none right behind gmx_ppmd_byte -- and this record's byte is owed next.
GMX_HD void gmx_ppmd_record(GmxPpmdState* s, uint8_t* a, uint32_t byte, float* ppm) {
  if (s->pending) gmx_ppmd_update_byte(s, a, s->last_byte);
  gmx_ppmd_prepare_byte(s, a);
  gmx_ppmd_normalise(s->sqp, ppm);
  s->last_byte = (uint8_t)byte;
  s->pending = 1;
}

#endif  // GMX_PPMD_H_
