// gmx_ctx.hip -- the context banks on the device: BasicContexts' context fields, IntervalContext, SkipContext and
// IndirectHash (contexts/*.cpp of the reference) for S streams, computed from the coded bits alone.
//
// A run of n bits is three launches on the bank's stream:
//   gmx_ctx_chain_kernel   the only sequential part: lane = (stream, IndirectHash variable) walks the run's byte
//                          openings through its table and leaves the variable's value at every opening in a scratch
//                          array [S][openings][H]
//   gmx_ctx_expand_kernel  everything else, parallel: block = (32 bytes of one stream); bytes are assembled from the
//                          bits, the stateless variables computed per byte, a byte's V values staged in LDS, and the
//                          eight bit records of every byte stored into up to three record batches with lanes running
//                          along a record's columns
//   gmx_ctx_commit_kernel  the board for the run's end (ring, recent_bits, values): a launch of its own because every
//                          block of the expand kernel reads the board of the run's beginning
// In the lock-step chain (gmx_chainstep_attach_ctx) a coded bit is one launch instead: gmx_ctx_step_kernel, a wave per
// stream around gmx_ctx_step.h, which leaves the board and the tables as a run over the same bits does; the per-bit
// surface (gmx_ctx_forward / gmx_ctx_learn) is the same step for one stream, gmx_ctx_bit_kernel.
//
// Geometry of a run.  The board holds recent_bits as of the stream's newest Predict and new_bit, the bit coded since
// (basic-contexts.cpp:28-34 runs at the NEXT Predict).  p = 2 recent_bits + new_bit is what record 0 sees before the
// ">= 256" test, nb0 = floor(log2 p) the bits of the open byte.  In "q space" position x < nb0 is a bit of p, position
// nb0 + t is bit t of the run; record t lies in byte slot (nb0 + t) / 8, slot j >= 1 opens with byte B[j] =
// q-space bits [8 j - 8, 8 j) completed, and B[c] for c <= 0 is ring[pos + c]: GetRecentByte(k) at slot j is
// B[j - k].  The very first Predict of a stream (first_prediction_) opens slot 0 with nothing completed.
#include <hip/hip_runtime.h>

#include "gmx_ckpt_walk.h"
#include "gmx_ctx.h"
#include "gmx_ctx_step.h"

namespace {

struct Geo {
  uint32_t p, nb0, fo, pos;
  uint32_t n, jmax;  // bits of the run; its last byte slot
};
__device__ __forceinline__ Geo run_geo(const GmxCtxBoard* b, uint32_t n) {
  Geo g;
  const uint32_t fp = b->first_prediction, rb = b->recent_bits;
  g.p = fp ? rb : 2u * rb + b->new_bit;
  g.nb0 = 31u - (uint32_t)__clz((int)g.p);
  g.fo = (fp && rb == 1u) ? 0u : 1u;  // slot j is byte opening j - fo of the run
  g.pos = b->pos;
  g.n = n;
  g.jmax = (g.nb0 + n - 1u) / 8u;
  return g;
}
__device__ __forceinline__ uint32_t qbit(const Geo& g, const uint8_t* bits, uint32_t x) {
  return x < g.nb0 ? (g.p >> (g.nb0 - 1u - x)) & 1u : (uint32_t)bits[x - g.nb0];
}
// B[c]: c >= 1 a byte the run completes (c <= jmax), c <= 0 a byte of the ring (c > -GMX_CTX_RING)
__device__ __forceinline__ uint32_t byte_at(const Geo& g, const GmxCtxBoard* b, const uint8_t* bits, int c) {
  if (c <= 0) return b->ring[(g.pos + (uint32_t)(GMX_CTX_RING + c)) % GMX_CTX_RING];
  uint32_t v = 0;
  const uint32_t x0 = 8u * (uint32_t)(c - 1);
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) v = (v << 1) | qbit(g, bits, x0 + i);
  return v;
}

__device__ __forceinline__ uint32_t run_bits(const GmxCtxRunArgs& a, int s) {
  return (uint32_t)(a.T_list ? a.T_list[s] : a.T);
}

}  // namespace

// ---- the chain ------------------------------------------------------------------------------------------------
// IndirectHash::Predict at a byte opening (indirect-hash.cpp:18-30): the entry at the OLD outer_hash_ takes the byte,
// outer_context_ / outer_hash_ move, the entry at the NEW index is hashed.  The lane keeps `cur`, the entry at its
// current index, in a register: the next opening's read-modify-write is this opening's load.  A table belongs to one
// lane, so the load behind a store to the same entry is one lane's program order; when old and new index are equal
// nothing is loaded at all.
__global__ __launch_bounds__(64) void gmx_ctx_chain_kernel(const GmxCtxDev* __restrict__ dv, GmxCtxRunArgs a) {
  const int lane = (int)threadIdx.x;
  const int s = (int)blockIdx.x * 4 + lane / GMX_CTX_MAX_HASH, h = lane % GMX_CTX_MAX_HASH;
  if (s >= a.n_streams || h >= dv->h) return;  // (no barrier below: lanes beyond S and H touch no memory)
  const uint32_t n = run_bits(a, s);
  if (n == 0) return;
  uint8_t* bank = a.banks + (size_t)s * dv->bank_bytes;
  const GmxCtxBoard* bd = (const GmxCtxBoard*)(bank + dv->board_off);
  const uint8_t* bits = a.bits + (size_t)s * a.rec_stride;
  const Geo g = run_geo(bd, n);
  const uint32_t fires = g.jmax + 1u - g.fo;
  if (fires == 0) return;
  const GmxCtxHashDev hd = dv->hash[h];
  uint32_t* tab = (uint32_t*)(bank + hd.tab_off);
  GmxCtxHashState* hs = (GmxCtxHashState*)(bank + dv->hstate_off) + h;
  uint64_t oc = hs->outer_context;
  uint32_t oh = hs->outer_hash;
  uint32_t idx = oh % hd.table_size;
  uint32_t cur = tab[idx];
  uint32_t* out = a.scratch + (size_t)s * a.max_fires * (size_t)dv->h + h;
  for (uint32_t f = 0; f < fires; ++f) {
    const uint32_t lb = byte_at(g, bd, bits, (int)(f + g.fo));
    cur = ((cur & hd.inner_mask) << 8) + lb;
    tab[idx] = cur;
    oc = ((oc & (uint64_t)hd.outer_mask) << 8) + lb;
    oh = gmx_ctx_murmur8(oc);
    const uint32_t idx2 = oh % hd.table_size;
    if (idx2 != idx) {
      idx = idx2;
      cur = tab[idx];
    }
    out[(size_t)f * dv->h] = gmx_ctx_murmur4(cur);
  }
  hs->outer_context = oc;
  hs->outer_hash = oh;
}

// ---- the expansion --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmx_ctx_expand_kernel(const GmxCtxDev* __restrict__ dv, GmxCtxRunArgs a) {
  const int s = (int)blockIdx.y, tid = (int)threadIdx.x;
  const uint32_t n = run_bits(a, s);
  if (n == 0) return;
  uint8_t* bank = a.banks + (size_t)s * dv->bank_bytes;
  GmxCtxBoard* bd = (GmxCtxBoard*)(bank + dv->board_off);
  const uint8_t* bits = a.bits + (size_t)s * a.rec_stride;
  const Geo g = run_geo(bd, n);
  const uint32_t j0 = blockIdx.x * GMX_CTX_TILE;
  if (j0 > g.jmax) return;  // (block-uniform)
  const int V = dv->v, H = dv->h;

  __shared__ uint8_t sB[2 * GMX_CTX_TILE];             // B[j0 - 31 + i]
  __shared__ uint8_t sBC[8 * GMX_CTX_TILE];            // bit_context of the tile's records
  __shared__ uint8_t sBit[8 * GMX_CTX_TILE];
  __shared__ uint8_t sPerBit[GMX_CTX_MAX_VARS];        // the variable moves within a byte: + bit_context
  __shared__ uint32_t sVal[GMX_CTX_TILE][GMX_CTX_MAX_VARS];
  __shared__ int32_t sRoute[3][GMX_CTX_MAX_ROUTE];

  // records of the tile: t in [t_lo, t_hi)
  const int64_t lo64 = 8ll * j0 - (int64_t)g.nb0;
  const uint32_t t_lo = lo64 < 0 ? 0u : (uint32_t)lo64;
  const uint64_t hi64 = 8ull * (j0 + GMX_CTX_TILE) - g.nb0;
  const uint32_t t_hi = hi64 > n ? n : (uint32_t)hi64;
  const uint32_t nrec = t_hi - t_lo;

  if (tid < 2 * GMX_CTX_TILE - 1) {
    const int c = (int)j0 - (GMX_CTX_TILE - 1) + tid;
    sB[tid] = (c <= (int)g.jmax && c > -GMX_CTX_RING) ? (uint8_t)byte_at(g, bd, bits, c) : 0;
  }
  if (tid < V) {
    const int k = dv->var[tid].kind;
    sPerBit[tid] = (k == GMX_CTXK_BIT_CONTEXT || k == GMX_CTXK_BYTE_PLUS_RECENT) ? 1 : 0;
  }
  for (int k = 0; k < 3; ++k)
    if (a.tg[k].ctx)
      for (int c = tid; c < a.tg[k].n_cols; c += 256) sRoute[k][c] = a.tg[k].route[c];
  if ((uint32_t)tid < nrec) {
    const uint32_t t = t_lo + tid, q = g.nb0 + t, pb = q & 7u, x0 = q - pb;
    uint32_t v = 1;
    for (uint32_t i = 0; i < pb; ++i) v = (v << 1) | qbit(g, bits, x0 + i);
    sBC[tid] = (uint8_t)(v - 1u);
    sBit[tid] = bits[t];
  }
  __syncthreads();
#define CTX_B(c) ((uint32_t)sB[(c) - (int)j0 + (GMX_CTX_TILE - 1)])

  for (int idx = tid; idx < GMX_CTX_TILE * V; idx += 256) {
    const int jl = idx / V, v = idx - jl * V;
    const int c = (int)j0 + jl;
    if (c > (int)g.jmax) break;
    const int f = c - (int)g.fo;  // the run's byte opening of this slot; < 0: slot 0 carries the board's values
    const GmxCtxVarDev vd = dv->var[v];
    uint32_t val = 0;
    switch (vd.kind) {
      case GMX_CTXK_RECENT_BYTE:
        val = CTX_B(c - vd.index);
        break;
      case GMX_CTXK_BYTE_PLUS_RECENT:
        val = CTX_B(c - vd.index) << 8;
        break;
      case GMX_CTXK_SKIP:
        if (f < 0) {
          val = bd->values[v];
        } else {
          uint64_t key = 0;
          for (int i = 0; i < vd.n_bytes; ++i) key = (key << 8) + CTX_B(c - (int)vd.bytes_to_use[i]);
          val = gmx_ctx_murmur8(key);
        }
        break;
      case GMX_CTXK_INTERVAL:
        if (f < 0) {
          val = bd->values[v];
        } else {
          // context_ = mask_ & ((context_ << shift_) + map_[last_byte]) unrolled over the run's openings: map values
          // are below 1 << shift_, so the sum is a concatenation and what is shifted beyond bit 31 is gone
          const uint8_t* map = dv->maps[vd.index];
          for (int i = 0; i <= f && i * vd.shift < 32; ++i) val += (uint32_t)map[CTX_B(c - i)] << (i * vd.shift);
          const int64_t cs = (int64_t)(f + 1) * vd.shift;
          if (cs < 32) val += bd->values[v] << cs;
          val &= (uint32_t)((1ull << vd.num_bits) - 1ull);
        }
        break;
      case GMX_CTXK_INDIRECT_HASH:
        val = f < 0 ? bd->values[v] : a.scratch[((size_t)s * a.max_fires + (size_t)f) * (size_t)H + vd.index];
        break;
      default:  // ZERO, BIT_CONTEXT
        break;
    }
    sVal[jl][v] = val;
  }
  __syncthreads();

  // the bit records: lanes run along a record's columns, records of a stream are contiguous
  const size_t row0 = (size_t)s * a.rec_stride + t_lo;
  if (a.values) {
    uint32_t* out = a.values + row0 * (size_t)V;
    for (uint32_t i = tid; i < nrec * (uint32_t)V; i += 256) {
      const uint32_t r = i / (uint32_t)V, col = i - r * (uint32_t)V;
      const uint32_t jl = (g.nb0 + t_lo + r) / 8u - j0;
      out[i] = sVal[jl][col] + (sPerBit[col] ? sBC[r] : 0u);
    }
  }
  for (int k = 0; k < 3; ++k) {
    const GmxCtxTarget& tg = a.tg[k];
    if (!tg.ctx) continue;
    const uint32_t nc = (uint32_t)tg.n_cols;
    const size_t trow = (size_t)s * tg.stride + t_lo;
    uint32_t* out = tg.ctx + trow * nc;
    for (uint32_t i = tid; i < nrec * nc; i += 256) {
      const uint32_t r = i / nc, col = i - r * nc;
      const int rt = sRoute[k][col];
      if (rt < 0) continue;
      const uint32_t jl = (g.nb0 + t_lo + r) / 8u - j0;
      out[i] = sVal[jl][rt] + (sPerBit[rt] ? sBC[r] : 0u);
    }
    if ((uint32_t)tid < nrec) {
      if (tg.bc) tg.bc[trow + tid] = sBC[tid];
      if (tg.bits) tg.bits[trow + tid] = sBit[tid];
    }
  }
  // the values at the run's last record, for the commit
  if (j0 + GMX_CTX_TILE > g.jmax && tid < V)
    bd->next_values[tid] = sVal[g.jmax - j0][tid] + (sPerBit[tid] ? sBC[nrec - 1u] : 0u);
#undef CTX_B
}

// ---- the board at the run's end ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmx_ctx_commit_kernel(const GmxCtxDev* __restrict__ dv, GmxCtxRunArgs a) {
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const uint32_t n = run_bits(a, s);
  if (n == 0) return;
  GmxCtxBoard* bd = (GmxCtxBoard*)(a.banks + (size_t)s * dv->bank_bytes + dv->board_off);
  const uint8_t* bits = a.bits + (size_t)s * a.rec_stride;
  const Geo g = run_geo(bd, n);
  // recent_bits of the last record: the leading one and the bits of its byte in front of it
  const uint32_t q = g.nb0 + n - 1u, pb = q & 7u;
  uint32_t rb = 1;
  for (uint32_t i = 0; i < pb; ++i) rb = (rb << 1) | qbit(g, bits, q - pb + i);
  __syncthreads();  // every thread has read the board of the run's beginning
  const uint32_t c0 = g.jmax > GMX_CTX_RING ? g.jmax - GMX_CTX_RING + 1u : 1u;
  for (uint32_t c = c0 + tid; c <= g.jmax; c += 256)  // (bytes the run completed: functions of p and the bits)
    bd->ring[(g.pos + c) % GMX_CTX_RING] = (uint8_t)byte_at(g, bd, bits, (int)c);
  if (tid < dv->v) bd->values[tid] = bd->next_values[tid];
  if (tid == 0) {
    bd->recent_bits = rb;
    bd->new_bit = bits[n - 1u];
    bd->first_prediction = 0;
    bd->pos = (g.pos + g.jmax) % GMX_CTX_RING;
  }
}

// ---- one lock-step bit (gmx_ctx_step.h): a wave per stream ---------------------------------------------------------
__global__ __launch_bounds__(64) void gmx_ctx_step_kernel(const GmxCtxDev* __restrict__ dv, GmxCtxStepArgs a) {
  __shared__ uint32_t stage[GMX_CTX_MAX_VARS];
  gmx_ctx_step_body(dv, a, (int)blockIdx.x, (int)threadIdx.x, stage);
}

// ---- one bit of ONE stream on the launch path (gmx_ctx_forward / gmx_ctx_learn): the same step, a block of one wave;
// what the stream asks and the bit come in as kernel arguments, the V values and bit_context go into a pinned reply
__global__ __launch_bounds__(64) void gmx_ctx_bit_kernel(const GmxCtxDev* __restrict__ dv, GmxCtxBitArgs a) {
  __shared__ uint32_t stage[GMX_CTX_MAX_VARS];
  const int lane = (int)threadIdx.x;
  if (!(a.what & (GMX_CTX_STEP_LEARN | GMX_CTX_STEP_PREDICT))) return;
  gmx_ctx_step_core(dv, a.banks + (size_t)a.stream * dv->bank_bytes, a.what, a.bit & 1u, lane, stage, nullptr, 0,
                    &a.reply->bit_context);
  if ((a.what & GMX_CTX_STEP_PREDICT) && lane < dv->v) a.reply->values[lane] = stage[lane];
}

// recent_bits, new_bit and first_prediction of every stream, gathered for one transfer (gmx_chainstep_attach_ctx)
__global__ void gmx_ctx_heads_kernel(const GmxCtxDev* __restrict__ dv, const uint8_t* banks, int n_streams, uint32_t* out) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= n_streams) return;
  const GmxCtxBoard* bd = (const GmxCtxBoard*)(banks + (size_t)s * dv->bank_bytes + dv->board_off);
  out[3 * s] = bd->recent_bits;
  out[3 * s + 1] = bd->new_bit;
  out[3 * s + 2] = bd->first_prediction;
}

__global__ void gmx_ctx_init_kernel(const GmxCtxDev* __restrict__ dv, uint8_t* banks, int n_streams) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= n_streams) return;
  GmxCtxBoard* bd = (GmxCtxBoard*)(banks + (size_t)s * dv->bank_bytes + dv->board_off);
  bd->recent_bits = 1;       // short-term-memory.h:67
  bd->first_prediction = 1;  // basic-contexts.h
}

// ---- checkpoint: IndirectHash::WriteToDisk's sparse branch packed on the device -----------------------------------
__global__ __launch_bounds__(256) void gmx_ctx_ckpt_count_kernel(GmxCtxCkptArgs a) {
  const GmxCtxCkptChunk ch = a.chunks[blockIdx.x];
  const GmxCtxHashDev hd = a.dev->hash[ch.hash];
  const uint32_t* tab = (const uint32_t*)(a.bank + hd.tab_off) + ch.first_entry;
  __shared__ uint32_t wsum[4];
  const uint32_t end = gmx_walk_chunk_end(hd.table_size, ch.first_entry, GMX_CTX_CKPT_CHUNK);
  const uint32_t total = gmx_walk_block_count_u32(tab, end, wsum);
  if (threadIdx.x == 0) a.chunk_cnt[blockIdx.x] = total;
}

// {key, value} pairs of a sparse table in ascending key order, ranked by the walk of gmx_ckpt_walk.h
__global__ __launch_bounds__(256) void gmx_ctx_ckpt_pack_kernel(GmxCtxCkptArgs a) {
  const GmxCtxCkptChunk ch = a.chunks[blockIdx.x];
  if (a.hash_dense[ch.hash]) return;  // (block-uniform; a dense table is copied as it lies)
  const GmxCtxHashDev hd = a.dev->hash[ch.hash];
  const uint32_t* tab = (const uint32_t*)(a.bank + hd.tab_off) + ch.first_entry;
  const uint32_t end = gmx_walk_chunk_end(hd.table_size, ch.first_entry, GMX_CTX_CKPT_CHUNK);
  uint32_t* const recs = a.buf + a.hash_off[ch.hash] + 2ull * a.chunk_base[blockIdx.x];
  __shared__ uint32_t wsum[2][4];
  gmx_walk_pack_sparse_u32(tab, end, ch.first_entry, a.chunk_cnt[blockIdx.x], wsum,
                           [recs](uint32_t r, uint32_t key, uint32_t v) {
                             recs[2ull * r] = key;
                             recs[2ull * r + 1] = v;
                           });
}

// import: the pairs of the sparse tables into tables zeroed before (keys checked on the host)
__global__ __launch_bounds__(256) void gmx_ctx_ckpt_scatter_kernel(GmxCtxCkptArgs a) {
  const int h = (int)blockIdx.y;
  if (a.hash_dense[h]) return;
  uint32_t* tab = (uint32_t*)(a.bank + a.dev->hash[h].tab_off);
  const uint32_t* in = a.buf + a.hash_off[h];
  const uint32_t cnt = a.hash_cnt[h];
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < cnt; i += gridDim.x * 256u)
    tab[in[2 * (size_t)i]] = in[2 * (size_t)i + 1];
}

// marks (nullable): two events recorded behind the chain and behind the expand kernel, for a timed run
extern "C" hipError_t gmx_launch_ctx_run(const GmxCtxDev* dv, int n_hash, const GmxCtxRunArgs* args,
                                         hipStream_t stream, hipEvent_t* marks) {
  const GmxCtxRunArgs& a = *args;
  hipError_t e0 = hipSuccess;
  if (n_hash > 0) {
    hipLaunchKernelGGL(gmx_ctx_chain_kernel, dim3((unsigned)((a.n_streams + 3) / 4)), dim3(64), 0, stream, dv, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (marks && (e0 = hipEventRecord(marks[0], stream)) != hipSuccess) return e0;
  const uint64_t slots = (a.T + 7) / 8 + 2;  // nb0 <= 8: the last byte slot is at most (8 + T - 1) / 8
  const unsigned tiles = (unsigned)((slots + GMX_CTX_TILE - 1) / GMX_CTX_TILE);
  hipLaunchKernelGGL(gmx_ctx_expand_kernel, dim3(tiles, (unsigned)a.n_streams), dim3(256), 0, stream, dv, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (marks && (e0 = hipEventRecord(marks[1], stream)) != hipSuccess) return e0;
  hipLaunchKernelGGL(gmx_ctx_commit_kernel, dim3((unsigned)a.n_streams), dim3(256), 0, stream, dv, a);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_ctx_step(const GmxCtxDev* dv, const GmxCtxStepArgs* args, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ctx_step_kernel, dim3((unsigned)args->n_streams), dim3(64), 0, stream, dv, *args);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_ctx_bit(const GmxCtxDev* dv, const GmxCtxBitArgs* args, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ctx_bit_kernel, dim3(1), dim3(64), 0, stream, dv, *args);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_ctx_heads(const GmxCtxDev* dv, const uint8_t* banks, int n_streams, uint32_t* out,
                                            hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ctx_heads_kernel, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, stream, dv, banks,
                     n_streams, out);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_ctx_init(const GmxCtxDev* dv, uint8_t* banks, int n_streams, hipStream_t stream) {
  hipLaunchKernelGGL(gmx_ctx_init_kernel, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, stream, dv, banks,
                     n_streams);
  return hipGetLastError();
}
extern "C" hipError_t gmx_launch_ctx_ckpt_count(const GmxCtxCkptArgs* a, hipStream_t stream) {
  hipLaunchKernelGGL(gmx_ctx_ckpt_count_kernel, dim3(a->n_chunks), dim3(256), 0, stream, *a);
  return hipGetLastError();
}
extern "C" hipError_t gmx_launch_ctx_ckpt_pack(const GmxCtxCkptArgs* a, hipStream_t stream) {
  hipLaunchKernelGGL(gmx_ctx_ckpt_pack_kernel, dim3(a->n_chunks), dim3(256), 0, stream, *a);
  return hipGetLastError();
}
extern "C" hipError_t gmx_launch_ctx_ckpt_scatter(const GmxCtxCkptArgs* a, int n_hash, hipStream_t stream) {
  hipLaunchKernelGGL(gmx_ctx_ckpt_scatter_kernel, dim3(64, (unsigned)n_hash), dim3(256), 0, stream, *a);
  return hipGetLastError();
}
