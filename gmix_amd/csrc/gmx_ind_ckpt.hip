// gmx_ind_ckpt.hip -- the checkpoint of a whole Indirect group on the device (gfx950): find the live entries of every
// model's table, pack them into the reference's on-disk section, and scatter such sections back.
//
// An entry is a u16: low byte = nonstationary state, high byte = run-map state; it is live when the low byte is not
// 255.  IndirectMemory's part of LongTermMemory::WriteToDisk (long-term-memory.cpp:8-32) stores per model `u32 cnt`,
// then either cnt records {u32 key, u8 ns, u8 rm} in ascending key order (cnt < size / 3) or the `size` nonstationary
// bytes followed by the `size` run-map bytes, then 2 x 256 floats.  Records are 6 bytes and `size` is odd, so nothing
// in a section can be taken to be dword-aligned: every store below looks at its address and goes out as dwords,
// halves or bytes; every byte of a section is written by exactly one lane.  Logits travel as bit patterns; no float
// arithmetic happens here.
//
//   count    one block per (chunk of 16 Ki entries, stream): 8 entries per lane and iteration in one 16-byte load,
//            the lanes' counts summed over the wave by ballot + popcount of their bits, one integer per chunk.
//   pack     the same walk.  Sparse model: an entry's rank inside its chunk = live entries of the block's earlier
//            iterations + of the waves below + of the lanes below (ballots) + of the lane's own earlier entries, so the
//            records ascend without sorting; the chunk's first record index comes from the host's scan.  Dense model:
//            a chunk writes its low bytes at header + 4 + first_entry and its high bytes `size` further on.  The first
//            chunk of a model writes `cnt` and copies the model's 2048 logit bytes.
//   scatter  (the banks are reset first: gmx_indirect_init_kernel) one lane per record, or per entry of a dense
//            model; the logits.  The host has validated every section before (cnt <= size, key < size, keys strictly
//            ascending: no two lanes write one entry).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmx_ckpt_walk.h"
#include "gmx_ind_ckpt.h"

static_assert(GMX_IND_CKPT_STEP == 256 * 8, "256 lanes, 8 entries each");
static_assert(GMX_IND_CKPT_CHUNK % GMX_IND_CKPT_STEP == 0, "a chunk is a whole number of iterations");

// ---- stores and loads at any byte address ---------------------------------------------------------------------------
__device__ __forceinline__ void gmx_ic_put8(uint8_t* d, uint32_t a, uint32_t b) {
  const uint32_t al = (uint32_t)(uintptr_t)d & 3u;
  if (al == 0) {
    ((uint32_t*)d)[0] = a;
    ((uint32_t*)d)[1] = b;
  } else if (al == 2) {
    ((uint16_t*)d)[0] = (uint16_t)a;
    ((uint16_t*)d)[1] = (uint16_t)(a >> 16);
    ((uint16_t*)d)[2] = (uint16_t)b;
    ((uint16_t*)d)[3] = (uint16_t)(b >> 16);
  } else {
    d[0] = (uint8_t)a;
    *(uint16_t*)(d + 1) = (uint16_t)(a >> 8);
    *(uint16_t*)(d + 3) = (uint16_t)((a >> 24) | (b << 8));
    *(uint16_t*)(d + 5) = (uint16_t)(b >> 8);
    d[7] = (uint8_t)(b >> 24);
  }
}
// the first n (< 8) of the same eight bytes
__device__ __forceinline__ void gmx_ic_put_head(uint8_t* d, uint32_t a, uint32_t b, uint32_t n) {
#pragma unroll
  for (uint32_t i = 0; i < 7; ++i)
    if (i < n) d[i] = (uint8_t)((i < 4 ? a : b) >> (8u * (i & 3u)));
}
__device__ __forceinline__ void gmx_ic_put_u32(uint8_t* d, uint32_t v) {
  if (((uintptr_t)d & 1u) == 0) {
    ((uint16_t*)d)[0] = (uint16_t)v;
    ((uint16_t*)d)[1] = (uint16_t)(v >> 16);
  } else {
    d[0] = (uint8_t)v;
    *(uint16_t*)(d + 1) = (uint16_t)(v >> 8);
    d[3] = (uint8_t)(v >> 24);
  }
}
__device__ __forceinline__ void gmx_ic_put_record(uint8_t* d, uint32_t key, uint32_t entry) {
  if (((uintptr_t)d & 1u) == 0) {
    ((uint16_t*)d)[0] = (uint16_t)key;
    ((uint16_t*)d)[1] = (uint16_t)(key >> 16);
    ((uint16_t*)d)[2] = (uint16_t)entry;  // ns in the low byte, rm in the high one: the record's order
  } else {
    d[0] = (uint8_t)key;
    *(uint16_t*)(d + 1) = (uint16_t)(key >> 8);
    *(uint16_t*)(d + 3) = (uint16_t)((key >> 24) | (entry << 8));
    d[5] = (uint8_t)(entry >> 8);
  }
}

// ---- the walk -------------------------------------------------------------------------------------------------------
// Entries e0 .. e0 + 7 of a chunk (one 16-byte granule; a table's room in the bank is a multiple of 256 bytes, so the
// granule of any entry of the table is inside it).  Bit e of the result: entry e0 + e is below `end` and live.
// Entries are counted from the chunk's first, so that no index passes 2^32 in the largest table there can be.
struct GmxIcGranule {
  uint32_t w[4];  // two entries per word, the lower one in the low half
  uint32_t live;
};
__device__ __forceinline__ GmxIcGranule gmx_ic_load(const uint8_t* tab, uint32_t e0, uint32_t end) {
  GmxIcGranule g;
  g.w[0] = g.w[1] = g.w[2] = g.w[3] = 0x00ff00ffu;
  if (e0 < end) {
    const uint4 v = *(const uint4*)(tab + 2ull * e0);
    g.w[0] = v.x;
    g.w[1] = v.y;
    g.w[2] = v.z;
    g.w[3] = v.w;
  }
  g.live = 0;
#pragma unroll
  for (uint32_t e = 0; e < 8; ++e) {
    const uint32_t lo = (g.w[e >> 1] >> (16u * (e & 1u))) & 255u;
    if (lo != 255u && e0 + e < end) g.live |= 1u << e;
  }
  return g;
}

__global__ void __launch_bounds__(256) gmx_ind_ckpt_count_kernel(const GmxIndCkptArgs a) {
  __shared__ uint32_t wsum[4];
  const uint32_t c = blockIdx.x, s = blockIdx.y;
  const GmxIndCkptChunk ch = a.chunks[c];
  const GmxIndModelDev& x = a.dev->m[ch.model];
  const uint8_t* tab = a.banks + (uint64_t)s * a.dev->bank_bytes + x.tab_off + 2ull * ch.first_entry;
  const uint32_t end = min((uint32_t)GMX_IND_CKPT_CHUNK, x.size - ch.first_entry);
  uint32_t n = 0;  // at most 8 iterations x 8 entries
  for (uint32_t e0 = threadIdx.x * 8u; e0 < end; e0 += GMX_IND_CKPT_STEP)
    n += (uint32_t)__popc(gmx_ic_load(tab, e0, end).live);
  uint32_t below, total, all;
  gmx_walk_wave_sum(n, 7, &below, &total);
  (void)gmx_walk_rank_step(wsum, total, 0u, &all);
  if (threadIdx.x == 0) a.chunk_cnt[(uint64_t)s * a.n_chunks + c] = all;
}

__global__ void __launch_bounds__(256) gmx_ind_ckpt_pack_kernel(const GmxIndCkptArgs a) {
  __shared__ uint32_t wsum[2][4];
  const uint32_t c = blockIdx.x, s = blockIdx.y;
  const GmxIndCkptChunk ch = a.chunks[c];
  const uint32_t k = (uint32_t)a.dev->k;
  const GmxIndModelDev& x = a.dev->m[ch.model];
  const uint8_t* bank = a.banks + (uint64_t)s * a.dev->bank_bytes;
  const uint8_t* tab = bank + x.tab_off + 2ull * ch.first_entry;
  const uint32_t size = x.size;
  const uint32_t end = min((uint32_t)GMX_IND_CKPT_CHUNK, size - ch.first_entry);
  const uint32_t mc = a.model_cnt[(uint64_t)s * k + ch.model];
  uint8_t* out = a.buf + a.model_off[(uint64_t)s * k + ch.model];
  const bool dense = mc >= size / 3u;
  if (ch.first_entry == 0) {  // the header, and the logits behind the model's records or byte tables
    if (threadIdx.x == 0) gmx_ic_put_u32(out, mc);
    const uint2 v = ((const uint2*)(bank + a.dev->pred_off + 2048ull * ch.model))[threadIdx.x];
    gmx_ic_put8(out + 4 + (dense ? 2ull * size : 6ull * mc) + 8u * threadIdx.x, v.x, v.y);
  }
  if (dense) {
    uint8_t* lo = out + 4 + ch.first_entry;
    uint8_t* hi = lo + size;
    for (uint32_t e0 = threadIdx.x * 8u; e0 < end; e0 += GMX_IND_CKPT_STEP) {
      const GmxIcGranule g = gmx_ic_load(tab, e0, end);
      uint32_t l[2], h[2];
#pragma unroll
      for (uint32_t q = 0; q < 2; ++q) {
        const uint32_t w0 = g.w[2 * q], w1 = g.w[2 * q + 1];
        l[q] = (w0 & 255u) | ((w0 >> 8) & 0xff00u) | ((w1 & 255u) << 16) | ((w1 << 8) & 0xff000000u);
        h[q] = ((w0 >> 8) & 255u) | ((w0 >> 16) & 0xff00u) | ((w1 << 8) & 0xff0000u) | (w1 & 0xff000000u);
      }
      const uint32_t n = end - e0;
      if (n >= 8) {
        gmx_ic_put8(lo + e0, l[0], l[1]);
        gmx_ic_put8(hi + e0, h[0], h[1]);
      } else {  // the table's last entries
        gmx_ic_put_head(lo + e0, l[0], l[1], n);
        gmx_ic_put_head(hi + e0, h[0], h[1], n);
      }
    }
    return;
  }
  // (the banks do not change between the count pass and this one: should they ever, a chunk still writes no more
  // records than the scan gave it room for)
  const uint32_t room = a.chunk_cnt[(uint64_t)s * a.n_chunks + c];
  uint8_t* rec = out + 4 + 6ull * a.chunk_base[(uint64_t)s * a.n_chunks + c];
  uint32_t done = 0, it = 0;
  for (uint32_t i0 = 0; i0 < end; i0 += GMX_IND_CKPT_STEP, ++it) {  // (uniform over the block)
    const uint32_t e0 = i0 + threadIdx.x * 8u;
    const GmxIcGranule g = gmx_ic_load(tab, e0, end);
    uint32_t below, total, all;
    gmx_walk_wave_sum((uint32_t)__popc(g.live), 4, &below, &total);
    uint32_t r = gmx_walk_rank_step(wsum[it & 1u], total, done + below, &all);
#pragma unroll
    for (uint32_t e = 0; e < 8; ++e)
      if ((g.live >> e) & 1u) {
        if (r < room)
          gmx_ic_put_record(rec + 6ull * r, ch.first_entry + e0 + e, (g.w[e >> 1] >> (16u * (e & 1u))) & 0xffffu);
        ++r;
      }
    done += all;
  }
}

// grid: x = blocks striding over a model's records (or entries, dense), y = model, z = stream
__global__ void __launch_bounds__(256) gmx_ind_ckpt_scatter_kernel(const GmxIndCkptArgs a) {
  const uint32_t j = blockIdx.y, s = blockIdx.z;
  const uint32_t k = (uint32_t)a.dev->k;
  const GmxIndModelDev& x = a.dev->m[j];
  uint8_t* bank = a.banks + (uint64_t)s * a.dev->bank_bytes;
  uint16_t* tab = (uint16_t*)(bank + x.tab_off);
  const uint32_t size = x.size;
  const uint32_t mc = a.model_cnt[(uint64_t)s * k + j];
  const uint8_t* in = a.buf + a.model_off[(uint64_t)s * k + j] + 4;
  const uint64_t first = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
  uint64_t body;
  if (mc < size / 3u) {
    body = 6ull * mc;
    for (uint64_t r = first; r < mc; r += stride) {
      const uint8_t* p = in + 6ull * r;
      const uint32_t key = gmx_walk_get_u32(p);
      if (key >= size) continue;  // (the host's validation has refused such a section already)
      tab[key] = (uint16_t)((uint32_t)p[4] | ((uint32_t)p[5] << 8));
    }
  } else {
    body = 2ull * size;
    for (uint64_t e = first; e < size; e += stride)
      tab[e] = (uint16_t)((uint32_t)in[e] | ((uint32_t)in[size + e] << 8));
  }
  if (blockIdx.x == 0) {
    const uint8_t* p = in + body + 8u * threadIdx.x;
    uint32_t* dst = (uint32_t*)(bank + a.dev->pred_off + 2048ull * j) + 2u * threadIdx.x;
    dst[0] = gmx_walk_get_u32(p);
    dst[1] = gmx_walk_get_u32(p + 4);
  }
}

extern "C" hipError_t gmx_launch_ind_ckpt_count(const GmxIndCkptArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ind_ckpt_count_kernel, dim3(a->n_chunks, (unsigned)a->n_streams), dim3(256), 0, stream, *a);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_ind_ckpt_pack(const GmxIndCkptArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ind_ckpt_pack_kernel, dim3(a->n_chunks, (unsigned)a->n_streams), dim3(256), 0, stream, *a);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_ind_ckpt_scatter(const GmxIndCkptArgs* a, int n_models, unsigned blocks_x,
                                                  hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ind_ckpt_scatter_kernel, dim3(blocks_x, (unsigned)n_models, (unsigned)a->n_streams),
                     dim3(256), 0, stream, *a);
  return hipGetLastError();
}
