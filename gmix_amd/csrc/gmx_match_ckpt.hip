// gmx_match_ckpt.hip -- the checkpoint of a whole Match group on the device (gfx950): count the valid entries of every
// stream's tables, assemble every stream's long section (long-term-memory.cpp:70-106) in one device image laid out
// as the caller's buffer, and put such an image back.  Count and pack walk the tables with gmx_ckpt_walk.h, as the
// per-stream kernels of gmx_match.hip do: the two are no independent witnesses of each other.
//
// A stream's long section: u64 history size, the history bytes, then per model u32 count of valid entries (entries
// that are not 0), the records {u32 key, 5 pointer bytes} in ascending key order (count < 5/9 of the table) or
// 5 bytes per entry, 256 floats, 256 ints.  The history has any length and records are 9 and 5 bytes, so nothing in a
// section can be taken to be aligned.  Stores into the image:
//   * counts, records, dense entries, the tails and the u64 header are BYTE stores, every byte written by exactly one
//     lane (as gmx_match_ckpt_pack_kernel writes them);
//   * history bytes (both directions) go through gmx_mk_copy, which stores a dword only at a destination address it
//     has itself rounded up to a multiple of 4, and bytes in front of and behind those;
//   * stores into the banks (tables, probabilities, counts, states) are dwords at offsets that gmx_match_create
//     rounds to 256 bytes.
// Loads from the image are byte loads; loads from the tables are 16-byte granules (a table's room in the bank is a
// multiple of 256 bytes, so the granule of any entry below the table size is inside it) whose entries at or beyond the
// chunk's end are masked.  No float arithmetic happens here: probabilities travel as bit patterns.
//
// Every grid is flat in x -- block = (stream, chunk) or (stream, model, slice) -- so that no stream count meets the
// 65 535 limit of grid y / z; the host refuses a call whose flat grid would not fit 31 bits.
//
//   count    one block per (stream, chunk of 16 Ki entries): 4 entries per lane and iteration in one 16-byte load, the
//            lanes' counts summed by ballot + popcount; the block of a stream's chunk 0 also copies the bank's 144
//            bytes of model and stream states into the array that travels to the host with the counts.
//   pack     the same walk.  Ranks by gmx_walk_pack_sparse_u32: valid entries of the block's earlier iterations
//            + of the waves below + of the lanes below, so the records ascend without sorting; a chunk's first record
//            index comes from the host's scan.  A model's first chunk writes its count and its 2 KiB tail.
//   history  u64 header and the history bytes [0, hist_size): nothing at or beyond the size is read.
//   zero     import: the tables of the call's banks.
//   scatter  import: one lane per record, or per entry of a dense model (the host has validated every section: keys
//            strictly ascending and below the table size, so no two lanes write one entry); slice 0 of a model puts
//            its tail back, slice 0 of model 0 the states -- slot values, ctx, new_bit and bit_context stay.
//   restore  import: the history bytes out of the image.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmx_ckpt_walk.h"
#include "gmx_match_ckpt.h"

static_assert(sizeof(GmxMatchGckStates) == 144, "8 model states and the stream state, contiguous in a bank");
static_assert(sizeof(GmxMatchGckModel) == 24 && sizeof(GmxMatchGckStream) == 16, "host and device agree");
static_assert(GMX_MATCH_CKPT_CHUNK % 1024 == 0, "a chunk is a whole number of 256-lane x 4-entry iterations");

// Bytes [0, n) from src to dst, both at any address.  Unit 0 is the `lead` bytes in front of dst's first multiple of
// 4; unit u >= 1 the four bytes from lead + 4 (u - 1): one dword store at an address that is a multiple of 4 by
// construction, or byte stores for the last, partial unit.  Units `first`, `first + stride`, ... are this lane's.
__device__ __forceinline__ void gmx_mk_copy(uint8_t* dst, const uint8_t* src, uint64_t n, uint64_t first,
                                            uint64_t stride) {
  uint64_t lead = (uint64_t)((4u - ((uint32_t)(uintptr_t)dst & 3u)) & 3u);
  if (lead > n) lead = n;
  const uint64_t units = 1 + (n - lead + 3) / 4;
  for (uint64_t u = first; u < units; u += stride) {
    if (u == 0) {
      for (uint64_t i = 0; i < lead; ++i) dst[i] = src[i];
      continue;
    }
    const uint64_t at = lead + 4 * (u - 1);
    if (n - at >= 4) {
      *(uint32_t*)(dst + at) = gmx_walk_get_u32(src + at);
    } else {
      for (uint64_t i = at; i < n; ++i) dst[i] = src[i];
    }
  }
}

__global__ void __launch_bounds__(256) gmx_match_gck_count_kernel(const GmxMatchGckArgs a) {
  __shared__ uint32_t wsum[4];
  const uint32_t s = blockIdx.x / a.n_chunks, c = blockIdx.x % a.n_chunks;
  const GmxMatchCkptChunk ch = a.chunks[c];
  const GmxMatchModelDev& x = a.dev->m[ch.model];
  const uint8_t* bank = a.banks + (uint64_t)s * a.dev->bank_bytes;
  const uint32_t* tab = (const uint32_t*)(bank + x.tab_off) + ch.first_entry;
  const uint32_t end = gmx_walk_chunk_end(x.table_size, ch.first_entry, GMX_MATCH_CKPT_CHUNK);
  const uint32_t total = gmx_walk_block_count_u32(tab, end, wsum);
  if (threadIdx.x == 0) a.chunk_cnt[blockIdx.x] = total;
  if (c == 0 && threadIdx.x < sizeof(GmxMatchGckStates) / 4)
    ((uint32_t*)(a.states + s))[threadIdx.x] = ((const uint32_t*)(bank + a.dev->mstate_off))[threadIdx.x];
}

__global__ void __launch_bounds__(256) gmx_match_gck_pack_kernel(const GmxMatchGckArgs a) {
  __shared__ uint32_t wsum[2][4];
  const uint32_t s = blockIdx.x / a.n_chunks, c = blockIdx.x % a.n_chunks;
  const GmxMatchCkptChunk ch = a.chunks[c];
  const GmxMatchModelDev& x = a.dev->m[ch.model];
  const uint8_t* bank = a.banks + (uint64_t)s * a.dev->bank_bytes;
  const uint32_t* tab = (const uint32_t*)(bank + x.tab_off) + ch.first_entry;
  const uint32_t size = x.table_size;
  const uint32_t end = gmx_walk_chunk_end(size, ch.first_entry, GMX_MATCH_CKPT_CHUNK);
  const GmxMatchGckModel md = a.md[(uint64_t)s * (uint32_t)a.dev->k + ch.model];
  uint8_t* const out = a.image + md.off;
  if (ch.first_entry == 0) {  // the count in front of the model's body, the probabilities and counts behind it
    if (threadIdx.x == 0) gmx_walk_put_u32(out, md.cnt);
    const uint64_t src = (threadIdx.x < 128u ? a.dev->pred_off : a.dev->cnt_off) + 1024ull * ch.model;
    const uint2 v = ((const uint2*)(bank + src))[threadIdx.x & 127u];
    uint8_t* o = out + 4 + (md.dense ? 5ull * size : 9ull * md.cnt) + 8u * threadIdx.x;
    gmx_walk_put_u32(o, v.x);
    gmx_walk_put_u32(o + 4, v.y);
  }
  if (md.dense) {
    uint8_t* const body = out + 4 + 5ull * ch.first_entry;
    for (uint32_t e0 = threadIdx.x * 4u; e0 < end; e0 += 1024u) {
      const uint4 v = gmx_walk_load4(tab, e0, end);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t i = 0; i < 4; ++i)
        if (e0 + i < end) {
          uint8_t* o = body + 5ull * (e0 + i);
          gmx_walk_put_u32(o, w[i]);
          o[4] = 0;
        }
    }
    return;
  }
  const uint32_t room = a.chunk_cnt[blockIdx.x];
  if (room == 0) return;  // (uniform over the block)
  uint8_t* const recs = out + 4 + 9ull * a.chunk_base[blockIdx.x];
  gmx_walk_pack_sparse_u32(tab, end, ch.first_entry, room, wsum, [recs](uint32_t r, uint32_t key, uint32_t v) {
    uint8_t* o = recs + 9ull * r;
    gmx_walk_put_u32(o, key);
    gmx_walk_put_u32(o + 4, v);
    o[8] = 0;
  });
}

// block = (stream, slice of a.blocks)
__global__ void __launch_bounds__(256) gmx_match_gck_history_kernel(const GmxMatchGckArgs a) {
  const uint32_t s = blockIdx.x / a.blocks, b = blockIdx.x % a.blocks;
  const GmxMatchGckStream st = a.st[s];
  uint8_t* const out = a.image + st.sec_off;
  if (b == 0 && threadIdx.x < 8u) out[threadIdx.x] = threadIdx.x < 4u ? (uint8_t)(st.hist_size >> (8u * threadIdx.x)) : 0;
  gmx_mk_copy(out + 8, a.hist + (uint64_t)s * a.dev->hist_cap, st.hist_size, (uint64_t)b * 256u + threadIdx.x,
              (uint64_t)a.blocks * 256u);
}

__global__ void __launch_bounds__(256) gmx_match_gck_restore_kernel(const GmxMatchGckArgs a) {
  const uint32_t s = blockIdx.x / a.blocks, b = blockIdx.x % a.blocks;
  const GmxMatchGckStream st = a.st[s];
  gmx_mk_copy(a.hist + (uint64_t)s * a.dev->hist_cap, a.image + st.sec_off + 8, st.hist_size,
              (uint64_t)b * 256u + threadIdx.x, (uint64_t)a.blocks * 256u);
}

__global__ void __launch_bounds__(256) gmx_match_gck_zero_kernel(const GmxMatchGckArgs a) {
  const uint32_t s = blockIdx.x / a.blocks, b = blockIdx.x % a.blocks;
  uint4* p = (uint4*)(a.banks + (uint64_t)s * a.dev->bank_bytes);
  const uint64_t n = a.dev->tab_bytes / 16u;  // (the tables' room is a multiple of 256 bytes)
  for (uint64_t i = (uint64_t)b * 256u + threadIdx.x; i < n; i += (uint64_t)a.blocks * 256u)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// block = (stream, model, slice of a.blocks)
__global__ void __launch_bounds__(256) gmx_match_gck_scatter_kernel(const GmxMatchGckArgs a) {
  const uint32_t k = (uint32_t)a.dev->k;
  const uint32_t bx = blockIdx.x % a.blocks, sj = blockIdx.x / a.blocks;
  const uint32_t j = sj % k, s = sj / k;
  const GmxMatchModelDev& x = a.dev->m[j];
  uint8_t* bank = a.banks + (uint64_t)s * a.dev->bank_bytes;
  uint32_t* tab = (uint32_t*)(bank + x.tab_off);
  const uint32_t size = x.table_size;
  const GmxMatchGckModel md = a.md[(uint64_t)s * k + j];
  const uint8_t* in = a.image + md.off + 4;
  const uint64_t first = (uint64_t)bx * 256u + threadIdx.x, stride = (uint64_t)a.blocks * 256u;
  uint64_t body;
  if (!md.dense) {
    body = 9ull * md.cnt;
    for (uint64_t r = first; r < md.cnt; r += stride) {
      const uint8_t* p = in + 9ull * r;
      const uint32_t key = gmx_walk_get_u32(p);
      if (key < size) tab[key] = gmx_walk_get_u32(p + 4);  // (the host's validation has refused any other section)
    }
  } else {
    body = 5ull * size;
    for (uint64_t e = first; e < size; e += stride) tab[e] = gmx_walk_get_u32(in + 5ull * e);
  }
  if (bx != 0) return;
  {
    const uint8_t* p = in + body + 8u * threadIdx.x;
    const uint64_t dst = (threadIdx.x < 128u ? a.dev->pred_off : a.dev->cnt_off) + 1024ull * j;
    uint32_t* d = (uint32_t*)(bank + dst) + 2u * (threadIdx.x & 127u);
    d[0] = gmx_walk_get_u32(p);
    d[1] = gmx_walk_get_u32(p + 4);
  }
  if (j != 0) return;
  if (threadIdx.x < k) {
    const GmxMatchGckModel mi = a.md[(uint64_t)s * k + threadIdx.x];
    GmxMatchModelState* m = (GmxMatchModelState*)(bank + a.dev->mstate_off) + threadIdx.x;
    m->cur_match = mi.cur_match;
    m->cur_byte = mi.cur_byte;
    m->bit_pos = mi.bit_pos;
    m->match_length = mi.match_length;
  }
  if (threadIdx.x == 64u) ((GmxMatchStreamState*)(bank + a.dev->sstate_off))->hist_size = a.st[s].hist_size;
}

#define GCK_LAUNCH(name, grid) \
  GMX_WALK_LAUNCH(gmx_launch_match_gck_##name, GmxMatchGckArgs, gmx_match_gck_##name##_kernel, grid)
GCK_LAUNCH(count, (uint64_t)a->n_streams * a->n_chunks)
GCK_LAUNCH(pack, (uint64_t)a->n_streams * a->n_chunks)
GCK_LAUNCH(history, (uint64_t)a->n_streams * a->blocks)
GCK_LAUNCH(restore, (uint64_t)a->n_streams * a->blocks)
GCK_LAUNCH(zero, (uint64_t)a->n_streams * a->blocks)
// (n_models: the host's copy of dev->k)
extern "C" hipError_t gmx_launch_match_gck_scatter(const GmxMatchGckArgs* a, int n_models, hipStream_t stream) {
  (void)hipGetLastError();
  const uint64_t blocks = (uint64_t)a->n_streams * (uint64_t)n_models * a->blocks;
  if (n_models < 1 || blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmx_match_gck_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, *a);
  return hipGetLastError();
}
