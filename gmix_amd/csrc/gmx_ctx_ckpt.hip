// gmx_ctx_ckpt.hip -- the checkpoint of a whole context group on the device (gfx950): count the non-zero entries of
// every stream's hash tables, assemble every stream's H IndirectHash::WriteToDisk sections (indirect-hash.cpp:33-54) in
// one device image laid out as the caller's buffer, put such an image back, and gather / scatter the blackboards.
// Count and pack walk the tables with gmx_ckpt_walk.h, as the per-stream kernels of gmx_ctx.hip do: the two are no
// independent witnesses of each other.
//
// A table's section: u32 count of non-zero entries; {u32 key, u32 value} in ascending key order (count < size / 2) or
// the whole table, 4 bytes an entry; u64 outer_context_, u32 outer_hash_.  Every section length is a multiple of 4
// (4 + 8 count + 12, or 4 + 4 size + 12) and a launch's image begins at a 256-byte boundary, so every access to the
// image is a dword at an address that is a multiple of 4, each dword written by exactly one lane.  Loads from the
// tables are 16-byte granules (a table's room in the bank is a multiple of 256 bytes, so the granule of any entry below
// the table size is inside it) whose entries at or beyond the table's end are masked by index -- the padding is not
// trusted to be zero.  No arithmetic happens on the tables: values travel as bit patterns.
//
// Every grid is flat in x -- block = (stream, chunk) or (stream, table, slice) -- so that no stream count meets the
// 65 535 limit of grid y / z; the host refuses a call whose flat grid would not fit 31 bits.
//
//   count          one block per (stream, chunk of 16 Ki entries): 4 entries per lane and iteration in one 16-byte
//                  load, the lanes' counts summed by ballot + popcount; the block of a stream's chunk 0 also copies the
//                  bank's 16 hash states into the array that travels to the host with the counts.
//   pack           the same walk.  Sparse: ranks by gmx_walk_pack_sparse_u32 -- pairs of the table's earlier chunks
//                  (the host's scan) + of the block's earlier rounds + of the waves below + of the lanes below, so the
//                  pairs ascend without sorting; a chunk without an entry returns at once.  Dense: the chunk's entries
//                  as they lie.  A table's first chunk writes the count in front and the 12-byte trailer behind.
//   zero           import: the sparse tables of the launch's streams.
//   scatter        import: one lane per pair, or per entry of a dense table (the host has validated every section:
//                  keys strictly ascending and below the table size, so no two lanes write one entry); slice 0 of a
//                  table puts its hash state back out of the image.  The boards are not touched.
//   board_gather   one block per stream: GmxCtxBoard -> a gmx_ctx_blackboard record (last_byte and recent_bytes are
//                  read off the ring).
//   board_scatter  the inverse; next_values (expand -> commit, internal) is cleared as gmx_ctx_blackboard_set clears it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gmx_ckpt_walk.h"
#include "gmx_ctx_ckpt.h"

static_assert(sizeof(GmxCtxHashState) == 16 && sizeof(GmxCtxGckTable) == 16, "host and device agree");
static_assert(sizeof(GmxCtxGckBoard) == 1316 && sizeof(GmxCtxGckBoard) % 4 == 0, "gmx_ctx_blackboard, in dwords");
static_assert(offsetof(GmxCtxGckBoard, rotating_history) % 4 == 0 && offsetof(GmxCtxBoard, ring) % 4 == 0 &&
                  GMX_CTX_RING % 4 == 0,
              "the ring travels in dwords");
static_assert(GMX_CTX_CKPT_CHUNK % 1024 == 0, "a chunk is a whole number of 256-lane x 4-entry iterations");

__global__ void __launch_bounds__(256) gmx_ctx_gck_count_kernel(const GmxCtxGckArgs a) {
  __shared__ uint32_t wsum[4];
  const uint32_t s = blockIdx.x / a.n_chunks, c = blockIdx.x % a.n_chunks;
  const GmxCtxCkptChunk ch = a.chunks[c];
  const GmxCtxHashDev& x = a.dev->hash[ch.hash];
  const uint8_t* bank = a.banks + (uint64_t)s * a.dev->bank_bytes;
  const uint32_t* tab = (const uint32_t*)(bank + x.tab_off) + ch.first_entry;
  const uint32_t end = gmx_walk_chunk_end(x.table_size, ch.first_entry, GMX_CTX_CKPT_CHUNK);
  const uint32_t total = gmx_walk_block_count_u32(tab, end, wsum);
  if (threadIdx.x == 0) a.chunk_cnt[blockIdx.x] = total;
  if (c == 0 && threadIdx.x < GMX_CTX_MAX_HASH * sizeof(GmxCtxHashState) / 4)
    ((uint32_t*)(a.states + (uint64_t)s * GMX_CTX_MAX_HASH))[threadIdx.x] =
        ((const uint32_t*)(bank + a.dev->hstate_off))[threadIdx.x];
}

__global__ void __launch_bounds__(256) gmx_ctx_gck_pack_kernel(const GmxCtxGckArgs a) {
  __shared__ uint32_t wsum[2][4];
  const uint32_t s = blockIdx.x / a.n_chunks, c = blockIdx.x % a.n_chunks;
  const GmxCtxCkptChunk ch = a.chunks[c];
  const GmxCtxHashDev& x = a.dev->hash[ch.hash];
  const uint8_t* bank = a.banks + (uint64_t)s * a.dev->bank_bytes;
  const uint32_t* tab = (const uint32_t*)(bank + x.tab_off) + ch.first_entry;
  const uint32_t size = x.table_size;
  const uint32_t end = gmx_walk_chunk_end(size, ch.first_entry, GMX_CTX_CKPT_CHUNK);
  const GmxCtxGckTable tb = a.tb[(uint64_t)s * (uint32_t)a.dev->h + ch.hash];
  uint32_t* const out = (uint32_t*)(a.image + tb.off);
  if (ch.first_entry == 0 && threadIdx.x < 4u) {  // the count in front of the body, the hash state behind it
    if (threadIdx.x == 0) {
      out[0] = tb.cnt;
    } else {  // u64 outer_context_, u32 outer_hash_: the state's first three dwords
      const uint32_t* st = (const uint32_t*)(bank + a.dev->hstate_off + (uint64_t)ch.hash * sizeof(GmxCtxHashState));
      out[1ull + (tb.dense ? (uint64_t)size : 2ull * tb.cnt) + (threadIdx.x - 1u)] = st[threadIdx.x - 1u];
    }
  }
  if (tb.dense) {
    uint32_t* const body = out + 1 + ch.first_entry;
    for (uint32_t e0 = threadIdx.x * 4u; e0 < end; e0 += 1024u) {
      const uint4 v = gmx_walk_load4(tab, e0, end);
      body[e0] = v.x;
      if (e0 + 1 < end) body[e0 + 1] = v.y;
      if (e0 + 2 < end) body[e0 + 2] = v.z;
      if (e0 + 3 < end) body[e0 + 3] = v.w;
    }
    return;
  }
  const uint32_t room = a.chunk_cnt[blockIdx.x];
  if (room == 0) return;  // (uniform over the block)
  uint32_t* const recs = out + 1 + 2ull * a.chunk_base[blockIdx.x];
  gmx_walk_pack_sparse_u32(tab, end, ch.first_entry, room, wsum, [recs](uint32_t r, uint32_t key, uint32_t v) {
    recs[2ull * r] = key;
    recs[2ull * r + 1] = v;
  });
}

// block = (stream, table, slice of a.blocks)
__global__ void __launch_bounds__(256) gmx_ctx_gck_zero_kernel(const GmxCtxGckArgs a) {
  const uint32_t h = (uint32_t)a.dev->h;
  const uint32_t bx = blockIdx.x % a.blocks, sj = blockIdx.x / a.blocks;
  const uint32_t j = sj % h, s = sj / h;
  if (a.tb[(uint64_t)s * h + j].dense) return;  // (every entry of a dense table is written by the scatter)
  const GmxCtxHashDev& x = a.dev->hash[j];
  uint4* p = (uint4*)(a.banks + (uint64_t)s * a.dev->bank_bytes + x.tab_off);
  const uint64_t n = (4ull * x.table_size + 255u) / 256u * 16u;  // (the table's room is a multiple of 256 bytes)
  for (uint64_t i = (uint64_t)bx * 256u + threadIdx.x; i < n; i += (uint64_t)a.blocks * 256u)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// block = (stream, table, slice of a.blocks)
__global__ void __launch_bounds__(256) gmx_ctx_gck_scatter_kernel(const GmxCtxGckArgs a) {
  const uint32_t h = (uint32_t)a.dev->h;
  const uint32_t bx = blockIdx.x % a.blocks, sj = blockIdx.x / a.blocks;
  const uint32_t j = sj % h, s = sj / h;
  const GmxCtxHashDev& x = a.dev->hash[j];
  uint8_t* bank = a.banks + (uint64_t)s * a.dev->bank_bytes;
  uint32_t* tab = (uint32_t*)(bank + x.tab_off);
  const uint32_t size = x.table_size;
  const GmxCtxGckTable tb = a.tb[(uint64_t)s * h + j];
  const uint32_t* in = (const uint32_t*)(a.image + tb.off) + 1;
  const uint64_t first = (uint64_t)bx * 256u + threadIdx.x, stride = (uint64_t)a.blocks * 256u;
  uint64_t body;
  if (!tb.dense) {
    body = 2ull * tb.cnt;
    for (uint64_t r = first; r < tb.cnt; r += stride) {
      const uint32_t key = in[2 * r];
      if (key < size) tab[key] = in[2 * r + 1];  // (the host's validation has refused any other section)
    }
  } else {
    body = size;
    for (uint64_t e = first; e < size; e += stride) tab[e] = in[e];
  }
  if (bx == 0 && threadIdx.x < 4u) {  // outer_context_, outer_hash_, and the state's padding word
    uint32_t* st = (uint32_t*)(bank + a.dev->hstate_off + (uint64_t)j * sizeof(GmxCtxHashState));
    st[threadIdx.x] = threadIdx.x < 3u ? in[body + threadIdx.x] : 0u;
  }
}

// block = stream
__global__ void __launch_bounds__(256) gmx_ctx_gck_board_gather_kernel(const GmxCtxGckArgs a) {
  const uint32_t s = blockIdx.x, t = threadIdx.x;
  const GmxCtxBoard* bd = (const GmxCtxBoard*)(a.banks + (uint64_t)s * a.dev->bank_bytes + a.dev->board_off);
  GmxCtxGckBoard* o = a.boards + s;
  const uint32_t pos = bd->pos;
  if (t == 0) {
    o->recent_bits = (int32_t)bd->recent_bits;
    o->new_bit = (int32_t)bd->new_bit;
    o->rotating_history_pos = pos;
    o->first_prediction = (int32_t)bd->first_prediction;
    o->last_byte = bd->ring[pos % GMX_CTX_RING];
  }
  if (t < 10u) o->recent_bytes[t] = bd->ring[(pos % GMX_CTX_RING + GMX_CTX_RING - t) % GMX_CTX_RING];
  if (t < (uint32_t)GMX_CTX_MAX_VARS) o->values[t] = t < (uint32_t)a.dev->v ? bd->values[t] : 0u;
  if (t < GMX_CTX_RING / 4) ((uint32_t*)o->rotating_history)[t] = ((const uint32_t*)bd->ring)[t];
}

__global__ void __launch_bounds__(256) gmx_ctx_gck_board_scatter_kernel(const GmxCtxGckArgs a) {
  const uint32_t s = blockIdx.x, t = threadIdx.x;
  GmxCtxBoard* bd = (GmxCtxBoard*)(a.banks + (uint64_t)s * a.dev->bank_bytes + a.dev->board_off);
  const GmxCtxGckBoard* in = a.boards + s;
  if (t == 0) {
    bd->recent_bits = (uint32_t)in->recent_bits;
    bd->new_bit = (uint32_t)in->new_bit;
    bd->first_prediction = in->first_prediction ? 1u : 0u;
    bd->pos = in->rotating_history_pos;
  }
  if (t < (uint32_t)GMX_CTX_MAX_VARS) {
    bd->values[t] = t < (uint32_t)a.dev->v ? in->values[t] : 0u;
    bd->next_values[t] = 0u;
  }
  if (t < GMX_CTX_RING / 4) ((uint32_t*)bd->ring)[t] = ((const uint32_t*)in->rotating_history)[t];
}

#define GCK_LAUNCH(name, grid) \
  GMX_WALK_LAUNCH(gmx_launch_ctx_gck_##name, GmxCtxGckArgs, gmx_ctx_gck_##name##_kernel, grid)
GCK_LAUNCH(count, (uint64_t)a->n_streams * a->n_chunks)
GCK_LAUNCH(pack, (uint64_t)a->n_streams * a->n_chunks)
GCK_LAUNCH(board_gather, (uint64_t)a->n_streams)
GCK_LAUNCH(board_scatter, (uint64_t)a->n_streams)
// (n_hash: the host's copy of dev->h)
#define GMX_CTX_GCK_LAUNCH_H(fn, kernel)                                                       \
  extern "C" hipError_t fn(const GmxCtxGckArgs* a, int n_hash, hipStream_t stream) {           \
    (void)hipGetLastError();                                                                   \
    const uint64_t blocks_ = (uint64_t)a->n_streams * (uint64_t)n_hash * a->blocks;            \
    if (n_hash < 1 || blocks_ == 0 || blocks_ > 0x7fffffffull) return hipErrorInvalidValue;    \
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks_), dim3(256), 0, stream, *a);             \
    return hipGetLastError();                                                                  \
  }
GMX_CTX_GCK_LAUNCH_H(gmx_launch_ctx_gck_zero, gmx_ctx_gck_zero_kernel)
GMX_CTX_GCK_LAUNCH_H(gmx_launch_ctx_gck_scatter, gmx_ctx_gck_scatter_kernel)
