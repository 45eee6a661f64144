// gmx_ckpt.hip -- the group checkpoint on the device (gfx950): find the learned rows of every bank, pack them
// into the reference's on-disk record format, and scatter such records back.
//
// A row is "learned" when its step counter (MixerData::steps) is not zero; LongTermMemory::WriteToDisk
// (long-term-memory.cpp:35-55) stores exactly those: per mixer `u32 cnt, u32 input_size`, then per learned row in
// ascending row order `u32 row, u64 steps, weight_size x f32`.  Every field is a multiple of four bytes, so a
// section is an array of dwords; weights travel as bit patterns, no float arithmetic happens here.
//
//   count    one block per (chunk of 256 rows, stream): each thread reads one counter (through rs_off / rs_pitch,
//            so every bank layout of build_topology works), ballot + popcount per wave, one integer per chunk.
//   pack     the same walk; a row's rank inside its chunk comes from the ballot, the chunk's offset from the
//            host's exclusive scan over the counts.  The block's four waves then copy the chunk's learned rows,
//            one wave per record.  The first chunk of a mixer writes its header, the first chunk of a stream the
//            3 x u64 scalars of every mixer.
//   scatter  one wave per record: weights to `row`, the counter where the layout keeps it; the scalars to scal_off.
//            The host has validated every record head before (row < table_size, rows of a mixer strictly
//            ascending: no two waves write one row) and zeroed the banks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmx_ckpt.h"
#include "gmx_ckpt_walk.h"

static_assert(GMX_CKPT_CHUNK == 256, "one thread per row of a chunk, four waves per block");

// Rows with steps != 0 among the chunk's 256: the thread's own flag and counter, the count over the block, and
// the thread's rank among the learned ones (ascending row order).
struct GmxCkptWalk {
  uint32_t row, rank, total;
  uint64_t steps;
  bool live;
};
__device__ __forceinline__ GmxCkptWalk gmx_ckpt_walk(const uint8_t* bank, const GmxMixerDev& x, uint32_t first_row,
                                                     uint32_t* wsum /* LDS [4] */) {
  GmxCkptWalk w;
  w.row = first_row + threadIdx.x;
  w.steps = 0;
  if (w.row < x.table_size) w.steps = *GMX_RS_PTR(bank, x, w.row);
  w.live = w.steps != 0;
  const unsigned long long b = __ballot(w.live);
  w.rank = gmx_walk_rank_step(wsum, (uint32_t)__popcll(b), 0u, &w.total) +
           (uint32_t)__popcll(b & ((1ull << (threadIdx.x & 63u)) - 1ull));
  return w;
}

__global__ void __launch_bounds__(GMX_CKPT_CHUNK) gmx_ckpt_count_kernel(const GmxCkptArgs a) {
  __shared__ uint32_t wsum[4];
  const uint32_t c = blockIdx.x, s = blockIdx.y;
  const GmxCkptChunk ch = a.chunks[c];
  const GmxMixerDev& x = a.topo->mx[ch.mixer];
  const uint8_t* bank = a.banks + (uint64_t)s * a.topo->bank_bytes;
  const GmxCkptWalk w = gmx_ckpt_walk(bank, x, ch.first_row, wsum);
  if (threadIdx.x == 0) a.chunk_cnt[(uint64_t)s * a.n_chunks + c] = w.total;
}

__global__ void __launch_bounds__(GMX_CKPT_CHUNK) gmx_ckpt_pack_kernel(const GmxCkptArgs a) {
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t l_row[GMX_CKPT_CHUNK], l_lo[GMX_CKPT_CHUNK], l_hi[GMX_CKPT_CHUNK];
  const uint32_t c = blockIdx.x, s = blockIdx.y;
  const GmxCkptChunk ch = a.chunks[c];
  const uint32_t m = (uint32_t)a.topo->m;
  const GmxMixerDev& x = a.topo->mx[ch.mixer];
  const uint8_t* bank = a.banks + (uint64_t)s * a.topo->bank_bytes;
  const GmxCkptWalk w = gmx_ckpt_walk(bank, x, ch.first_row, wsum);
  if (w.live) {
    l_row[w.rank] = w.row;
    l_lo[w.rank] = (uint32_t)w.steps;
    l_hi[w.rank] = (uint32_t)(w.steps >> 32);
  }
  __syncthreads();
  // (the banks do not change between the count pass and this one: should they ever, a chunk still writes no
  // more records than the scan gave it room for)
  const uint32_t cnt = min(w.total, a.chunk_cnt[(uint64_t)s * a.n_chunks + c]);
  const uint32_t ws = x.weight_size, rec = 3u + ws;
  uint32_t* out = a.long_buf + (a.chunk_off[(uint64_t)s * a.n_chunks + c] >> 2);
  if (ch.first_row == 0 && threadIdx.x == 0) {  // the mixer's header lies right in front of its first record
    const uint32_t mc = a.mixer_cnt[(uint64_t)s * m + ch.mixer];
    out[-2] = mc;
    out[-1] = mc ? ws : 0u;
  }
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t r = wave; r < cnt; r += 4) {
    uint32_t* o = out + (uint64_t)r * rec;
    const uint32_t row = l_row[r];
    const uint32_t* src = (const uint32_t*)(bank + x.w_off) + (uint64_t)row * x.stride;
    if (lane == 0) o[0] = row;
    if (lane == 1) o[1] = l_lo[r];
    if (lane == 2) o[2] = l_hi[r];
    for (uint32_t i = lane; i < ws; i += 64) o[3 + i] = src[i];
  }
  if (c == 0) {
    const uint32_t* sc = (const uint32_t*)(bank + a.topo->scal_off);
    uint32_t* so = a.short_buf + (uint64_t)s * 6u * m;
    for (uint32_t i = threadIdx.x; i < 6u * m; i += GMX_CKPT_CHUNK) so[i] = sc[i];
  }
}

// grid: x = blocks of four waves striding over a mixer's records, y = mixer, z = stream
__global__ void __launch_bounds__(256) gmx_ckpt_scatter_kernel(const GmxCkptArgs a) {
  const uint32_t j = blockIdx.y, s = blockIdx.z;
  const uint32_t m = (uint32_t)a.topo->m;
  const GmxMixerDev& x = a.topo->mx[j];
  uint8_t* bank = a.banks + (uint64_t)s * a.topo->bank_bytes;
  const uint32_t cnt = a.mixer_cnt[(uint64_t)s * m + j];
  const uint32_t ws = x.weight_size, rec = 3u + ws;
  const uint32_t* in = a.long_buf + (a.mixer_off[(uint64_t)s * m + j] >> 2);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t r = blockIdx.x * 4u + wave; r < cnt; r += gridDim.x * 4u) {
    const uint32_t* p = in + (uint64_t)r * rec;
    const uint32_t row = p[0];
    if (row >= x.table_size) continue;  // (the host's validation has refused such a section already)
    uint32_t* dst = (uint32_t*)(bank + x.w_off) + (uint64_t)row * x.stride;
    for (uint32_t i = lane; i < ws; i += 64) dst[i] = p[3 + i];
    if (lane == 0) *GMX_RS_PTR(bank, x, row) = (uint64_t)p[1] | ((uint64_t)p[2] << 32);
  }
  if (blockIdx.x == 0 && threadIdx.x < 6u) {
    uint32_t* sc = (uint32_t*)(bank + a.topo->scal_off);
    sc[6u * j + threadIdx.x] = a.short_buf[(uint64_t)s * 6u * m + 6u * j + threadIdx.x];
  }
}

extern "C" hipError_t gmx_launch_ckpt_count(const GmxCkptArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ckpt_count_kernel, dim3(a->n_chunks, (unsigned)a->n_streams), dim3(GMX_CKPT_CHUNK), 0,
                     stream, *a);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_ckpt_pack(const GmxCkptArgs* a, hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ckpt_pack_kernel, dim3(a->n_chunks, (unsigned)a->n_streams), dim3(GMX_CKPT_CHUNK), 0,
                     stream, *a);
  return hipGetLastError();
}

extern "C" hipError_t gmx_launch_ckpt_scatter(const GmxCkptArgs* a, int n_mixers, unsigned blocks_x,
                                              hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_ckpt_scatter_kernel, dim3(blocks_x, (unsigned)n_mixers, (unsigned)a->n_streams), dim3(256),
                     0, stream, *a);
  return hipGetLastError();
}
