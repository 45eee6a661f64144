// gmx_ckpt_walk.h -- the device's walk over a chunk of a table whose live entries are to be counted, or placed in
// ascending order without sorting: the one copy that the checkpoint kernels share (gmx_match_ckpt.hip and
// gmx_ctx_ckpt.hip, the per-stream kernels of gmx_match.hip and gmx_ctx.hip; gmx_ind_ckpt.hip and gmx_ckpt.hip, whose
// entries are not u32, take the wave sum and the rank step).  Device code only; blocks are 256 lanes, four waves.
//
// A live entry's rank inside its chunk = live entries of the block's earlier rounds + of the waves below + of the lanes
// below (+ of the lane's own earlier entries, where a lane holds several).  What a record looks like and how it is
// stored -- bytes, dwords, an address looked at first -- is the caller's: nothing here stores into an image.
#ifndef GMX_CKPT_WALK_H_
#define GMX_CKPT_WALK_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

// a u32 at any byte address, least significant byte first
__device__ __forceinline__ void gmx_walk_put_u32(uint8_t* o, uint32_t v) {
  o[0] = (uint8_t)v;
  o[1] = (uint8_t)(v >> 8);
  o[2] = (uint8_t)(v >> 16);
  o[3] = (uint8_t)(v >> 24);
}
__device__ __forceinline__ uint32_t gmx_walk_get_u32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Entries e0 .. e0 + 3 of a chunk that begins at `tab` (one 16-byte load: e0 is a multiple of 4 and `tab` 16-byte
// aligned); entries at or beyond `end` read as 0, which is not live.
__device__ __forceinline__ uint4 gmx_walk_load4(const uint32_t* tab, uint32_t e0, uint32_t end) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (e0 < end) {
    v = *(const uint4*)(tab + e0);
    if (e0 + 1 >= end) v.y = 0u;
    if (e0 + 2 >= end) v.z = 0u;
    if (e0 + 3 >= end) v.w = 0u;
  }
  return v;
}

// Entries of the chunk that begins at `first_entry`: the chunk's length, clamped to the table's size.
__device__ __forceinline__ uint32_t gmx_walk_chunk_end(uint32_t size, uint32_t first_entry, uint32_t chunk) {
  const uint32_t left = size - first_entry;
  return left < chunk ? left : chunk;
}

// Sum of `v` (below 2^bits) over the wave, and over the lanes below this one: ballot + popcount per bit of v.
__device__ __forceinline__ void gmx_walk_wave_sum(uint32_t v, uint32_t bits, uint32_t* below, uint32_t* total) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint32_t b = 0, t = 0;
  for (uint32_t k = 0; k < bits; ++k) {
    const unsigned long long bal = __ballot((v >> k) & 1u);
    b += (uint32_t)__popcll(bal & lt) << k;
    t += (uint32_t)__popcll(bal) << k;
  }
  *below = b;
  *total = t;
}

// The cross-wave step of a round: every wave leaves its sum in wsum (LDS), one barrier, and every lane gets `rank`
// (what it counts below itself inside its wave and in earlier rounds) + the sums of the waves below its own
// (returned), and the sum of all four.  A loop passes two sets in turn, wsum[round & 1]: a wave that runs ahead writes
// the other set, and cannot come back to this one before every wave has passed the next barrier.
__device__ __forceinline__ uint32_t gmx_walk_rank_step(uint32_t* wsum /* LDS [4] */, uint32_t wave_total,
                                                       uint32_t rank, uint32_t* all) {
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) wsum[wave] = wave_total;
  __syncthreads();
  uint32_t sum = 0;
#pragma unroll
  for (unsigned w = 0; w < 4; ++w) {
    const uint32_t t = wsum[w];
    if (w < wave) rank += t;
    sum += t;
  }
  *all = sum;
  return rank;
}

// Non-zero entries among [0, end) of a chunk of u32 entries (at most 16 Ki: 16 iterations x 4 entries a lane), on
// every lane of the block.
__device__ __forceinline__ uint32_t gmx_walk_block_count_u32(const uint32_t* tab, uint32_t end,
                                                             uint32_t* wsum /* LDS [4] */) {
  uint32_t n = 0;
  for (uint32_t e0 = threadIdx.x * 4u; e0 < end; e0 += 1024u) {
    const uint4 v = gmx_walk_load4(tab, e0, end);
    n += (uint32_t)(v.x != 0u) + (uint32_t)(v.y != 0u) + (uint32_t)(v.z != 0u) + (uint32_t)(v.w != 0u);
  }
  uint32_t below, total, all;  // n <= 64: seven ballots
  gmx_walk_wave_sum(n, 7, &below, &total);
  (void)gmx_walk_rank_step(wsum, total, 0u, &all);
  return all;
}

// The non-zero entries among [0, end) of a chunk of u32 entries, in ascending order: put(rank, key, value) for each
// whose rank is below `room` (what the count pass found -- the banks do not change between the two passes: should they
// ever, a chunk still writes no more records than the scan gave it room for).  key = first_entry + index.  The loop
// is uniform over the block and ends once `room` records are placed.
template <class Put>
__device__ __forceinline__ void gmx_walk_pack_sparse_u32(const uint32_t* tab, uint32_t end, uint32_t first_entry,
                                                         uint32_t room, uint32_t (*wsum)[4] /* LDS [2][4] */,
                                                         Put put) {
  const unsigned lane = threadIdx.x & 63u;
  uint32_t done = 0, it = 0;
  for (uint32_t e0 = 0; e0 < end && done < room; e0 += 256u, ++it) {
    const uint32_t e = e0 + threadIdx.x;
    const uint32_t v = e < end ? tab[e] : 0u;
    const unsigned long long bal = __ballot(v != 0u);
    uint32_t all;
    const uint32_t r = gmx_walk_rank_step(wsum[it & 1u], (uint32_t)__popcll(bal),
                                          done + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)), &all);
    if (v != 0u && r < room) put(r, first_entry + e, v);
    done += all;
  }
}

// A launcher of a kernel whose grid is flat in x, 256 lanes a block: the last error is cleared, and a grid of no
// block, or of more than 31 bits, is refused.
#define GMX_WALK_LAUNCH(fn, args_t, kernel, grid)                                              \
  extern "C" hipError_t fn(const args_t* a, hipStream_t stream) {                              \
    (void)hipGetLastError();                                                                   \
    const uint64_t blocks_ = (grid);                                                           \
    if (blocks_ == 0 || blocks_ > 0x7fffffffull) return hipErrorInvalidValue;                  \
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks_), dim3(256), 0, stream, *a);             \
    return hipGetLastError();                                                                  \
  }

#endif  // GMX_CKPT_WALK_H_
