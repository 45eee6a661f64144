// gmx_pair.hip -- the lane-pair, register-resident bit loop of gmx_wide.hip for ANY three-layer bank:
// 4..256 inputs, 1..24 layer-0 mixers, 1..8 layer-1 mixers, a final mixer, one skip input at any index
// (gmx_topology_register_rows_eligible).  Opt-in: gmx_group_set_register_rows.
//
// gmx_wide.hip's design does not depend on its two literal shapes; what it needs at compile time is
// the REGISTER a weight lives in.  Here the input count n, the layer widths l0 / l1 and every table are run-time
// values, and the register positions stay constants because the row is split where that keeps them so:
//
//   * one wave = one stream.  Layer-0 mixer m is the lane pair (m, m+32).  With r = n % 4, U = HALF - 28 (a
//     constant of the instantiation) and LO = n - r - U, lane m holds stored floats [0, LO) of the row, lane m+32
//     holds [LO, LO + HALF): the last U + r inputs in registers 0 .. U+r-1, then the cascade weights (outputs of
//     layer-0 mixers 0..m-1, mixer.cpp:60-64) from register U + r on, then zero padding.  LO is a multiple of 4
//     (16-byte pieces), only r moves the cascade weights, and a wave-uniform switch over r picks one of four
//     compiled cascades.  An instantiation serves n - r in [HALF - 28, 2 * HALF - 28]:
//         HALF  32:   4 ..  39 inputs      HALF  96: 104 .. 167 inputs
//         HALF  64:  40 .. 103 inputs      HALF 144: 168 .. 256 inputs
//     (the host takes the smallest that fits; 4 inputs is the least any of them can split).
//   * the strict left-to-right sum (mixer.cpp:56-59) runs as the two phases of gmx_wide.hip: inputs [0, LO) in
//     lanes 0..l0-1 (a run-time quad count), the partial sums handed to lane+32 by ds_bpermute, the last U + r
//     inputs and the cascade there.  Nothing is multiplied by a padding zero that could be stale: the images of
//     the inputs in LDS are zero wherever a lane's registers are padding, and the r inputs of the quad the
//     cascade weights start in are added under `e < r`.
//   * layer-1 mixer k is lane 24 + k, the final mixer lane 56.  Their rows (l0 + k + 1 resp. l0 + l1 + 1 stored
//     weights) sit in nine register quads at positions that do not depend on l0 / l1: registers 0..23 face the
//     layer-0 outputs, 24..31 the own-layer inputs (stored float l0 + i), register 32 is the final mixer's skip
//     weight (stored float l0 + l1).  The lane reads and writes its staging slot float by float to get there.
//   * rows travel through a staging image in LDS in coalesced 16-byte pieces (global_load_lds_dwordx4 in, one
//     store per piece out), only when the gate context selects another row, and only the pieces that hold
//     weights: the row-step counter may live in the row's padding (the 90- and 256-input layouts) or in a table
//     of its own (everything else) -- GmxMixerDev::rs_off / rs_pitch say where, the layout is build_topology's.
//   * the update w -= update * x (mixer.cpp:129-172) runs on both halves at once; the layer-0 outputs are put
//     behind the inputs in the upper image, as the stored row has them, and a lane takes those below its own
//     weight_size.  Weights past weight_size see x = 0 and stay zero.
//   * the next bit's record is requested behind this bit's row traffic and collected by one s_waitcnt at the
//     end of the bit (request and wait in the same loop iteration).
// Per-block bit counts (GmxRunArgs::T_list) and the outputs of a stream's last bit (out_last) are served.
// Same floats as the general kernel and the oracle (tests/test_gpu_pair_kernel.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gmx_internal.h"
#include "gmx_math.h"

typedef float gmx_f4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kL0Max = 24, kL1Max = 8;
constexpr int kTail = 28;      // registers of an upper half behind its U full input quads: r <= 3 inputs + 23 cascade weights
constexpr int kQS = 9;         // quads of a layer-1 / final row in registers and in HBM (<= 33 of 64 stored floats)
constexpr int kFinLane = 56;
constexpr int kPitchS = 4 * kQS + 4;   // staging slot of a small row; floats 36..39 are never moved (scratch)

__device__ __forceinline__ void pair_ld16(gmx_f4& d, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(d) : "v"(p) : "memory");
}
__device__ __forceinline__ void pair_ld4(uint32_t& d, const void* p) {
  asm volatile("global_load_dword %0, %1, off" : "=v"(d) : "v"(p) : "memory");
}
__device__ __forceinline__ void pair_ld1(uint32_t& d, const void* p) {
  asm volatile("global_load_ubyte %0, %1, off" : "=v"(d) : "v"(p) : "memory");
}
__device__ __forceinline__ uint32_t rl_u(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ float rl_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ uint32_t pair_lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}
// One coalesced piece of a row, HBM -> LDS without a VGPR round trip: the lanes of `mask` move 16 bytes each
// from sbase + voff to LDS[lds_byte + 16 * lane] (LDS base in M0).  Called only where all 64 lanes of the wave
// are active (wave-uniform control flow, blocks of one full wave), so exec goes back to all ones; M0 is saved.
__device__ __forceinline__ void pair_dma16(uint64_t sbase, uint32_t voff, uint32_t lds_byte, uint64_t mask) {
  uint32_t sm0;
  asm volatile(
      "s_mov_b64 exec, %3\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %2, %1 nt\n\ts_mov_b32 m0, %0\n\ts_mov_b64 exec, -1"
      : "=&s"(sm0)
      : "s"(sbase), "v"(voff), "s"(mask), "s"(lds_byte)
      : "memory");
}
// ... and back: the lanes of `mask` store 16 bytes each to sbase + voff.
__device__ __forceinline__ void pair_st16(uint64_t sbase, uint32_t voff, const gmx_f4& v, uint64_t mask) {
  asm volatile(
      "s_mov_b64 exec, %3\n\t"
      "global_store_dwordx4 %1, %2, %0 nt\n\ts_mov_b64 exec, -1"
      :
      : "s"(sbase), "v"(voff), "v"(v), "s"(mask)
      : "memory");
}
__device__ __forceinline__ float el(const gmx_f4& v, int e) { return e == 0 ? v.x : (e == 1 ? v.y : (e == 2 ? v.z : v.w)); }
__device__ __forceinline__ void set_el(gmx_f4& v, int e, float f) {
  if (e == 0) v.x = f; else if (e == 1) v.y = f; else if (e == 2) v.z = f; else v.w = f;
}

}  // namespace

template <int HALF, bool HAS_MASK>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2)))
gmx_pair_kernel(const GmxTopoDev* __restrict__ tp, const GmxRunArgs a) {
  constexpr int kQ = HALF / 4;           // register quads per lane
  constexpr int kU = HALF - kTail;       // inputs an upper half faces in full quads
  constexpr int kQF = kU / 4;            // ... and their count; quad kQF starts with the r inputs left over
  constexpr int kPitch = HALF + 4;       // staging slots of layer-0 halves: odd quad pitch, conflict-free transposed reads
  constexpr int kQR = kQ > kQS ? kQ : kQS;  // register quads: a small row needs nine even where a half has eight
  static_assert(HALF % 8 == 0 && kU >= 4 && (kPitch / 4) % 2 == 1, "bucket");
  // inputs of the bit: [0, HALF) what the lower halves face (inputs [0, LO), then zeros), [HALF, 2 HALF) what the
  // upper halves face (inputs [LO, n), then the layer-0 outputs, then zeros)
  __shared__ __attribute__((aligned(16))) float ximg[2 * HALF];
  __shared__ uint64_t s_tab[32];
  extern __shared__ __attribute__((aligned(16))) float stage[];  // 2 l0 halves, then l1 + 1 small rows
  const int lane = threadIdx.x;
  const int rec = a.rec_base + (int)blockIdx.x;
  const int s = a.stream_base + (int)blockIdx.x;
  const uint64_t T = a.T_list ? a.T_list[blockIdx.x] : a.T;  // (wave-uniform: one stream per block)
  if (T == 0) return;
  const int n = tp->n, l0 = tp->l0, l1 = tp->l1, n_pad = tp->n_pad, MW = tp->mask_words;
  const int M = l0 + l1 + 1;
  const int r = n & 3;
  const int LO = n - r - kU;             // floats of a lower half, a multiple of 4 in [0, HALF] (the host checked)
  const int stage_small = 2 * l0 * kPitch;
  const int stage_floats = stage_small + (l1 + 1) * kPitchS;
  if (lane < 32) s_tab[lane] = gmx_exp2f_tab[lane];
  // the images start out zero: the padding pieces of a row are not fetched, so what the owner reads there must
  // be the zeros the write-back path put (or these); the inputs' padding is never written at all
  for (int i = 4 * lane; i < stage_floats; i += 256) *(gmx_f4*)(stage + i) = gmx_f4{0.f, 0.f, 0.f, 0.f};
  for (int i = 4 * lane; i < 2 * HALF; i += 256) *(gmx_f4*)(ximg + i) = gmx_f4{0.f, 0.f, 0.f, 0.f};
  const bool do_learn = (a.mode & GMX_MODE_LEARN) != 0;
  uint8_t* const bank = a.banks + (uint64_t)s * tp->bank_bytes;

  // ---- who this lane is ------------------------------------------------------------------
  const int half = lane >> 5, li = lane & 31;
  const int k1 = li - kL0Max;                                 // output index of a layer-1 lane
  const bool is_l0 = li < l0;                                 // both halves of a layer-0 pair
  const bool is_l1 = half == 0 && k1 >= 0 && k1 < l1;         // lanes 24 .. 24 + l1 - 1
  const bool is_fin = lane == kFinLane;
  const bool act = is_l0 || is_l1 || is_fin;
  const bool owner = act && !(is_l0 && half);                 // writes the row's step counter and the mixer's scalars
  const int mxi = is_fin ? M - 1 : (is_l1 ? l0 + k1 : (is_l0 ? li : 0));
  const GmxMixerDev d = tp->mx[mxi];
  const int skip_idx = tp->skip_idx[0];
  const bool all_pow2 = __ballot(act && (d.table_size & (d.table_size - 1u)) != 0) == 0;
  uint64_t* const scal = (uint64_t*)(bank + tp->scal_off) + 3 * mxi;
  uint64_t steps = 0, max_steps = 1, seen_cnt = 0;
  if (act) {
    steps = scal[0];
    max_steps = scal[1];
    seen_cnt = scal[2];
  }
  uint8_t* const rs_tab = bank + d.rs_off;
  const uint32_t rs_pitch = d.rs_pitch;
  uint8_t* const w_tab = bank + d.w_off + ((is_l0 && half) ? (uint32_t)LO * 4u : 0u);
  const uint32_t row_bytes = d.stride * 4u;
  // staging slot of this lane's row piece and its length in 16-byte lanes (0: nothing to move)
  const uint32_t my_off = is_l0 ? (uint32_t)((half * l0 + li) * kPitch)
                                : (uint32_t)(stage_small + (is_fin ? l1 : (is_l1 ? k1 : 0)) * kPitchS);
  const uint32_t my_pieces = !act ? 0u : is_l0 ? (half ? (uint32_t)(kU + r + li + 3) / 4u : (uint32_t)LO / 4u) : (uint32_t)kQS;
  float* const my_stage = stage + my_off;
  // a small row's registers: position p < 24 is stored float p (layer-0 output p), 24 + i stored float l0 + i (the
  // own-layer input i), 32 stored float l0 + l1 (the final mixer's skip weight); vs_*: the positions this row has
  const uint32_t wsz = d.weight_size;
  uint32_t vs_lo = 0, vs_hi = 0;
  if (is_l1 || is_fin) {
    vs_lo = l0 >= 32 ? ~0u : ((1u << l0) - 1u);
    const int own = is_fin ? l1 : k1 + 1;  // own-layer inputs: the mixers before it and its skip input / all of them
    vs_lo |= ((1u << own) - 1u) << kL0Max;
    vs_hi = is_fin ? 1u : 0u;
  }
  float* const small_own = my_stage + l0 - kL0Max;  // + p: stored float l0 + (p - 24)

  const uint64_t RS = a.rec_stride;
  const float* const pred_s = a.pred + (uint64_t)rec * RS * (uint64_t)n_pad;
  const uint32_t* const mask_s = HAS_MASK ? a.mask + (uint64_t)rec * RS * (uint64_t)MW : nullptr;
  const uint32_t* const ctx_s = a.ctx + (uint64_t)rec * RS * (uint64_t)M;
  const uint8_t* const bits_s = a.bits + (uint64_t)rec * RS;
  const float* const dec_s = a.decay + (uint64_t)a.decay_idx[blockIdx.x] * a.T;
  float* const p_s = a.p_out + (uint64_t)rec * RS;
  float* const oa_s = a.out_all ? a.out_all + (uint64_t)rec * RS * (uint64_t)M : nullptr;

  // ---- the resident row ---------------------------------------------------------------------
  gmx_f4 w[kQR];
#pragma unroll
  for (int q = 0; q < kQR; ++q) w[q] = gmx_f4{0.f, 0.f, 0.f, 0.f};
  uint32_t tag = 0xffffffffu;
  uint64_t rs = 0;      // MixerData::steps of the resident row (long-term-memory.h:29)
  bool dirty = false;

  const uint32_t stage_base = pair_lds_addr(stage);
  const uint32_t lane16 = (uint32_t)lane * 16u;
  // registers -> staging slot (all of a layer-0 half: its padding registers are zero; a small row float by float,
  // positions it does not have into the slot's scratch float)
  auto to_stage = [&](bool on) {
    if (on && is_l0) {
#pragma unroll
      for (int q = 0; q < kQ; ++q) *(gmx_f4*)(my_stage + 4 * q) = w[q];
    }
    if (on && !is_l0) {
#pragma unroll
      for (int p = 0; p <= kL0Max + kL1Max; ++p) {
        const bool v = p < 32 ? ((vs_lo >> p) & 1u) != 0 : vs_hi != 0;
        float* const at = p < kL0Max ? my_stage + p : (p < kL0Max + kL1Max ? small_own + p : small_own + kL0Max + l1);
        *(v ? at : my_stage + 4 * kQS) = el(w[p / 4], p % 4);
      }
    }
  };
  auto from_stage = [&](bool on) {
    if (on && is_l0) {
#pragma unroll
      for (int q = 0; q < kQ; ++q) w[q] = *(const gmx_f4*)(my_stage + 4 * q);
    }
    if (on && !is_l0) {
#pragma unroll
      for (int p = 0; p <= kL0Max + kL1Max; ++p) {
        const bool v = p < 32 ? ((vs_lo >> p) & 1u) != 0 : vs_hi != 0;
        const float* const at = p < kL0Max ? my_stage + p : (p < kL0Max + kL1Max ? small_own + p : small_own + kL0Max + l1);
        const float f = *(v ? at : my_stage + 4 * kQS);
        set_el(w[p / 4], p % 4, v ? f : 0.f);
      }
    }
  };
  auto evict = [&](bool ev) {
    uint64_t em = __ballot(ev);
    if (em == 0) return;
    const uint64_t dst = (uint64_t)(w_tab + (uint64_t)tag * row_bytes);
    const uint32_t dlo = (uint32_t)dst, dhi = (uint32_t)(dst >> 32);
    to_stage(ev);
    if (ev && owner) *(uint64_t*)(rs_tab + (uint64_t)tag * rs_pitch) = rs;
    while (em) {
      const int h = __builtin_ctzll(em);
      em &= em - 1;
      const uint32_t pcs = rl_u(my_pieces, h);
      if (pcs == 0) continue;
      const uint32_t off = rl_u(my_off, h);
      const uint64_t sb = ((uint64_t)rl_u(dhi, h) << 32) | rl_u(dlo, h);
      const gmx_f4 v = *(const gmx_f4*)(stage + off + 4 * ((uint32_t)lane < pcs ? lane : 0));
      pair_st16(sb, lane16, v, (1ull << pcs) - 1ull);
    }
  };
  // the rows of the lanes in `nm` (non-empty) from HBM into the staging image
  auto fetch = [&](uint64_t nm, uint64_t src) {
    const uint32_t slo = (uint32_t)src, shi = (uint32_t)(src >> 32);
    while (nm) {
      const int h = __builtin_ctzll(nm);
      nm &= nm - 1;
      const uint32_t pcs = rl_u(my_pieces, h);
      if (pcs == 0) continue;
      const uint32_t off = rl_u(my_off, h);
      const uint64_t sb = ((uint64_t)rl_u(shi, h) << 32) | rl_u(slo, h);
      pair_dma16(sb, lane16, stage_base + off * 4u, (1ull << pcs) - 1ull);
    }
  };

  // ---- prefetched record fields (_n: of the bit about to be computed) --------------------
  uint32_t ctx_n = 0, mask_n = ~0u, bit_n = 0, dec_n = 0;
  gmx_f4 x_n = gmx_f4{0.f, 0.f, 0.f, 0.f};
  const bool has_x = 4 * lane < n_pad;
  auto request = [&](uint64_t t) {
    const uint64_t tt = t < T ? t : T - 1;  // past the end: a harmless re-read of the last record
    pair_ld4(ctx_n, ctx_s + tt * (uint64_t)M + mxi);
    pair_ld16(x_n, pred_s + tt * (uint64_t)n_pad + 4 * (has_x ? lane : 0));
    if (HAS_MASK) pair_ld4(mask_n, mask_s + tt * (uint64_t)MW + (lane < MW ? lane : 0));
    pair_ld1(bit_n, bits_s + tt);
    pair_ld4(dec_n, dec_s + tt);
  };
  // The wait that releases a request sits in the SAME loop iteration as the request (at its end):
  // across the back edge the compiler may copy the destination registers before the data is in.
  auto landed = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(ctx_n), "+v"(x_n), "+v"(mask_n), "+v"(bit_n), "+v"(dec_n));
  };
  request(0);
  landed();

  // where this lane's quad of the record goes in the images, and which of its four slots are inputs at all
  float* const x_at = ximg + (4 * lane < LO ? 4 * lane : HALF + 4 * lane - LO);
  const int n_here = n - 4 * lane;
  const uint32_t in_bits = n_here >= 4 ? 15u : (n_here > 0 ? (1u << n_here) - 1u : 0u);
  // what a lane multiplies its registers with in the update: its half's image, upper halves up to their own
  // weight_size (inputs, then the outputs of the layer-0 mixers before this one)
  const float* const x_from = ximg + (half ? HALF : 0);
  const int x_lim = half ? (int)wsz - LO : HALF;
  // the quads any lane has weights in
  const int ext = max(max(LO, kU + r + l0 - 1), 4 * kQS);

  for (uint64_t t = 0; t < T; ++t) {
    const uint32_t ctx = ctx_n, mword = mask_n, bit = bit_n & 1u;
    const float dec = __uint_as_float(dec_n);
    const gmx_f4 xv = x_n;

    // ---- FindMixerData (mixer.cpp:29-37): replace the resident row if the context moved ----
    const uint32_t row = all_pow2 ? (ctx & (d.table_size - 1u)) : (ctx % d.table_size);
    const bool need = act && row != tag;
    evict(need && dirty);
    const uint64_t nm = __ballot(need);
    if (nm) {
      // the staging image is free again once the write-back has read it (its ds_reads are done:
      // their data went into the stores above)
      fetch(nm, (uint64_t)(w_tab + (uint64_t)row * row_bytes));
      if (need) rs = *(const uint64_t*)(rs_tab + (uint64_t)row * rs_pitch);
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(rs) : : "memory");
      from_stage(need);
      if (need) {
        tag = row;
        dirty = false;
      }
    }
    request(t + 1);  // a whole bit ahead of its use

    // ---- the blackboard of this bit into LDS ----------------------------------------------
    // the skip input is read raw, possibly stale (mixer.cpp:76-79)
    const float skip = rl_f(el(xv, skip_idx & 3), skip_idx >> 2);
    {
      // only active_models are visited (mixer.cpp:57-59): silent slots contribute nothing; neither does the
      // record's padding behind input n-1
      uint32_t b = in_bits;
      if (HAS_MASK) {
        const uint32_t word = (uint32_t)__builtin_amdgcn_ds_bpermute((has_x ? (lane >> 3) : 0) << 2, (int)mword);
        b &= word >> ((4u * (uint32_t)lane) & 31u);
      }
      gmx_f4 v = xv;
      v.x = (b & 1u) ? v.x : 0.f;
      v.y = (b & 2u) ? v.y : 0.f;
      v.z = (b & 4u) ? v.z : 0.f;
      v.w = (b & 8u) ? v.w : 0.f;
      if (has_x) *(gmx_f4*)x_at = v;
    }
    const bool seen = act && rs != 0;  // an unseen row is "no row": output 0 (mixer.cpp:52-55)

    // ---- layer 0, inputs [0, LO) in lanes 0..l0-1 (mixer.cpp:56-59) -----------------------
    float acc = 0.f;
#pragma unroll
    for (int q0 = 0; q0 < kQ; q0 += 4) {
      if (4 * q0 < LO) {  // (behind LO the image and the registers are both zero: whole groups are skipped for speed)
#pragma unroll
        for (int q = q0; q < q0 + 4 && q < kQ; ++q) {
          const gmx_f4 x = *(const gmx_f4*)(ximg + 4 * q);
          acc = acc + x.x * w[q].x;
          acc = acc + x.y * w[q].y;
          acc = acc + x.z * w[q].z;
          acc = acc + x.w * w[q].w;
        }
      }
    }
    // ---- ... handed to lanes 32.., which go on with inputs [LO, n) -------------------------
    acc = __int_as_float(__builtin_amdgcn_ds_bpermute((lane & 31) << 2, __float_as_int(acc)));
#pragma unroll
    for (int q = 0; q < kQF; ++q) {
      const gmx_f4 x = *(const gmx_f4*)(ximg + HALF + 4 * q);
      acc = acc + x.x * w[q].x;
      acc = acc + x.y * w[q].y;
      acc = acc + x.z * w[q].z;
      acc = acc + x.w * w[q].w;
    }
    {
      const gmx_f4 x = *(const gmx_f4*)(ximg + HALF + kU);
      if (r > 0) acc = acc + x.x * w[kQF].x;
      if (r > 1) acc = acc + x.y * w[kQF].y;
      if (r > 2) acc = acc + x.z * w[kQF].z;
    }
    acc = seen ? acc : 0.f;
    // ---- layer-0 cascade: mixer k adds outputs 0..k-1 in order (mixer.cpp:60-64) -----------
    float o0[kL0Max];
    const bool up0 = is_l0 && half && seen;
    auto cascade = [&](auto rc) {
      constexpr int R = decltype(rc)::value;
#pragma unroll
      for (int i = 0; i < kL0Max; ++i) {
        o0[i] = rl_f(acc, 32 + i);   // (0 for i >= l0: not `seen`)
        if (i + 1 < kL0Max) {
          const float wt = el(w[(kU + R + i) / 4], (kU + R + i) % 4);
          acc = (up0 && li > i) ? acc + o0[i] * wt : acc;
        }
      }
    };
    switch (r) {
      case 0: cascade(std::integral_constant<int, 0>()); break;
      case 1: cascade(std::integral_constant<int, 1>()); break;
      case 2: cascade(std::integral_constant<int, 2>()); break;
      default: cascade(std::integral_constant<int, 3>()); break;
    }
    // the outputs behind the inputs of the upper image, as the stored row has them
    if (is_l0 && half) ximg[HALF + kU + r + li] = acc;
    // ---- layers 1 and 2: the layer-0 outputs first (mixer.cpp:66-68, 82-84) ----------------
    const bool up1 = (is_l1 || is_fin) && seen;
    float a1 = 0.f;
#pragma unroll
    for (int i = 0; i < kL0Max; ++i) a1 = a1 + o0[i] * el(w[i / 4], i % 4);
    a1 = up1 ? a1 : 0.f;
    // layer-1 cascade, each mixer's skip input when its turn comes (mixer.cpp:69-80); the final
    // mixer takes every layer-1 output, then the skip input (mixer.cpp:85-97)
    float o1[kL1Max];
#pragma unroll
    for (int i = 0; i < kL1Max; ++i) {
      const float wt = el(w[(kL0Max + i) / 4], (kL0Max + i) % 4);
      a1 = (is_l1 && k1 == i && seen) ? a1 + skip * wt : a1;
      o1[i] = rl_f(a1, kL0Max + i);  // (0 for i >= l1)
      a1 = (((is_l1 && k1 > i) || is_fin) && seen) ? a1 + o1[i] * wt : a1;
    }
    a1 = (is_fin && seen) ? a1 + skip * w[(kL0Max + kL1Max) / 4].x : a1;
    static_assert((kL0Max + kL1Max) % 4 == 0, "the final mixer's skip weight is element 0 of its quad");

    // every lane's own mixer output (both halves of a layer-0 pair hold it)
    const float own0 = __int_as_float(__builtin_amdgcn_ds_bpermute((32 + (lane & 31)) << 2, __float_as_int(acc)));
    const float own = is_l0 ? own0 : a1;
    // Sigmoid::Logistic of it: the final mixer's is Predictor::Predict's result after clamping
    // (predictor.cpp:369-375), all of them feed Mixer::Learn (mixer.cpp:113-122)
    const float pl = gmx_logistic_tab(own, s_tab);
    if (is_fin) p_s[t] = gmx_clamp_prob(pl);
    if (oa_s && owner) oa_s[t * (uint64_t)M + mxi] = own;
    if (a.out_last && owner && t + 1 == T) a.out_last[(uint64_t)rec * M + mxi] = own;

    if (do_learn) {
      // ---- Mixer::Learn (mixer.cpp:108-176) --------------------------------------------------
      const double dd = (double)dec * (1.5 - ((double)rs) / (double)max_steps);  // mixer.cpp:112
      const float decay = (float)dd;
      const float upd = decay * d.lr * (pl - (float)bit);  // mixer.cpp:123
      const uint64_t rs_new = rs + 1;
      const float scl = ((rs_new & 1023u) == 0) ? (1.0f - 3.0e-6f) : 1.0f;  // mixer.cpp:173-175; * 1.0f is exact
      if (act) {
        ++steps;
        if (rs_new > max_steps) max_steps = rs_new;
        if (rs == 0) ++seen_cnt;  // FindOrCreateMixerData (mixer.cpp:44-46)
        rs = rs_new;
        dirty = true;             // row and counter go back to HBM when the row is replaced
      }
      // w -= update * x over the segments Predict walked (mixer.cpp:129-172)
#pragma unroll
      for (int q = 0; q < kQR; ++q) {
        if (4 * q >= ext) continue;  // (wave-uniform) no lane has weights here: zeros stay zeros
        gmx_f4 x = gmx_f4{0.f, 0.f, 0.f, 0.f};
        if (q < kQ) x = *(const gmx_f4*)(x_from + 4 * q);
        if (q >= kQF && q < kQ) {
          // behind an upper half's full input quads: its last r inputs, the outputs of the layer-0 mixers before
          // it, then padding (lower halves: x_lim = HALF, their image is zero behind LO by itself)
          x.x = 4 * q + 0 < x_lim ? x.x : 0.f;
          x.y = 4 * q + 1 < x_lim ? x.y : 0.f;
          x.z = 4 * q + 2 < x_lim ? x.z : 0.f;
          x.w = 4 * q + 3 < x_lim ? x.w : 0.f;
        }
        if (q < kQS) {
          // layer-1 / final rows: layer-0 outputs, own-layer outputs before this mixer (all of
          // them for the final mixer), the skip input, padding
          float sm[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int idx = 4 * q + e;
            float v = 0.f;
            if (idx < kL0Max) {
              v = o0[idx];
            } else if (idx < kL0Max + kL1Max) {
              const int i = idx - kL0Max;
              v = (is_fin || k1 > i) ? o1[i] : (k1 == i ? skip : 0.f);
            } else if (idx == kL0Max + kL1Max) {
              v = is_fin ? skip : 0.f;
            }
            sm[e] = v;
          }
          x.x = is_l0 ? x.x : sm[0];
          x.y = is_l0 ? x.y : sm[1];
          x.z = is_l0 ? x.z : sm[2];
          x.w = is_l0 ? x.w : sm[3];
        } else {
          x.x = is_l0 ? x.x : 0.f;
          x.y = is_l0 ? x.y : 0.f;
          x.z = is_l0 ? x.z : 0.f;
          x.w = is_l0 ? x.w : 0.f;
        }
        w[q].x = (w[q].x - upd * x.x) * scl;
        w[q].y = (w[q].y - upd * x.y) * scl;
        w[q].z = (w[q].z - upd * x.z) * scl;
        w[q].w = (w[q].w - upd * x.w) * scl;
      }
    }
    landed();  // requested a whole bit's work ago: no stall
  }
  evict(act && dirty);
  if (owner && do_learn) {
    scal[0] = steps;
    scal[1] = max_steps;
    scal[2] = seen_cnt;
  }
}

// The instantiation a bank of n inputs takes: floats per lane of a pair, 0 when none serves it.
extern "C" int gmx_pair_kernel_half(int n_inputs) {
  if (n_inputs < 4 || n_inputs > 256) return 0;
  const int n4 = n_inputs & ~3;
  return n4 <= 2 * 32 - kTail ? 32 : n4 <= 2 * 64 - kTail ? 64 : n4 <= 2 * 96 - kTail ? 96 : 144;
}

// Eligible (the host checked, gmx_topology_register_rows_eligible): 4..256 inputs, 1..24 layer-0 + 1..8 layer-1 +
// final, one skip input, batched Predict(+Learn).
extern "C" hipError_t gmx_launch_pair_kernel(const GmxTopoDev* tp_dev, const GmxRunArgs* args, int n_streams,
                                             int has_mask, int n_inputs, int l0, int l1, hipStream_t stream) {
  (void)hipGetLastError();
  const int half = gmx_pair_kernel_half(n_inputs);
  if (half == 0 || l0 < 1 || l0 > kL0Max || l1 < 1 || l1 > kL1Max) return hipErrorInvalidValue;
  const int lo = (n_inputs & ~3) - (half - kTail);
  if (lo < 0 || lo > half) return hipErrorInvalidValue;
  const dim3 grid(n_streams), block(64);
  const size_t lds = ((size_t)2 * l0 * (half + 4) + (size_t)(l1 + 1) * kPitchS) * sizeof(float);
#define GMX_PAIR_LAUNCH(H)                                                                          \
  do {                                                                                              \
    if (has_mask)                                                                                   \
      hipLaunchKernelGGL((gmx_pair_kernel<H, true>), grid, block, lds, stream, tp_dev, *args);      \
    else                                                                                            \
      hipLaunchKernelGGL((gmx_pair_kernel<H, false>), grid, block, lds, stream, tp_dev, *args);     \
  } while (0)
  switch (half) {
    case 32: GMX_PAIR_LAUNCH(32); break;
    case 64: GMX_PAIR_LAUNCH(64); break;
    case 96: GMX_PAIR_LAUNCH(96); break;
    default: GMX_PAIR_LAUNCH(144); break;
  }
#undef GMX_PAIR_LAUNCH
  return hipGetLastError();
}
