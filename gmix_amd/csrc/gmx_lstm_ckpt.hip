// gmx_lstm_ckpt.hip -- the checkpoint of a whole LSTM group on the device (gfx950): pack the banks of a slice of
// consecutive streams into the staging buffer in the reference's file layout (the LSTM section of the `.long` file, or
// LstmModel's stretch of `.short`), and scatter such sections back into banks.  The layouts are gmx_lstm_ckpt.h's
// segment table; one block moves one tile of it for one stream, so a launch is a flat grid of streams x tiles.
//
// No arithmetic happens here: every value travels as a 32-bit pattern.  A section starts at a multiple of its size
// (5 560 200 = 8 mod 16, 1 458 256 with every field 12 bytes off a 16-byte boundary) in a buffer that the runtime
// aligns, so 4 bytes is all that a file-side address is guaranteed: every access to the staging buffer is one dword
// per lane, the lanes of a wave on consecutive dwords.  The bank side is read and written the same way: a wave's 64
// consecutive dwords are 256 contiguous bytes on either side, and the link, not the device, bounds a checkpoint
// (DESIGN 4.19).
//
// The two transposes go through an LDS tile so that BOTH sides are contiguous per wave:
//   out_layer   file [symbol][51 hidden], bank [51 hidden][256 symbols].  Tile = 64 symbols of one epoch: 3 264
//               consecutive file words; in the bank 51 rows of 64 consecutive words.  LDS holds the tile in file order,
//               pitch 51.  The transposed side has lane = symbol at a fixed hidden unit: word 51 * lane + j.  51 is odd,
//               so the 32 lanes that ds_read_b32 / ds_write_b32 serve together fall on 32 different banks -- the row
//               length is its own padding.
//   cell_major  file [50 cells][563 inputs], bank gmx_l_mat(input, cell).  Tile = 64 inputs x 50 cells: in the file 50
//               rows of 64 consecutive words; in the bank 4 096 consecutive words -- [input][64 cells] for the symbol
//               rows, [block of 4 inputs][64 cells][4] for the layer-input rows.  LDS holds [cell][input] at a padded
//               pitch.  The bank side walks its 4 096 words in order: for the symbol rows a wave is 64 cells of one
//               input, word pitch * cell + input, conflict-free at pitch 65; for the layer-input rows a wave is 16
//               cells x 4 inputs, word pitch * cell + q, and 32 lanes (8 cells x 4) are on 32 banks at pitch 68
//               (68 c + q = 4 c + q mod 32).  The file side reads rows: consecutive words, any pitch.
// The pitch-changing rows and the plain vectors are element-parallel: lane = file word.
//
//   pack      bank -> staging buffer.  The range header comes from the host's per-stream record or from scal[3] / [6].
//   scatter   staging buffer -> bank.  The host has cleared the banks, so padding and every field the file leaves out
//             stay zero: no lane writes a padding word.  scal[0 .. 6] come from the host's per-stream record (the bit
//             prediction is the host's logf), lin_t is written beside layer_input, hidden[50] becomes 1.0f.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmx_lstm_ckpt.h"

static_assert(GMX_L_HID % 2 == 1, "the out_layer tile's pitch is odd: no padding needed");
static_assert(sizeof(GmxLstmCkptSeg) == 48 && sizeof(GmxLstmCkptTile) == 8, "host and device agree");
#define GMX_LCK_PITCH_SYM 65u
#define GMX_LCK_PITCH_LIN 68u
#define GMX_LCK_LDS_WORDS (GMX_L_NC * GMX_LCK_PITCH_LIN)
static_assert(GMX_LCK_LDS_WORDS >= GMX_LCK_JTILE * GMX_L_HID, "one LDS array serves both transposes");
static_assert(GMX_LCK_JTILE == 64, "a wave is a tile's row");

template <bool IMPORT>
__device__ __forceinline__ void gmx_lstm_ckpt_block(const GmxLstmCkptArgs& a) {
  __shared__ uint32_t lds[GMX_LCK_LDS_WORDS];
  const uint32_t s = blockIdx.x / a.n_tiles, t = blockIdx.x % a.n_tiles;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const GmxLstmCkptTile tl = a.half->tile[t];
  const GmxLstmCkptSeg& sg = a.half->seg[tl.seg];
  uint32_t* const bank = a.banks + (uint64_t)s * a.bank_floats;
  uint32_t* const file = (uint32_t*)(a.buf + (uint64_t)s * a.stride + sg.file_off);
  const uint32_t kind = sg.kind;

  if (kind == GMX_LCK_OUT_LAYER) {
    const uint32_t e = tl.first / GMX_L_NO, i0 = tl.first % GMX_L_NO;
    uint32_t* const rows = bank + sg.bank_off + (uint64_t)e * GMX_L_HID * GMX_L_NO + i0 + lane;
    uint32_t* const words = file + (uint64_t)tl.first * GMX_L_HID;
    const uint32_t n = GMX_LCK_JTILE * GMX_L_HID;
    if (!IMPORT) {
      for (uint32_t j = wave; j < GMX_L_HID; j += 4) lds[lane * GMX_L_HID + j] = rows[j * GMX_L_NO];
      __syncthreads();
      for (uint32_t k = tid; k < n; k += 256) words[k] = lds[k];
    } else {
      for (uint32_t k = tid; k < n; k += 256) lds[k] = words[k];
      __syncthreads();
      for (uint32_t j = wave; j < GMX_L_HID; j += 4) rows[j * GMX_L_NO] = lds[lane * GMX_L_HID + j];
    }
    return;
  }

  if (kind == GMX_LCK_CELL_MAJOR) {
    const uint32_t j0 = tl.first;
    const uint32_t nj = GMX_L_W - j0 < GMX_LCK_JTILE ? GMX_L_W - j0 : GMX_LCK_JTILE;
    const bool sym = j0 < GMX_L_NO;
    const uint32_t pitch = sym ? GMX_LCK_PITCH_SYM : GMX_LCK_PITCH_LIN;
    // the tile's 4 096 consecutive bank words (fewer in the last tile: bounded by nj below); in either part of
    // gmx_l_mat an input takes GMX_L_CP words
    uint32_t* const mat = bank + sg.bank_off + (uint64_t)j0 * GMX_L_CP;
    uint32_t* const rows = file + j0 + lane;
    if (IMPORT) {
      for (uint32_t c = wave; c < GMX_L_NC; c += 4)
        if (lane < nj) lds[c * pitch + lane] = rows[c * GMX_L_W];
      __syncthreads();
    }
    for (uint32_t w = tid; w < GMX_LCK_JTILE * GMX_L_CP; w += 256) {
      uint32_t jj, c;
      if (sym) {
        jj = w >> 6;
        c = w & 63u;
      } else {
        jj = (w >> 8) * 4u + (w & 3u);
        c = (w >> 2) & 63u;
      }
      if (c < GMX_L_NC && jj < nj) {  // neither a padding cell nor an input beyond the matrix
        if (IMPORT) mat[w] = lds[c * pitch + jj];
        else lds[c * pitch + jj] = mat[w];
      }
    }
    if (!IMPORT) {
      __syncthreads();
      for (uint32_t c = wave; c < GMX_L_NC; c += 4)
        if (lane < nj) rows[c * GMX_L_W] = lds[c * pitch + lane];
    }
    return;
  }

  // ---- element-parallel: lane = file word
  const uint32_t end = sg.floats - tl.first < GMX_LCK_TILE ? sg.floats : tl.first + GMX_LCK_TILE;
  if (kind == GMX_LCK_RANGE) {
    if (!IMPORT) {
      if (tid < 3u) {
        const GmxLstmCkptOut r = a.out[s];
        const uint32_t* scal = bank + a.half->scal;
        int32_t tmb[3] = {255, 127, 0};
        if (r.fixed) {
          tmb[0] = r.tmb[0];
          tmb[1] = r.tmb[1];
          tmb[2] = r.tmb[2];
        } else if (scal[6]) {  // the eighth bit of the last coded byte: [b & ~1, b | 1], mid_ = bot_
          tmb[2] = (int32_t)(scal[3] & 0xfeu);
          tmb[1] = tmb[2];
          tmb[0] = tmb[2] + 1;
        }
        file[tid] = (uint32_t)(tid == 0 ? tmb[0] : tid == 1 ? tmb[1] : tmb[2]);
      }
    } else if (tid < 7u) {  // the block of the section's first segment also stores what the host derived from it
      bank[a.half->scal + tid] = a.in[s].scal[tid];
    }
    return;
  }
  if (kind == GMX_LCK_SCAL) {
    if (!IMPORT)
      for (uint32_t k = tl.first + tid; k < end; k += 256) file[k] = k < sg.n ? bank[sg.bank_off + k] : 0u;
    return;  // (import: the host's record has them)
  }
  const uint32_t n = sg.n, bpitch = sg.pitch;
  for (uint32_t k = tl.first + tid; k < end; k += 256) {
    const uint32_t r = kind == GMX_LCK_ROWS ? k / n : 0u, col = kind == GMX_LCK_ROWS ? k % n : k;
    uint32_t* const p = bank + sg.bank_off + (uint64_t)r * bpitch + col;
    if (!IMPORT) {
      file[k] = *p;
    } else {
      const uint32_t v = k == sg.one_at ? 0x3f800000u : file[k];
      *p = v;
      if (sg.twin) bank[sg.twin + (uint64_t)col * GMX_L_HP + r] = v;
    }
  }
}

__global__ void __launch_bounds__(256) gmx_lstm_ckpt_pack_kernel(const GmxLstmCkptArgs a) {
  gmx_lstm_ckpt_block<false>(a);
}

__global__ void __launch_bounds__(256) gmx_lstm_ckpt_scatter_kernel(const GmxLstmCkptArgs a) {
  gmx_lstm_ckpt_block<true>(a);
}

#define GMX_LCK_LAUNCH(fn, kernel)                                                             \
  extern "C" hipError_t fn(const GmxLstmCkptArgs* a, hipStream_t stream) {                     \
    (void)hipGetLastError();                                                                   \
    const uint64_t blocks_ = (uint64_t)a->n_streams * a->n_tiles;                              \
    if (a->n_streams < 1 || blocks_ == 0 || blocks_ > 0x7fffffffull) return hipErrorInvalidValue; \
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks_), dim3(256), 0, stream, *a);             \
    return hipGetLastError();                                                                  \
  }
GMX_LCK_LAUNCH(gmx_launch_lstm_ckpt_pack, gmx_lstm_ckpt_pack_kernel)
GMX_LCK_LAUNCH(gmx_launch_lstm_ckpt_scatter, gmx_lstm_ckpt_scatter_kernel)
