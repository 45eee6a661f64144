// gmx_lstm_any.hip -- the reference's LSTM byte model (models/lstm-model.cpp, lstm.cpp, lstm-layer.cpp; one layer, 256
// inputs, 256 outputs) for ANY num_cells (1..256), horizon (2..256), learning_rate and gradient_clip, the shape read
// from the bank's descriptor at run time: one 256-thread workgroup per stream, bytes in sequence.  The stock shape
// keeps gmx_lstm.hip, whose extents are compile-time constants; this kernel is what a maintainer's own Lstm(...) line
// gets (gmx_lstm_create_shaped), and what GMX_LSTM_BUILD=any puts the stock shape through for the tests.
//
// Every float operation of the reference is performed once, in the reference's order (see gmx_lstm.hip's header and
// oracle/gmx_oracle_lstm.c): serial multiply-then-add chains for the dot products, expression sums from the last
// element down, plain valarray sums from the first up, gmx_math.h's tanhf / expf / logf, nothing fused.  Parallelism
// comes only from what the reference leaves independent, and because 3 x num_cells may exceed the 256 threads every
// such set is a loop of items over the threads:
//   * gate chains: item = gate * cp + cell (cp = num_cells rounded up to 64), so a wave holds 64 neighbouring cells of
//     ONE gate and each of the 257 + num_cells steps reads a coalesced row of the input-major matrix;
//   * the 256 output chains (num_cells + 1 steps) and the output layer's SGD step: thread = symbol;
//   * the num_cells hidden-error chains (256 steps): thread = cell, 16-byte loads along its own row;
//   * per gate the num_cells transposed products (item = gate * cp + cell, along a row of transpose_);
//   * the (257 + num_cells) x num_cells accumulators of each gate, kept in HBM as the reference keeps update_ -- an
//     epoch adds its product to each, element = thread + 256 k -- with Adam applied by the same thread in the last
//     epoch; the 256 symbol rows, of which an epoch touches one, likewise;
//   * the 8 bit predictions of a byte, one lane each.
// The ordered reductions (layer norm's two sums, softmax's sum) are one thread's, over LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gmx_lstm_any.h"
#include "gmx_math.h"

namespace {

constexpr int NI = GMX_L_NI, NO = GMX_L_NO;
constexpr int kMaxNC = GMX_LA_MAX_CELLS;
constexpr int kMaxLinP = 576;  // 256 + 256 + 1 rounded up to 64
constexpr int kMaxHidP = 320;  // 256 + 1 rounded up to 64
constexpr uint32_t kUpdateLimit = GMX_LA_UPDATE_LIMIT;

struct LdsAny {
  alignas(16) float probs[NO];      // LstmModel::probs_ / softmax scratch
  alignas(16) float err[NO];        // output-layer error of an epoch
  alignas(16) float xin[kMaxLinP];  // layer input of the epoch at hand
  alignas(16) float hid[kMaxHidP];  // Lstm::hidden_ (hid[num_cells] = 1)
  float herr[kMaxNC];               // Lstm::hidden_error_
  float nrm[3][kMaxNC];             // per gate: pre-norm sums / products for the ordered reductions
  float act[3][kMaxNC];             // per gate: activated state forward / error backward
  float fsum[3][kMaxNC];            // per gate: the transposed products of an epoch
  float red[8];
  uint32_t ired[4];
  uint64_t exptab[32];
};

// acc + p[0] + ... + p[n-1] strictly in that order, n a multiple of 4 up to 4*Q4, p 16-byte aligned in LDS
template <int Q4>
__device__ __forceinline__ float any_ordered_sum4(float acc, const float* p, int n) {
  float4 v[Q4];
#pragma unroll
  for (int q = 0; q < Q4; ++q) v[q] = *(const float4*)(p + 4 * (4 * q < n ? q : 0));
#pragma unroll
  for (int q = 0; q < Q4; ++q)
    if (4 * q < n) {
      acc += v[q].x;
      acc += v[q].y;
      acc += v[q].z;
      acc += v[q].w;
    }
  return acc;
}

}  // namespace

__global__ void __launch_bounds__(256)
gmx_lstm_any_kernel(const GmxLstmAnyDev* __restrict__ dvp, const GmxLstmRunArgs a) {
  __shared__ LdsAny L;
  const GmxLstmAnyDev& dv = *dvp;
  const GmxLstmDev& o = dv.o;
  const int NC = dv.nc, H = dv.h, CP = dv.cp, LIN = dv.lin, LINP = dv.linp, HID = dv.hid;
  const int items = 3 * CP;  // (gate, cell) pairs, the padding cells of a gate idle
  const float lr = dv.lr, clipv = dv.clip;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int s = blockIdx.x;
  const uint64_t NB = a.n_list ? a.n_list[s] : a.n_bytes;
  if (NB == 0) return;
  float* const B = a.banks + (uint64_t)(a.stream_base + s) * o.bank_floats;
  uint32_t* const scal = (uint32_t*)(B + o.scal);
  uint32_t* const hist = (uint32_t*)(B + o.input_history);
  float* const out_layer = B + o.out_layer;
  const float* const ppm_s = a.ppm + (uint64_t)s * a.rec_stride * NI;
  const uint8_t* const bytes_s = a.bytes + (uint64_t)s * a.rec_stride;
  const float* const adam_s = a.adam + (uint64_t)s * a.max_bptt * 4;
  float* const pred_s = a.pred_out + (uint64_t)s * a.rec_stride * 8;
  uint8_t* const act_s = a.act_out + (uint64_t)s * a.rec_stride * 8;
  uint32_t* const ctx_s = a.ctx_out + (uint64_t)s * a.rec_stride;

  if (tid < 32) L.exptab[tid] = gmx_exp2f_tab[tid];
  for (int i = tid; i < HID; i += 256) L.hid[i] = (B + o.hidden)[i];
  if (tid < NC) L.herr[tid] = (B + o.hidden_error)[tid];
  L.probs[tid] = (B + o.probs)[tid];
  uint32_t epoch = scal[0], l_epoch = scal[1], update_steps = scal[2], last_byte = scal[3], context = scal[4];
  uint32_t coded = scal[6];
  float prediction = __uint_as_float(scal[5]);
  if (a.last_byte >= 0) last_byte = (uint32_t)a.last_byte;
  uint32_t bptt_done = 0;
  const uint32_t phases = a.phases;
  const bool learn = a.learn != 0;
  __syncthreads();

  auto clipf = [&](float v) { return v < -clipv ? -clipv : (v > clipv ? clipv : v); };
  // The 8 bit predictions of a byte (lstm-model.cpp:34-48) by the first 8 lanes of wave 0: lane k sums the two halves
  // of bit k's range of L.probs in order, lane 0 then walks the bits (a silent bit keeps the previous prediction).
  auto bit_predictions = [&](uint32_t byte_b, uint64_t n_b, uint32_t context_b) {
    float logit = 0.0f, state = 0.0f;
    if (lane < 8) {
      const int k = lane;
      const int size = 256 >> k, half = size >> 1;
      const int bot = k == 0 ? 0 : (int)((byte_b >> (8 - k)) << (8 - k));
      const int mid = bot + half - 1, top = bot + size - 1;
      float num = 0.0f, denom;  // std::accumulate from 0.0f over the upper half, then on over the lower half
      if (half >= 4) {
#pragma unroll 1
        for (int q = 0; q < half; q += 64) num = any_ordered_sum4<16>(num, L.probs + mid + 1 + q, half - q < 64 ? half - q : 64);
        denom = num;
#pragma unroll 1
        for (int q = 0; q < half; q += 64) denom = any_ordered_sum4<16>(denom, L.probs + bot + q, half - q < 64 ? half - q : 64);
      } else {
        for (int i = mid + 1; i <= top; ++i) num += L.probs[i];
        denom = num;
        for (int i = bot; i <= mid; ++i) denom += L.probs[i];
      }
      const float p = num / denom;
      logit = gmx_logit(p);
      state = denom != 0.0f ? (p == 0.5f ? 1.0f : 2.0f) : 0.0f;  // 0 silent, 1 inactive, 2 active
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float st = __shfl(state, k), lg = __shfl(logit, k);
      if (lane == 0) {
        if (st != 0.0f) prediction = lg;
        pred_s[n_b * 8 + k] = prediction;
        act_s[n_b * 8 + k] = st == 2.0f ? 1 : 0;
      }
    }
    if (lane == 0) ctx_s[n_b] = context_b;
  };

  for (uint64_t n = 0; n < NB; ++n) {
    const uint32_t byte = bytes_s[n];
    // ======================= Lstm::SetInput + Lstm::Predict (lstm.cpp:45-50, :95-123) =======================
    if (phases & 1u) {
      const uint32_t e = epoch, le = l_epoch;
      L.xin[tid] = ppm_s[n * NI + tid];
      if (tid < NC) {
        L.xin[NI + tid] = L.hid[tid];
        (B + o.last_state + (uint64_t)le * CP)[tid] = (B + o.state)[tid];  // lstm-layer.cpp:200
      }
      if (tid == 0) L.xin[LIN - 1] = 1.0f;
      __syncthreads();
      for (int j = tid; j < LIN; j += 256) (B + o.layer_input + (uint64_t)e * LINP)[j] = L.xin[j];
      // LstmLayer::ForwardPass(NeuronLayer&) (lstm-layer.cpp:221-241): the 3 x num_cells chains
      for (int it = tid; it < items; it += 256) {
        const int g = it / CP, c = it - g * CP;
        if (c < NC) {
          const float* w = B + o.gate[g].weights;
          float f = w[(uint64_t)last_byte * CP + c];
          const float* wl = w + (uint64_t)NO * CP + c;
#pragma unroll 8
          for (int j = 0; j < LIN; ++j) f += L.xin[j] * wl[(uint64_t)j * CP];
          L.nrm[g][c] = f;
        }
      }
      __syncthreads();
      if (tid < 3) {
        const float* nr = L.nrm[tid];
        float sq = nr[NC - 1] * nr[NC - 1];  // expression .sum(): last element first
        for (int i = NC - 2; i >= 0; --i) sq += nr[i] * nr[i];
        const float iv = gmx_lstm_norm_scale(sq, (float)NC);
        L.red[tid] = iv;
        (B + o.gate[tid].ivar)[le] = iv;
      }
      __syncthreads();
      for (int it = tid; it < items; it += 256) {
        const int g = it / CP, c = it - g * CP;
        if (c < NC) {
          const GmxLstmGateOff& go = o.gate[g];
          const float nv = L.nrm[g][c] * L.red[g];
          (B + go.norm + (uint64_t)le * CP)[c] = nv;
          float st = nv * (B + go.gamma)[c] + (B + go.beta)[c];
          st = g == 1 ? gmx_tanhf(st) : gmx_logistic_tab(st, L.exptab);  // lstm-layer.cpp:205-211
          (B + go.state + (uint64_t)le * CP)[c] = st;
          L.act[g][c] = st;
        }
      }
      __syncthreads();
      if (tid < NC) {  // lstm-layer.cpp:212-217
        const float f = L.act[0][tid];
        const float igs = 1.0f - f;
        float st = (B + o.state)[tid] * f;
        st = st + L.act[1][tid] * igs;
        const float ts = gmx_tanhf(st);
        (B + o.input_gate_state + (uint64_t)le * CP)[tid] = igs;
        (B + o.state)[tid] = st;
        (B + o.tanh_state + (uint64_t)le * CP)[tid] = ts;
        L.hid[tid] = L.act[2][tid] * ts;
      }
      __syncthreads();
      // output layer + softmax (lstm.cpp:106-118): thread = output symbol
      const float* ol = out_layer + (uint64_t)e * HID * NO;
      float sum = 0.0f;
#pragma unroll 8
      for (int j = 0; j < HID; ++j) sum += L.hid[j] * ol[(uint64_t)j * NO + tid];
      float mx = sum > 0.0f ? sum : 0.0f;  // max_out = max(0, every sum): order does not matter for a maximum
      for (int q = 32; q > 0; q >>= 1) {
        const float other = __shfl_xor(mx, q);
        mx = other > mx ? other : mx;
      }
      if (lane == 0) L.red[4 + wave] = mx;
      __syncthreads();
      mx = L.red[4];
      for (int k = 1; k < 4; ++k) mx = L.red[4 + k] > mx ? L.red[4 + k] : mx;
      L.probs[tid] = gmx_expf_tab(sum - mx, L.exptab);
      __syncthreads();
      if (tid == 0) {  // valarray::sum(): first element first (0 + p[0] is p[0])
        float t = 0.0f;
#pragma unroll 1
        for (int q = 0; q < NO; q += 64) t = any_ordered_sum4<16>(t, L.probs + q, 64);
        L.red[0] = t;
      }
      __syncthreads();
      const float p = L.probs[tid] / L.red[0];
      __syncthreads();
      L.probs[tid] = p;
      (B + o.output + (uint64_t)e * NO)[tid] = p;
      epoch = epoch + 1 == (uint32_t)H ? 0 : epoch + 1;
      l_epoch = l_epoch + 1 == (uint32_t)H ? 0 : l_epoch + 1;
      // lstm_prediction_context: the first symbol with the largest probability (lstm-model.cpp:25-33)
      float pm = p;
      for (int q = 32; q > 0; q >>= 1) {
        const float other = __shfl_xor(pm, q);
        pm = other > pm ? other : pm;
      }
      if (lane == 0) L.red[4 + wave] = pm;
      if (tid == 0) L.ired[0] = 0xffffffffu;
      __syncthreads();
      pm = L.red[4];
      for (int k = 1; k < 4; ++k) pm = L.red[4 + k] > pm ? L.red[4 + k] : pm;
      if (p == pm) atomicMin(&L.ired[0], (uint32_t)tid);
      __syncthreads();
      context = pm > 0.0f ? L.ired[0] : 0u;
    }
    // ======================= the 8 bit predictions (lstm-model.cpp:34-48) ====================================
    if ((phases & 2u) && wave == 0) bit_predictions(byte, n, context);
    __syncthreads();
    if (phases & 6u) {  // the byte is known from here on
      last_byte = byte;
      coded = 1;
    }
    if (!learn || !(phases & 4u)) continue;
    // ======================= Lstm::Perceive (lstm.cpp:52-93) =================================================
    const uint32_t last_epoch = epoch == 0 ? (uint32_t)H - 1 : epoch - 1;
    const uint32_t old_input = hist[last_epoch];
    __syncthreads();
    if (tid == 0) hist[last_epoch] = byte;
    __syncthreads();
    if (epoch == 0) {
      const float alpha = adam_s[bptt_done * 4 + 0], d1 = adam_s[bptt_done * 4 + 1], d2 = adam_s[bptt_done * 4 + 2];
      const float beta1 = 0.025f, beta2 = 0.9999f;
      // Adam (lstm-layer.cpp:12-35) of one element whose gradient is gr
      auto adam1 = [&](float gr, float* mp, float* vp, float* wp) {
        float m = *mp * beta1;
        m += (1.0f - beta1) * gr;
        float v = *vp * beta2;
        v += (1.0f - beta2) * gr * gr;
        *mp = m;
        *vp = v;
        *wp = gmx_lstm_adam_step(*wp, alpha, m, d1, v, d2);
      };
      for (int ep = H - 1; ep >= 0; --ep) {
        const bool first = ep == H - 1;
        // output-layer error of this epoch and its pull on the hidden state (lstm.cpp:61-69)
        {
          const float ov = (B + o.output + (uint64_t)ep * NO)[tid];
          L.err[tid] = ((uint32_t)tid == hist[ep]) ? (ov - 1.0f) : ov;
          for (int j = tid; j < LIN; j += 256) L.xin[j] = (B + o.layer_input + (uint64_t)ep * LINP)[j];
        }
        __syncthreads();
        if (tid < NC) {  // hidden_error_[j] += lstm_output_layer[ep][i][j] * error[i], i = 0..255 in order
          const float4* row = (const float4*)(out_layer + ((uint64_t)ep * HID + tid) * NO);
          float he = L.herr[tid];
#pragma unroll 8
          for (int q = 0; q < NO / 4; ++q) {
            const float4 v = row[q];
            const float4 ev = *(const float4*)(L.err + 4 * q);
            he += v.x * ev.x;
            he += v.y * ev.y;
            he += v.z * ev.z;
            he += v.w * ev.w;
          }
          L.herr[tid] = he;
        }
        __syncthreads();
        const uint32_t prev_epoch = ep == 0 ? (uint32_t)H - 1 : (uint32_t)ep - 1;
        const uint32_t symbol = ep == 0 ? old_input : hist[prev_epoch];
        // LstmLayer::BackwardPass (lstm-layer.cpp:252-292)
        if (tid < NC) {
          const int i = tid;
          float stored = (B + o.stored_error)[i], serr = (B + o.state_error)[i];
          if (first) {
            stored = L.herr[i];
            serr = 0.0f;
          } else {
            stored += L.herr[i];
          }
          const float ts = (B + o.tanh_state + (uint64_t)ep * CP)[i];
          const float og = (B + o.gate[2].state + (uint64_t)ep * CP)[i];
          const float in = (B + o.gate[1].state + (uint64_t)ep * CP)[i];
          const float fg = (B + o.gate[0].state + (uint64_t)ep * CP)[i];
          const float igs = (B + o.input_gate_state + (uint64_t)ep * CP)[i];
          const float ls = (B + o.last_state + (uint64_t)ep * CP)[i];
          L.act[2][i] = ts * stored * og * (1.0f - og);
          serr += stored * og * (1.0f - (ts * ts));
          L.act[1][i] = serr * igs * (1.0f - (in * in));
          L.act[0][i] = (ls - in) * serr * fg * igs;
          L.herr[i] = 0.0f;
          if (ep > 0) {
            serr *= fg;
            stored = 0.0f;
          }
          (B + o.stored_error)[i] = stored;
          (B + o.state_error)[i] = serr;
        }
        if (ep == 0 && update_steps < kUpdateLimit) ++update_steps;
        __syncthreads();
        // LstmLayer::BackwardPass(NeuronLayer&) (lstm-layer.cpp:294-355) of the three gates side by side
        for (int it = tid; it < items; it += 256) {
          const int g = it / CP, c = it - g * CP;
          if (c < NC) {
            const GmxLstmGateOff& go = o.gate[g];
            if (first) {  // transpose_ (lstm-layer.cpp:300-304): the recurrent weights and the bias column
              for (int j = 0; j < HID; ++j)
                (B + go.transpose)[(uint64_t)j * CP + c] = (B + go.weights)[(uint64_t)(NO + NI + j) * CP + c];
            }
            float err = L.act[g][c];
            const float nv = (B + go.norm + (uint64_t)ep * CP)[c];
            const float bu = first ? 0.0f : (B + go.beta_u)[c];
            const float gu = first ? 0.0f : (B + go.gamma_u)[c];
            (B + go.beta_u)[c] = bu + err;
            (B + go.gamma_u)[c] = gu + err * nv;
            err *= (B + go.gamma)[c] * (B + go.ivar)[ep];
            L.act[g][c] = err;
            L.nrm[g][c] = err * nv;
          }
        }
        if (first) {  // update_ = 0: the symbol rows here, the layer-input rows where their first product lands
          for (int g = 0; g < 3; ++g) {
            float* up = B + o.gate[g].update;
            for (int ix = tid; ix < NO * CP; ix += 256) up[ix] = 0.0f;
          }
        }
        __syncthreads();
        if (tid < 3) {
          const float* nr = L.nrm[tid];
          float t = nr[NC - 1];  // expression .sum(): last element first
          for (int i = NC - 2; i >= 0; --i) t += nr[i];
          L.red[tid] = t / (float)NC;
        }
        __syncthreads();
        for (int it = tid; it < items; it += 256) {
          const int g = it / CP, c = it - g * CP;
          if (c < NC) {
            const GmxLstmGateOff& go = o.gate[g];
            const float nv = (B + go.norm + (uint64_t)ep * CP)[c];
            const float err = L.act[g][c] - L.red[g] * nv;
            L.act[g][c] = err;
            (B + go.error)[c] = err;
            (B + go.update)[(uint64_t)symbol * CP + c] += err;  // lstm-layer.cpp:342
          }
        }
        __syncthreads();
        if (ep > 0) {  // through transpose_, the recurrent weights as the pass found them (lstm-layer.cpp:330-338)
          for (int it = tid; it < items; it += 256) {
            const int g = it / CP, c = it - g * CP;
            if (c < NC) {
              const float* tr = B + o.gate[g].transpose + (uint64_t)c * CP;
              float f = 0.0f;
#pragma unroll 8
              for (int j = 0; j < NC; ++j) f += L.act[g][j] * tr[j];
              L.fsum[g][c] = f;
            }
          }
        }
        // update_[cell][256 + j] += error[cell] * input[j] (lstm-layer.cpp:341); in the last epoch Adam right behind it
        const int n_acc = LIN * CP;
        for (int g = 0; g < 3; ++g) {
          const GmxLstmGateOff& go = o.gate[g];
          float* up = B + go.update + (uint64_t)NO * CP;
          for (int ix = tid; ix < n_acc; ix += 256) {
            const int j = ix / CP, c = ix - j * CP;
            if (c < NC) {
              const float old = first ? 0.0f : up[ix];
              const float acc = old + L.act[g][c] * L.xin[j];
              up[ix] = acc;
              if (ep == 0) {
                const uint64_t at = (uint64_t)NO * CP + ix;
                adam1(acc, B + go.m + at, B + go.v + at, B + go.weights + at);
              }
            }
          }
          if (ep == 0) {  // the symbol rows and the layer-norm parameters
            for (int ix = tid; ix < NO * CP; ix += 256) {
              const int c = ix % CP;
              if (c < NC) adam1((B + go.update)[ix], B + go.m + ix, B + go.v + ix, B + go.weights + ix);
            }
            for (int c = tid; c < NC; c += 256) {
              adam1((B + go.gamma_u)[c], B + go.gamma_m + c, B + go.gamma_v + c, B + go.gamma + c);
              adam1((B + go.beta_u)[c], B + go.beta_m + c, B + go.beta_v + c, B + go.beta + c);
            }
          }
        }
        __syncthreads();
        if (tid < NC) {  // the three gates add to stored_error_ in their order, then the clips
          float stored = (B + o.stored_error)[tid];
          if (ep > 0) {
            stored += L.fsum[0][tid];
            stored += L.fsum[1][tid];
            stored += L.fsum[2][tid];
          }
          (B + o.stored_error)[tid] = clipf(stored);
          (B + o.state_error)[tid] = clipf((B + o.state_error)[tid]);
          L.herr[tid] = clipf(L.herr[tid]);
        }
        __syncthreads();
      }
      ++bptt_done;
    }
    // the output layer's own step (lstm.cpp:81-88)
    {
      const float ov = (B + o.output + (uint64_t)last_epoch * NO)[tid];
      const float error = ((uint32_t)tid == byte) ? (ov - 1.0f) : ov;
      const float le = lr * error;
      const float* src = out_layer + (uint64_t)last_epoch * HID * NO;
      float* dst = out_layer + (uint64_t)epoch * HID * NO;
#pragma unroll 8
      for (int j = 0; j < HID; ++j) dst[(uint64_t)j * NO + tid] = src[(uint64_t)j * NO + tid] - le * L.hid[j];
    }
    __syncthreads();
  }
  // state back to the bank
  for (int i = tid; i < HID; i += 256) (B + o.hidden)[i] = L.hid[i];
  if (tid < NC) (B + o.hidden_error)[tid] = L.herr[tid];
  (B + o.probs)[tid] = L.probs[tid];
  if (tid == 0) {
    scal[0] = epoch;
    scal[1] = l_epoch;
    scal[2] = update_steps;
    scal[3] = last_byte;
    scal[4] = context;
    scal[5] = __float_as_uint(prediction);
    scal[6] = coded;
  }
}

extern "C" hipError_t gmx_launch_lstm_any_kernel(const GmxLstmAnyDev* dv, const GmxLstmRunArgs* args, int n_streams,
                                                 hipStream_t stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(gmx_lstm_any_kernel, dim3(n_streams), dim3(256), 0, stream, dv, *args);
  return hipGetLastError();
}
