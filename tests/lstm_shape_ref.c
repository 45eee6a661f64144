/* lstm_shape_ref.c -- the reference's LSTM byte model (LstmModel around Lstm / LstmLayer / NeuronLayer, one layer,
 * 256 inputs, 256 outputs, update_limit 3000) for ANY num_cells, horizon, learning_rate and gradient_clip, in plain C.
 * TEST INFRASTRUCTURE: what gmx_lstm_create_shaped's banks are compared with.  Pinned to the real classes by
 * tests/golden/lstm_shapes.npz (tests/test_lstm_shape_ref.py) and to oracle/gmx_oracle_lstm.c at the stock shape.
 *
 * Every float operation is written in the order the reference performs it: dot products are serial multiply-then-add
 * chains, .sum() of a valarray EXPRESSION runs from the last element down (libstdc++'s _Expr::sum) and .sum() of a
 * plain valarray from the first up; libm's tanhf / expf / logf / powf / sqrtf and rand() are the system's, as in the
 * reference.  Build with -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { NI = 256, NO = 256, UPDATE_LIMIT = 3000 };

typedef struct {
  float *error, *ivar, *gamma, *gamma_u, *gamma_m, *gamma_v, *beta, *beta_u, *beta_m, *beta_v;
  float *state /* [H][NC] */, *update, *m, *v /* [NC][W] */, *transpose /* [NC + 1][NC] */, *norm /* [H][NC] */;
  float* weights; /* [NC][W]: LongTermMemory::neuron_layer_weights[gate] */
} gate_t;

typedef struct lsr {
  int nc, h, lin, w, hid;
  float lr, clip;
  /* Lstm */
  uint32_t* input_history; /* [H] */
  float *hidden /* [HID] */, *hidden_error /* [NC] */, *layer_input /* [H][LIN] */, *output /* [H][NO] */;
  float* out_layer; /* [H][NO][HID]: LongTermMemory::lstm_output_layer */
  uint32_t epoch;
  /* LstmLayer */
  float *state, *state_error, *stored_error, *tanh_state, *input_gate_state, *last_state; /* [NC], [H][NC] */
  uint32_t l_epoch;
  uint64_t update_steps;
  gate_t gate[3]; /* forget gate, input node, output gate */
  /* LstmModel */
  int32_t top, mid, bot;
  float probs[NO];
  /* the blackboard between runs */
  uint32_t last_byte, context;
  float prediction;
  /* evidence for the tests, part of no checkpoint */
  uint64_t clipped[3]; /* elements moved by ClipGradients in state_error_, stored_error_, hidden_error_ */
  uint64_t backward_passes;
} lsr;

static float* fz(size_t n) { return (float*)calloc(n ? n : 1, sizeof(float)); }

void lsr_destroy(lsr* l) {
  if (!l) return;
  for (int g = 0; g < 3; ++g) {
    gate_t* n = &l->gate[g];
    float* all[] = {n->error, n->ivar, n->gamma, n->gamma_u, n->gamma_m, n->gamma_v, n->beta, n->beta_u, n->beta_m,
                    n->beta_v, n->state, n->update, n->m, n->v, n->transpose, n->norm, n->weights};
    for (size_t k = 0; k < sizeof all / sizeof *all; ++k) free(all[k]);
  }
  float* all[] = {l->hidden, l->hidden_error, l->layer_input, l->output, l->out_layer, l->state, l->state_error,
                  l->stored_error, l->tanh_state, l->input_gate_state, l->last_state};
  for (size_t k = 0; k < sizeof all / sizeof *all; ++k) free(all[k]);
  free(l->input_history);
  free(l);
}

/* Lstm::Lstm, LstmLayer::LstmLayer, NeuronLayer::NeuronLayer, LstmModel::LstmModel.  draw != 0: srand(seed), then the
 * initial gate weights as LstmLayer's constructor draws them (cell by cell, column by column, the three gates in
 * turn), the forget gate's bias column set to 1 afterwards. */
lsr* lsr_create(int nc, int h, float lr, float clip, unsigned seed, int draw) {
  if (nc < 1 || h < 2) return 0;
  lsr* l = (lsr*)calloc(1, sizeof *l);
  l->nc = nc;
  l->h = h;
  l->lin = NI + nc + 1;
  l->w = l->lin + NO;
  l->hid = nc + 1;
  l->lr = lr;
  l->clip = clip;
  const size_t H = (size_t)h, NC = (size_t)nc, W = (size_t)l->w;
  l->input_history = (uint32_t*)calloc(H, 4);
  l->hidden = fz(l->hid);
  l->hidden_error = fz(NC);
  l->layer_input = fz(H * l->lin);
  l->output = fz(H * NO);
  l->out_layer = fz(H * NO * l->hid);
  l->state = fz(NC);
  l->state_error = fz(NC);
  l->stored_error = fz(NC);
  l->tanh_state = fz(H * NC);
  l->input_gate_state = fz(H * NC);
  l->last_state = fz(H * NC);
  for (int g = 0; g < 3; ++g) {
    gate_t* n = &l->gate[g];
    n->error = fz(NC);
    n->ivar = fz(H);
    float** vecs[] = {&n->gamma, &n->gamma_u, &n->gamma_m, &n->gamma_v, &n->beta, &n->beta_u, &n->beta_m, &n->beta_v};
    for (int k = 0; k < 8; ++k) *vecs[k] = fz(NC);
    for (int i = 0; i < nc; ++i) n->gamma[i] = 1.0f;
    n->state = fz(H * NC);
    n->norm = fz(H * NC);
    n->update = fz(NC * W);
    n->m = fz(NC * W);
    n->v = fz(NC * W);
    n->weights = fz(NC * W);
    n->transpose = fz((NC + 1) * NC);
  }
  l->hidden[l->hid - 1] = 1;
  for (int e = 0; e < h; ++e) {
    l->layer_input[(size_t)e * l->lin + l->lin - 1] = 1;
    for (int i = 0; i < NO; ++i) l->output[(size_t)e * NO + i] = (float)(1.0 / NO);
  }
  if (draw) {
    srand(seed);
    float val = sqrtf(6.0f / (float)(NI + NO));
    float low = -val, range = 2 * val;
    for (int i = 0; i < nc; ++i) {
      for (int j = 0; j < l->w; ++j)
        for (int g = 0; g < 3; ++g) l->gate[g].weights[(size_t)i * W + j] = low + ((float)rand() / (float)RAND_MAX) * range;
      l->gate[0].weights[(size_t)i * W + W - 1] = 1;
    }
  }
  l->top = 255;
  l->mid = 127;
  l->bot = 0;
  for (int i = 0; i < NO; ++i) l->probs[i] = (float)(1.0 / 256);
  return l;
}

void lsr_weights(const lsr* l, float* w) {
  const size_t n = (size_t)l->nc * l->w;
  for (int g = 0; g < 3; ++g) memcpy(w + g * n, l->gate[g].weights, n * 4);
}
void lsr_set_weights(lsr* l, const float* w) {
  const size_t n = (size_t)l->nc * l->w;
  for (int g = 0; g < 3; ++g) memcpy(l->gate[g].weights, w + g * n, n * 4);
}
void lsr_output_layer(const lsr* l, float* o) { memcpy(o, l->out_layer, (size_t)l->h * NO * l->hid * 4); }
void lsr_clip_counts(const lsr* l, uint64_t* out) { memcpy(out, l->clipped, sizeof l->clipped); }
uint64_t lsr_backward_passes(const lsr* l) { return l->backward_passes; }
uint64_t lsr_update_steps(const lsr* l) { return l->update_steps; }

static float logistic(float x) { return 1 / (1 + expf(-x)); }

/* LstmLayer::ForwardPass(NeuronLayer&, ...) */
static void gate_forward(lsr* l, gate_t* n, const float* input, int symbol) {
  const int nc = l->nc, W = l->w;
  const uint32_t e = l->l_epoch;
  float* norm = n->norm + (size_t)e * nc;
  float* st = n->state + (size_t)e * nc;
  for (int i = 0; i < nc; ++i) {
    const float* wr = n->weights + (size_t)i * W;
    float f = wr[symbol];
    for (int j = 0; j < l->lin; ++j) f += input[j] * wr[NO + j];
    norm[i] = f;
  }
  float s = norm[nc - 1] * norm[nc - 1]; /* expression sum: from the last element down */
  for (int i = nc - 2; i >= 0; --i) s += norm[i] * norm[i];
  n->ivar[e] = 1.0f / sqrtf((s / nc) + 1e-5f);
  for (int i = 0; i < nc; ++i) norm[i] *= n->ivar[e];
  for (int i = 0; i < nc; ++i) st[i] = norm[i] * n->gamma[i] + n->beta[i];
}

/* LstmLayer::ForwardPass */
static void layer_forward(lsr* l, const float* input, int symbol) {
  const int nc = l->nc;
  const size_t at = (size_t)l->l_epoch * nc;
  memcpy(l->last_state + at, l->state, (size_t)nc * 4);
  for (int g = 0; g < 3; ++g) gate_forward(l, &l->gate[g], input, symbol);
  float *fg = l->gate[0].state + at, *in = l->gate[1].state + at, *og = l->gate[2].state + at;
  for (int i = 0; i < nc; ++i) {
    fg[i] = logistic(fg[i]);
    in[i] = tanhf(in[i]);
    og[i] = logistic(og[i]);
  }
  float *igs = l->input_gate_state + at, *ts = l->tanh_state + at;
  for (int i = 0; i < nc; ++i) igs[i] = 1.0f - fg[i];
  for (int i = 0; i < nc; ++i) l->state[i] *= fg[i];
  for (int i = 0; i < nc; ++i) l->state[i] += in[i] * igs[i];
  for (int i = 0; i < nc; ++i) ts[i] = tanhf(l->state[i]);
  for (int i = 0; i < nc; ++i) l->hidden[i] = og[i] * ts[i];
  if (++l->l_epoch == (uint32_t)l->h) l->l_epoch = 0;
}

/* Lstm::SetInput + Lstm::Predict */
static const float* lstm_predict(lsr* l, const float* ppm, uint32_t last_byte) {
  const uint32_t e = l->epoch;
  float* in = l->layer_input + (size_t)e * l->lin;
  memcpy(in, ppm, NI * 4);
  memcpy(in + NI, l->hidden, (size_t)l->nc * 4);
  layer_forward(l, in, (int)last_byte);
  float* out = l->output + (size_t)e * NO;
  const float* ol = l->out_layer + (size_t)e * NO * l->hid;
  float max_out = 0;
  for (int i = 0; i < NO; ++i) {
    float sum = 0;
    for (int j = 0; j < l->hid; ++j) sum += l->hidden[j] * ol[(size_t)i * l->hid + j];
    out[i] = sum;
    max_out = sum > max_out ? sum : max_out;
  }
  for (int i = 0; i < NO; ++i) out[i] = expf(out[i] - max_out);
  float s = out[0]; /* plain valarray sum: from the first element up */
  for (int i = 1; i < NO; ++i) s += out[i];
  for (int i = 0; i < NO; ++i) out[i] /= s;
  if (++l->epoch == (uint32_t)l->h) l->epoch = 0;
  return out;
}

static void clip(lsr* l, float* a, int which) {
  for (int i = 0; i < l->nc; ++i) {
    if (a[i] < -l->clip) {
      a[i] = -l->clip;
      ++l->clipped[which];
    } else if (a[i] > l->clip) {
      a[i] = l->clip;
      ++l->clipped[which];
    }
  }
}

/* Adam on n elements */
static void adam(const lsr* l, const float* g, float* m, float* v, float* w, int n, float t) {
  const float beta1 = 0.025, beta2 = 0.9999, eps = 1e-6f;
  const unsigned long long limit = UPDATE_LIMIT;
  float alpha, d1, d2;
  if (t < limit) alpha = l->lr * 0.1f / sqrtf(5e-5f * t + 1.0f);
  else alpha = l->lr * 0.1f / sqrtf(5e-5f * limit + 1.0f);
  for (int j = 0; j < n; ++j) m[j] *= beta1;
  for (int j = 0; j < n; ++j) m[j] += (1.0f - beta1) * g[j];
  for (int j = 0; j < n; ++j) v[j] *= beta2;
  for (int j = 0; j < n; ++j) v[j] += (1.0f - beta2) * g[j] * g[j];
  if (t < limit) {
    d1 = (float)(1.0f - powf(beta1, t));
    d2 = (float)(1.0f - powf(beta2, t));
  } else {
    d1 = (float)(1.0f - powf(beta1, limit));
    d2 = (float)(1.0f - powf(beta2, limit));
  }
  for (int j = 0; j < n; ++j) w[j] -= alpha * ((m[j] / d1) / (sqrtf(v[j] / d2 + eps)));
}

/* LstmLayer::BackwardPass(NeuronLayer&, ...), layer 0 */
static void gate_backward(lsr* l, gate_t* n, const float* input, int epoch, int symbol) {
  const int nc = l->nc, W = l->w, rec = W - NO - NI; /* nc + 1 rows of transpose_ */
  const float* norm = n->norm + (size_t)epoch * nc;
  if (epoch == l->h - 1) {
    memset(n->gamma_u, 0, (size_t)nc * 4);
    memset(n->beta_u, 0, (size_t)nc * 4);
    for (int i = 0; i < nc; ++i) {
      memset(n->update + (size_t)i * W, 0, (size_t)W * 4);
      for (int j = 0; j < rec; ++j) n->transpose[(size_t)j * nc + i] = n->weights[(size_t)i * W + j + NO + NI];
    }
  }
  for (int i = 0; i < nc; ++i) n->beta_u[i] += n->error[i];
  for (int i = 0; i < nc; ++i) n->gamma_u[i] += n->error[i] * norm[i];
  for (int i = 0; i < nc; ++i) n->error[i] *= n->gamma[i] * n->ivar[epoch];
  float s = n->error[nc - 1] * norm[nc - 1];
  for (int i = nc - 2; i >= 0; --i) s += n->error[i] * norm[i];
  s = s / nc;
  for (int i = 0; i < nc; ++i) n->error[i] -= s * norm[i];
  if (epoch > 0) {
    for (int i = 0; i < nc; ++i) {
      float f = 0;
      for (int j = 0; j < nc; ++j) f += n->error[j] * n->transpose[(size_t)i * nc + j];
      l->stored_error[i] += f;
    }
  }
  for (int i = 0; i < nc; ++i) {
    float* u = n->update + (size_t)i * W;
    for (int j = 0; j < l->lin; ++j) u[NO + j] += n->error[i] * input[j];
    u[symbol] += n->error[i];
  }
  if (epoch == 0) {
    const float t = (float)l->update_steps;
    for (int i = 0; i < nc; ++i)
      adam(l, n->update + (size_t)i * W, n->m + (size_t)i * W, n->v + (size_t)i * W, n->weights + (size_t)i * W, W, t);
    adam(l, n->gamma_u, n->gamma_m, n->gamma_v, n->gamma, nc, t);
    adam(l, n->beta_u, n->beta_m, n->beta_v, n->beta, nc, t);
  }
}

/* LstmLayer::BackwardPass */
static void layer_backward(lsr* l, const float* input, int epoch, int symbol) {
  const int nc = l->nc;
  const size_t at = (size_t)epoch * nc;
  gate_t *fg = &l->gate[0], *in = &l->gate[1], *og = &l->gate[2];
  const float *ts = l->tanh_state + at, *igs = l->input_gate_state + at, *ls = l->last_state + at;
  const float *fs = fg->state + at, *is = in->state + at, *os = og->state + at;
  if (epoch == l->h - 1) {
    memcpy(l->stored_error, l->hidden_error, (size_t)nc * 4);
    memset(l->state_error, 0, (size_t)nc * 4);
  } else {
    for (int i = 0; i < nc; ++i) l->stored_error[i] += l->hidden_error[i];
  }
  for (int i = 0; i < nc; ++i) og->error[i] = ts[i] * l->stored_error[i] * os[i] * (1.0f - os[i]);
  for (int i = 0; i < nc; ++i) l->state_error[i] += l->stored_error[i] * os[i] * (1.0f - (ts[i] * ts[i]));
  for (int i = 0; i < nc; ++i) in->error[i] = l->state_error[i] * igs[i] * (1.0f - (is[i] * is[i]));
  for (int i = 0; i < nc; ++i) fg->error[i] = (ls[i] - is[i]) * l->state_error[i] * fs[i] * igs[i];
  memset(l->hidden_error, 0, (size_t)nc * 4);
  if (epoch > 0) {
    for (int i = 0; i < nc; ++i) l->state_error[i] *= fs[i];
    memset(l->stored_error, 0, (size_t)nc * 4);
  } else if (l->update_steps < UPDATE_LIMIT) {
    ++l->update_steps;
  }
  gate_backward(l, fg, input, epoch, symbol);
  gate_backward(l, in, input, epoch, symbol);
  gate_backward(l, og, input, epoch, symbol);
  clip(l, l->state_error, 0);
  clip(l, l->stored_error, 1);
  clip(l, l->hidden_error, 2);
}

/* Lstm::Perceive */
static void lstm_perceive(lsr* l, uint32_t input) {
  const int h = l->h, hid = l->hid;
  int last_epoch = (int)l->epoch - 1;
  if (last_epoch == -1) last_epoch = h - 1;
  const uint32_t old_input = l->input_history[last_epoch];
  l->input_history[last_epoch] = input;
  if (l->epoch == 0) {
    ++l->backward_passes;
    for (int epoch = h - 1; epoch >= 0; --epoch) {
      const float* out = l->output + (size_t)epoch * NO;
      const float* ol = l->out_layer + (size_t)epoch * NO * hid;
      for (uint32_t i = 0; i < NO; ++i) {
        float error = (i == l->input_history[epoch]) ? (out[i] - 1) : out[i];
        for (int j = 0; j < l->nc; ++j) l->hidden_error[j] += ol[(size_t)i * hid + j] * error;
      }
      int prev_epoch = epoch - 1;
      if (prev_epoch == -1) prev_epoch = h - 1;
      uint32_t symbol = l->input_history[prev_epoch];
      if (epoch == 0) symbol = old_input;
      layer_backward(l, l->layer_input + (size_t)epoch * l->lin, epoch, (int)symbol);
    }
  }
  const float* out = l->output + (size_t)last_epoch * NO;
  const float* src = l->out_layer + (size_t)last_epoch * NO * hid;
  float* dst = l->out_layer + (size_t)l->epoch * NO * hid;
  for (uint32_t i = 0; i < NO; ++i) {
    float error = (i == input) ? (out[i] - 1) : out[i];
    float le = l->lr * error;
    for (int j = 0; j < hid; ++j) dst[(size_t)i * hid + j] = src[(size_t)i * hid + j];
    for (int j = 0; j < hid; ++j) dst[(size_t)i * hid + j] -= le * l->hidden[j];
  }
}

/* Sigmoid::Logit */
static float logit(float p) {
  if (p < 0.0001) p = 0.0001;
  else if (p > 0.9999) p = 0.9999;
  return logf(p / (1 - p));
}

/* LstmModel::Predict for one bit; returns 1 when SetPrediction marks the model active */
static int model_predict(lsr* l, int recent_bits, int new_bit, const float* ppm) {
  if (recent_bits == 1) {
    memcpy(l->probs, lstm_predict(l, ppm, l->last_byte), sizeof l->probs);
    l->top = 255;
    l->bot = 0;
    float max_pred = 0;
    l->context = 0;
    for (int i = 0; i < 256; ++i)
      if (l->probs[i] > max_pred) {
        max_pred = l->probs[i];
        l->context = (uint32_t)i;
      }
  } else {
    if (new_bit) l->bot = l->mid + 1;
    else l->top = l->mid;
  }
  l->mid = l->bot + ((l->top - l->bot) / 2);
  float num = 0.0f;
  for (int i = l->mid + 1; i <= l->top; ++i) num += l->probs[i];
  float denom = num;
  for (int i = l->bot; i <= l->mid; ++i) denom += l->probs[i];
  if (denom != 0) {
    float p = num / denom;
    l->prediction = logit(p);
    return p == 0.5 ? 0 : 1;
  }
  return 0;
}

/* n whole bytes: per byte the distribution (probs_out nullable), per bit the prediction and the active flag, per byte
 * lstm_prediction_context; learn == 0 leaves LstmModel::Learn out (generation). */
void lsr_run(lsr* l, uint64_t n_bytes, const float* ppm, const uint8_t* bytes, int learn, float* probs_out, float* pred_out,
             uint8_t* act_out, uint32_t* ctx_out) {
  for (uint64_t n = 0; n < n_bytes; ++n) {
    int recent_bits = 1, new_bit = 0;
    for (int k = 0; k < 8; ++k) {
      const int act = model_predict(l, recent_bits, new_bit, ppm + n * 256);
      if (k == 0) {
        if (probs_out) memcpy(probs_out + n * 256, l->probs, sizeof l->probs);
        if (ctx_out) ctx_out[n] = l->context;
      }
      if (pred_out) pred_out[n * 8 + k] = l->prediction;
      if (act_out) act_out[n * 8 + k] = (uint8_t)act;
      new_bit = (bytes[n] >> (7 - k)) & 1;
      const int current = recent_bits * 2 + new_bit;
      if (learn && current >= 256) lstm_perceive(l, (uint32_t)(current - 256)); /* LstmModel::Learn */
      recent_bits = current;
    }
    l->last_byte = bytes[n];
  }
}

/* Lstm::Predict at a byte boundary with LstmModel::Predict's bookkeeping, and Lstm::Perceive: the per-byte surface */
void lsr_predict_byte(lsr* l, const float* ppm, uint32_t last_byte, float* probs_out, uint32_t* ctx_out) {
  l->last_byte = last_byte;
  model_predict(l, 1, 0, ppm);
  if (probs_out) memcpy(probs_out, l->probs, sizeof l->probs);
  if (ctx_out) *ctx_out = l->context;
}
void lsr_perceive_byte(lsr* l, uint32_t byte) { lstm_perceive(l, byte); }

/* ---- persistence: raw arrays in declaration order, no headers ------------------------------------------------
 * `.short`: LstmModel::WriteToDisk -> Lstm::WriteToDisk -> LstmLayer::WriteToDisk -> three NeuronLayer::WriteToDisk;
 * `.long`: the LSTM section of LongTermMemory::WriteToDisk (lstm_output_layer, then the three NeuronLayerWeights). */
typedef struct {
  uint8_t* buf;
  size_t off;
} out_t;
static void put(out_t* o, const void* p, size_t n) {
  if (o->buf) memcpy(o->buf + o->off, p, n);
  o->off += n;
}

size_t lsr_export_short(const lsr* l, uint8_t* buf) {
  out_t o = {buf, 0};
  const size_t NC = (size_t)l->nc, H = (size_t)l->h, W = (size_t)l->w;
  put(&o, &l->top, 4);
  put(&o, &l->mid, 4);
  put(&o, &l->bot, 4);
  put(&o, l->probs, sizeof l->probs);
  put(&o, l->input_history, H * 4);
  put(&o, l->hidden, (size_t)l->hid * 4);
  put(&o, l->hidden_error, NC * 4);
  put(&o, l->layer_input, H * l->lin * 4);
  put(&o, l->output, H * NO * 4);
  put(&o, &l->epoch, 4);
  put(&o, l->state, NC * 4);
  put(&o, l->state_error, NC * 4);
  put(&o, l->stored_error, NC * 4);
  put(&o, l->tanh_state, H * NC * 4);
  put(&o, l->input_gate_state, H * NC * 4);
  put(&o, l->last_state, H * NC * 4);
  put(&o, &l->l_epoch, 4);
  put(&o, &l->update_steps, 8);
  for (int g = 0; g < 3; ++g) {
    const gate_t* n = &l->gate[g];
    put(&o, n->error, NC * 4);
    put(&o, n->ivar, H * 4);
    const float* vecs[] = {n->gamma, n->gamma_u, n->gamma_m, n->gamma_v, n->beta, n->beta_u, n->beta_m, n->beta_v};
    for (int k = 0; k < 8; ++k) put(&o, vecs[k], NC * 4);
    put(&o, n->state, H * NC * 4);
    put(&o, n->update, NC * W * 4);
    put(&o, n->m, NC * W * 4);
    put(&o, n->v, NC * W * 4);
    put(&o, n->transpose, (NC + 1) * NC * 4);
    put(&o, n->norm, H * NC * 4);
  }
  return o.off;
}

size_t lsr_export_long(const lsr* l, uint8_t* buf) {
  out_t o = {buf, 0};
  put(&o, l->out_layer, (size_t)l->h * NO * l->hid * 4);
  for (int g = 0; g < 3; ++g) put(&o, l->gate[g].weights, (size_t)l->nc * l->w * 4);
  return o.off;
}

/* LstmModel::GetMemoryUsage with Lstm::, LstmLayer:: and NeuronLayer::GetMemoryUsage behind it, and the LSTM's share
 * of LongTermMemory::GetMemoryUsage as gmx_lstm_memory_usage counts it for the stock shape */
uint64_t lsr_memory_usage(const lsr* l) {
  const uint64_t H = l->h, NC = l->nc, W = l->w, HID = l->hid, LIN = l->lin;
  const uint64_t neuron = 4 + 40 * NC + 4 * H * NC + 3 * (4 * NC * W) + 4 * (W - NO - NI) * NC + 4 * H * NC;
  const uint64_t layer = 44 + 3 * (4 * NC) + 3 * (4 * H * NC) + 3 * neuron;
  const uint64_t lstm = 24 + 4 * H + 4 * HID + 4 * NC + 4 * H * LIN + 4 * H * NO + layer;
  return 16 + 256 * 4 + 4 * H * NO * HID + 3 * (4 * NC * W) + lstm;
}
