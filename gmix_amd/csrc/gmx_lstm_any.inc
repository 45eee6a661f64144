// gmx_lstm_any.inc -- the shape of an LSTM bank (included by gmx_capi.cpp in front of gmx_lstm.inc): which shapes
// gmx_lstm_create_shaped accepts, the extents that follow from one, and the bank layout gmx_lstm_any.hip works on.
// DESIGN.md section 4.21.

extern "C" hipError_t gmx_launch_lstm_any_kernel(const GmxLstmAnyDev* dv, const GmxLstmRunArgs* args, int n_streams,
                                                 hipStream_t stream);

static const gmx_lstm_shape kLstmStockShape = {GMX_L_NC, GMX_L_H, 0.03f, 10.0f};

extern "C" int gmx_lstm_shape_supported(const gmx_lstm_shape* shape) {
  if (!shape) return 0;
  if (shape->num_cells < 1 || shape->num_cells > GMX_LA_MAX_CELLS) return 0;
  if (shape->horizon < 2 || shape->horizon > GMX_LA_MAX_HORIZON) return 0;
  if (!std::isfinite(shape->learning_rate) || !(shape->learning_rate > 0.0f)) return 0;
  if (!std::isfinite(shape->gradient_clip) || !(shape->gradient_clip > 0.0f)) return 0;
  return 1;
}

static bool lstm_shape_is_stock(const gmx_lstm_shape& s) {
  return s.num_cells == kLstmStockShape.num_cells && s.horizon == kLstmStockShape.horizon &&
         s.learning_rate == kLstmStockShape.learning_rate && s.gradient_clip == kLstmStockShape.gradient_clip;
}

// GMX_LSTM_BUILD=any: a stock-shape bank created while it is set gets the general layout and the general kernel (the
// other values of the variable choose among the stock kernel's builds at every launch, gmx_lstm.hip)
static bool lstm_env_forces_any() {
  const char* e = getenv("GMX_LSTM_BUILD");
  return e && strcmp(e, "any") == 0;
}

// The extents of a bank's arrays, and where element (input j, cell c) of a gate matrix lies
struct LstmDims {
  int NC, H, CP, LIN, LINP, HID, HIDP, W;
  bool any;
  uint64_t mat_floats;
  uint64_t mat(int j, int c) const { return any ? (uint64_t)j * CP + (uint64_t)c : gmx_l_mat(j, c); }
};

static LstmDims lstm_dims_of(const gmx_lstm_shape& s, bool any) {
  LstmDims d;
  d.any = any;
  d.NC = s.num_cells;
  d.H = s.horizon;
  d.LIN = GMX_L_NI + d.NC + 1;
  d.HID = d.NC + 1;
  d.W = GMX_L_NO + d.LIN;
  if (any) {
    d.CP = (d.NC + 63) / 64 * 64;
    d.LINP = (d.LIN + 63) / 64 * 64;
    d.HIDP = (d.HID + 63) / 64 * 64;
    d.mat_floats = (uint64_t)d.W * d.CP;
  } else {
    d.CP = GMX_L_CP;
    d.LINP = GMX_L_LINP;
    d.HIDP = GMX_L_CP;
    d.mat_floats = GMX_L_MAT_FLOATS;
  }
  return d;
}

static void lstm_layout_any(GmxLstmAnyDev* a, const gmx_lstm_shape& s) {
  const LstmDims k = lstm_dims_of(s, true);
  memset(a, 0, sizeof *a);
  a->nc = k.NC;
  a->h = k.H;
  a->cp = k.CP;
  a->lin = k.LIN;
  a->linp = k.LINP;
  a->hid = k.HID;
  a->hidp = k.HIDP;
  a->w = k.W;
  a->lr = s.learning_rate;
  a->clip = s.gradient_clip;
  GmxLstmDev* d = &a->o;
  uint64_t off = 0;
  auto take = [&off](uint64_t n) {
    uint64_t o = off;
    off += (n + 63) / 64 * 64;
    return o;
  };
  const uint64_t H = k.H, CP = k.CP;
  d->out_layer = take(H * k.HID * GMX_L_NO);
  for (int g = 0; g < 3; ++g) {
    GmxLstmGateOff& o = d->gate[g];
    o.weights = take(k.mat_floats);
    o.update = take(k.mat_floats);
    o.m = take(k.mat_floats);
    o.v = take(k.mat_floats);
    uint64_t* vecs[] = {&o.gamma, &o.gamma_u, &o.gamma_m, &o.gamma_v, &o.beta, &o.beta_u, &o.beta_m, &o.beta_v, &o.error};
    for (uint64_t* p : vecs) *p = take(CP);
    o.state = take(H * CP);
    o.norm = take(H * CP);
    o.ivar = take(H);
    o.transpose = take((uint64_t)k.HID * CP);
  }
  d->state = take(CP);
  d->state_error = take(CP);
  d->stored_error = take(CP);
  d->tanh_state = take(H * CP);
  d->input_gate_state = take(H * CP);
  d->last_state = take(H * CP);
  d->hidden = take(k.HIDP);
  d->hidden_error = take(CP);
  d->layer_input = take(H * k.LINP);
  d->output = take(H * GMX_L_NO);
  d->input_history = take(H);
  d->probs = take(GMX_L_NO);
  d->scal = take(16);
  d->bank_floats = off;
}
