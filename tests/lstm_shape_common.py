"""Shared by the tests of the shaped LSTM banks: tests/lstm_shape_ref.c -- the reference's LSTM byte model for any
num_cells / horizon / learning_rate / gradient_clip in plain C -- through ctypes, the fixtures recorded from the real
classes (tests/golden/lstm_shapes.npz, made by tests/golden/make_lstm_shape_golden.py), and the synthetic inputs."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lstm_shapes.npz")
STOCK = (50, 100, 0.03, 10.0)

_cache = {}


def ref_lib():
    """tests/lstm_shape_ref.c, built like ctx_common.py builds ctx_ref.c (-ffp-contract=off: separate roundings)."""
    if "lib" in _cache:
        return _cache["lib"]
    src = os.path.join(HERE, "lstm_shape_ref.c")
    out = os.path.join(HERE, "lstm_shape_ref.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out, "-lm"])
    L = C.CDLL(out)
    vp, u64, i32, u32, f32 = C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_float
    L.lsr_create.restype = vp
    L.lsr_create.argtypes = [i32, i32, f32, f32, C.c_uint, i32]
    L.lsr_destroy.argtypes = [vp]
    L.lsr_destroy.restype = None
    for f in (L.lsr_weights, L.lsr_set_weights, L.lsr_output_layer, L.lsr_clip_counts):
        f.argtypes = [vp, vp]
        f.restype = None
    for f in (L.lsr_backward_passes, L.lsr_update_steps, L.lsr_memory_usage):
        f.argtypes = [vp]
        f.restype = u64
    L.lsr_run.argtypes = [vp, u64, vp, vp, i32, vp, vp, vp, vp]
    L.lsr_run.restype = None
    L.lsr_predict_byte.argtypes = [vp, vp, u32, vp, C.POINTER(u32)]
    L.lsr_predict_byte.restype = None
    L.lsr_perceive_byte.argtypes = [vp, u32]
    L.lsr_perceive_byte.restype = None
    for f in (L.lsr_export_short, L.lsr_export_long):
        f.argtypes = [vp, vp]
        f.restype = C.c_size_t
    _cache["lib"] = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Ref:
    """One stream of the byte model at a shape (cells, horizon, learning_rate, gradient_clip).  seed: srand(seed) and
    the reference's draw of the initial gate weights; None: all-zero gate weights (set_weights follows)."""

    def __init__(self, shape, seed=None):
        self.L = ref_lib()
        self.nc, self.h = int(shape[0]), int(shape[1])
        self.lr, self.clip = float(shape[2]), float(shape[3])
        self.w, self.hid = 513 + self.nc, self.nc + 1
        self.p = self.L.lsr_create(self.nc, self.h, self.lr, self.clip, 0 if seed is None else int(seed),
                                   0 if seed is None else 1)
        assert self.p

    def __del__(self):
        if getattr(self, "p", None):
            self.L.lsr_destroy(self.p)
            self.p = None

    def weights(self):
        w = np.zeros((3, self.nc, self.w), np.float32)
        self.L.lsr_weights(self.p, _p(w))
        return w

    def set_weights(self, w):
        w = np.ascontiguousarray(w, np.float32)
        assert w.shape == (3, self.nc, self.w)
        self.L.lsr_set_weights(self.p, _p(w))

    def output_layer(self):
        o = np.zeros((self.h, 256, self.hid), np.float32)
        self.L.lsr_output_layer(self.p, _p(o))
        return o

    def run(self, ppm, data, learn=True):
        """{probs [n,256], pred [n,8], act [n,8], ctx [n]} of n whole bytes."""
        ppm = np.ascontiguousarray(ppm, np.float32)
        data = np.ascontiguousarray(data, np.uint8)
        n = len(data)
        assert ppm.shape == (n, 256)
        out = dict(probs=np.zeros((n, 256), np.float32), pred=np.zeros((n, 8), np.float32),
                   act=np.zeros((n, 8), np.uint8), ctx=np.zeros(n, np.uint32))
        self.L.lsr_run(self.p, n, _p(ppm), _p(data), 1 if learn else 0, _p(out["probs"]), _p(out["pred"]),
                       _p(out["act"]), _p(out["ctx"]))
        return out

    def predict_byte(self, ppm, last_byte):
        x = np.ascontiguousarray(ppm, np.float32)
        probs = np.zeros(256, np.float32)
        ctx = C.c_uint32(0)
        self.L.lsr_predict_byte(self.p, _p(x), int(last_byte), _p(probs), C.byref(ctx))
        return probs, ctx.value

    def perceive_byte(self, byte):
        self.L.lsr_perceive_byte(self.p, int(byte))

    def export_long(self):
        buf = np.zeros(self.L.lsr_export_long(self.p, None), np.uint8)
        self.L.lsr_export_long(self.p, _p(buf))
        return buf.tobytes()

    def export_short(self):
        buf = np.zeros(self.L.lsr_export_short(self.p, None), np.uint8)
        self.L.lsr_export_short(self.p, _p(buf))
        return buf.tobytes()

    def clip_counts(self):
        """How many elements ClipGradients moved so far in (state_error_, stored_error_, hidden_error_)."""
        c = np.zeros(3, np.uint64)
        self.L.lsr_clip_counts(self.p, _p(c))
        return tuple(int(x) for x in c)

    def backward_passes(self):
        return int(self.L.lsr_backward_passes(self.p))

    def update_steps(self):
        """LstmLayer::update_steps_: Adam's step count, which stops at update_limit 3000."""
        return int(self.L.lsr_update_steps(self.p))

    def memory_usage(self):
        return int(self.L.lsr_memory_usage(self.p))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the hard regimes and the corners of the advertised range (tests/test_lstm_shape_census.py counts them on the CPU,
# tests/test_gpu_lstm_shape_regimes.py recounts and then looks at the general kernel) ----------------------------------
_CLAMP = np.float32(np.log(np.float32(np.float32(0.9999) / (np.float32(1) - np.float32(0.9999)))))


def regime_evidence(ref, out):
    """What the restatement alone says about a run: `out` is what ref.run() returned, the counters are ref's (they
    count from its creation).  zero_probs, silent_bits and clamped_logits as goldenlib.lstm_regime_evidence defines them:
    softmax outputs exactly 0.0f; bits where the model stayed silent (denom == 0: not active, the previous prediction
    repeated and not the 0 an inactive p == 0.5 stores); predictions at +-logit(0.9999f).  clips: Ref.clip_counts().
    nan: NaNs among the distributions, the gate weights and the output layer -- a row that reaches one pins nothing."""
    flat, fact = out["pred"].reshape(-1), out["act"].reshape(-1)
    prev = np.concatenate([[np.float32(0)], flat[:-1]])
    silent = int(((fact == 0) & (u32(flat) == u32(prev)) & (flat != 0)).sum())
    nan = int(np.isnan(out["probs"]).sum() + np.isnan(ref.weights()).sum() + np.isnan(ref.output_layer()).sum())
    return dict(zero_probs=int((out["probs"] == 0.0).sum()), silent_bits=silent,
                clamped_logits=int((np.abs(flat) >= _CLAMP).sum()), clips=ref.clip_counts(),
                backward_passes=ref.backward_passes(), update_steps=ref.update_steps(), nan=nan)


def assert_needs(row, s, ev):
    """The counts a row exists for are there (on the stream `on` that reaches them), and no stream met a NaN."""
    assert ev["nan"] == 0, (row["shape"], s, ev)
    if s != row.get("on", s):
        return
    for k in row["needs"]:
        v = min(ev[k][:2]) if k == "clips" else ev[k]      # clips: in state_error_ and in stored_error_
        assert v > 0, (row["shape"], s, k, ev)


# Shaped banks, three launches by chunks_for (at horizon 256 and 513 bytes these are 255, 257 and 1 bytes).  Stream s has
# gate weights of seed `wseed` + s and the inputs make_streams(seed = `seed`) gives it: stream 1 is the sparse / one-hot
# family, where the hot shapes reach their regimes.  lin = 257 + cells, hid = cells + 1, cp = cells rounded up to 64.
CORNER_ROWS = [
    # lin 320 and hid 64 fill their 64-float pitches; 10 passes
    dict(shape=(63, 4, 8.0, 0.5), S=3, N=41, needs=("clips", "clamped_logits"), on=1),
    # lin 512 and hid 256 fill theirs
    dict(shape=(255, 9, 30.0, 0.05), S=3, N=46, needs=("zero_probs", "silent_bits", "clamped_logits", "clips"), on=1),
    # cp exactly 128
    dict(shape=(128, 3, 0.03, 10.0), S=3, N=10, needs=()),
    # odd horizon, tiny clip, huge rate
    dict(shape=(7, 33, 100.0, 0.001), S=3, N=200, needs=("zero_probs", "silent_bits", "clamped_logits", "clips"), on=1),
    # the horizon maximum with one cell
    dict(shape=(1, 256, 0.03, 10.0), S=3, N=769, needs=()),
    # cp 192 (576 items), the horizon maximum
    dict(shape=(192, 256, 4.0, 0.2), S=2, N=513, needs=("clips", "clamped_logits"), on=1),
    # both maxima: the largest bank
    dict(shape=(256, 256, 0.03, 10.0), S=2, N=513, needs=("clips",), on=0),
]
for _r in CORNER_ROWS:
    _r.setdefault("seed", 76)
    _r.setdefault("wseed", 4)

# One ragged launch, then learning on, off across two horizon boundaries, and on again
SWITCH_ROW = dict(shape=(63, 4, 8.0, 0.5), S=3, ragged=[0, 3, 9], schedule=[(14, True), (7, False), (20, True)],
                  seed=76, wseed=4, needs=("clips", "clamped_logits"), on=1)

# Many backward passes in one launch, and Adam's step count at update_limit 3000: two streams over the SAME 6101 bytes
# (synth seed 77), stream 1 with other gate weights and its launches one byte off stream 0's, so that its passes fall at
# other rows of the launch's Adam table.  The first launch holds 2000 passes, the 3000th falls inside the second.
LIMIT_BYTES, LIMIT_LAUNCHES = 6101, [[4001, 2050, 50], [4000, 2050, 51]]
LIMIT_ROWS = [
    dict(shape=(3, 2, 0.03, 10.0), family=0, seed=77, wseed=5, needs=(), passes=3050, steps=3000),
    dict(shape=(2, 2, 2.0, 1.0), family=1, seed=77, wseed=5, needs=("clips", "clamped_logits"), passes=3050, steps=3000),
]


def limit_inputs(gmxo, row):
    """(ppm, data) of LIMIT_BYTES bytes, and of the 10 bytes that follow the export / import."""
    return (gmxo.lstm_synth(LIMIT_BYTES, seed=row["seed"], mask=255, family=row["family"]),
            gmxo.lstm_synth(10, seed=row["seed"] + 1, mask=255, family=row["family"]))


def run_refs(row, streams):
    """[(Ref, its initial gate weights, what its run() over the stream's whole input returned)]: stream s draws its
    weights from seed row["wseed"] + s."""
    refs = []
    for s, (ppm, data) in enumerate(streams):
        r = Ref(row["shape"], seed=row["wseed"] + s)
        w0 = r.weights()
        refs.append((r, w0, r.run(ppm, data)))
    return refs


def switch_evidence(row, streams):
    """SWITCH_ROW on the restatement alone: [regime_evidence over the ragged launch and the whole schedule] per stream;
    a stretch without Learn runs no backward pass."""
    evs = []
    for s, (ppm, data) in enumerate(streams):
        r = Ref(row["shape"], seed=row["wseed"] + s)
        pos = row["ragged"][s]
        outs = [r.run(ppm[:pos], data[:pos])]
        for n, learn in row["schedule"]:
            before = r.backward_passes()
            outs.append(r.run(ppm[pos:pos + n], data[pos:pos + n], learn=learn))
            assert learn or r.backward_passes() == before
            pos += n
        evs.append(regime_evidence(r, {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}))
    return evs


# The stock kernel's fixtures (tests/golden/cases.py) replayed on a stock-shape bank of the general layout
ANY_FIXTURES = ["lstm_saturated", "lstm_onehot", "lstm_clipped", "lstm_short"]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def golden():
    """[{name, shape, seed, synth_seed, mask, family, n_bytes, probs (uint32 [n,256]), sha_weights, sha_output_layer,
    sha_long, sha_short, clips (3), backward_passes}] of tests/golden/lstm_shapes.npz."""
    if "golden" not in _cache:
        z = np.load(GOLDEN)
        cases = []
        for name in z["names"]:
            name = str(name)
            g = lambda k: z[name + "_" + k]
            cases.append(dict(name=name, shape=(int(g("cells")), int(g("horizon")), float(g("lr")), float(g("clip"))),
                              seed=int(g("seed")), synth_seed=int(g("synth_seed")), mask=int(g("mask")),
                              family=int(g("family")), n_bytes=int(g("n_bytes")), probs=g("probs"),
                              sha_weights=str(g("sha_weights")), sha_output_layer=str(g("sha_output_layer")),
                              sha_long=str(g("sha_long")), sha_short=str(g("sha_short")),
                              clips=tuple(int(x) for x in g("clips")), backward_passes=int(g("backward_passes"))))
        _cache["golden"] = cases
    return _cache["golden"]
