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

    def memory_usage(self):
        return int(self.L.lsr_memory_usage(self.p))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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
