"""What the analysis tests share: the checker (tests/cpp/analysis_check.cpp: gmix_amd/csrc/gmx_analysis.h built for the
host, loaded through ctypes -- never a machine's libm), the fixture tests/golden/analysis_trace.npz, the operand list the
fixture's `operands` case was recorded on, and the column tables of the stock Predictor."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INPUT, MIXER, FINAL_P = 0, 1, 2
N_INPUTS, N_MIXERS = 90, 33          # the stock Predictor's blackboard and mixers (24 / 8 / 1)
START = -1.0                         # entropy[] as the Predictor's constructor leaves it (predictor.cpp:39)
TILE = 64                            # GMX_AN_TILE: bits of a tile of gmx_analysis_kernel

_lib = None
_dir = None


def checker():
    """The host-built header as a ctypes library (built once per process)."""
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="gmx_analysis_check_")
        so = os.path.join(_dir.name, "libanalysis_check.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-pthread",
                               "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", so,
                               os.path.join(ROOT, "tests", "cpp", "analysis_check.cpp")])
        L = C.CDLL(so)
        u32p, u64p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
        L.an_log2f.argtypes, L.an_log2f.restype = [C.c_float], C.c_float
        L.an_logistic.argtypes, L.an_logistic.restype = [C.c_float], C.c_float
        L.an_entropy.argtypes, L.an_entropy.restype = [C.c_float, C.c_int], C.c_float
        L.an_entropy_of_prob.argtypes, L.an_entropy_of_prob.restype = [C.c_float, C.c_int], C.c_float
        L.an_step.argtypes, L.an_step.restype = [C.c_double, C.c_float], C.c_double
        for f in (L.an_sweep_log2f, L.an_sweep_prob):
            f.argtypes, f.restype = [C.c_uint32, C.c_uint32, C.c_int, u32p], C.c_uint64
        L.an_thresholds.argtypes, L.an_thresholds.restype = [C.POINTER(C.c_float)], None
        L.an_run.argtypes = [f64p, u64p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, f64p, u64p,
                             C.c_uint64, f64p]
        L.an_run.restype = C.c_uint64
        _lib = L
    return _lib


def thresholds():
    out = (C.c_float * 4)()
    checker().an_thresholds(out)
    return np.array(list(out), np.float32)


class Stream:
    """One stream of the device object as the checker walks it."""

    def __init__(self, n_columns, is_prob=None, ema=None, bits_seen=0, frequency=0):
        self.C = n_columns
        self.is_prob = np.zeros(n_columns, np.uint8) if is_prob is None else np.ascontiguousarray(is_prob, np.uint8)
        self.ema = np.zeros(n_columns, np.float64) if ema is None else np.array(ema, np.float64)
        self.bits_seen = int(bits_seen)
        self.F = int(frequency)
        self.rows, self.labels = [], []

    def run(self, values, bits, trail=False):
        """values [n][C] float32, bits [n]; returns the averages after every bit with trail=True."""
        v = np.ascontiguousarray(values, np.float32).reshape(-1, self.C)
        b = np.ascontiguousarray(bits, np.uint8)
        n = len(b)
        assert len(v) == n
        rows, labels = np.zeros((max(n, 1), self.C), np.float64), np.zeros(max(n, 1), np.uint64)
        tr = np.zeros((max(n, 1), self.C), np.float64) if trail else None
        seen = C.c_uint64(self.bits_seen)
        f64p = C.POINTER(C.c_double)
        k = checker().an_run(self.ema.ctypes.data_as(f64p), C.byref(seen), self.F, v.ctypes.data, self.is_prob.ctypes.data,
                             b.ctypes.data, n, self.C, rows.ctypes.data_as(f64p),
                             labels.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                             tr.ctypes.data_as(f64p) if trail else None)
        self.bits_seen = seen.value
        self.rows.extend(rows[:k])
        self.labels.extend(int(x) for x in labels[:k])
        return tr[:n] if trail else None

    def take(self):
        """(averages, bits_seen, rows [k][C], labels [k]) and the rows start anew, as after the device's take."""
        rows = np.array(self.rows, np.float64).reshape(-1, self.C)
        labels = np.array(self.labels, np.uint64)
        self.rows, self.labels = [], []
        return self.ema.copy(), self.bits_seen, rows, labels


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def fixture():
    return np.load(os.path.join(GOLDEN, "analysis_trace.npz"))


def stock_columns(indexes):
    """entropy[] indexes of the stock Predictor -> the device object's (kind, index) columns: the blackboard's 90 slots,
    then the 24 + 8 + 1 mixers in construction order."""
    return [(INPUT, int(i)) if i < N_INPUTS else (MIXER, int(i) - N_INPUTS) for i in indexes]


def column_values(cols, pred, act, outputs, p):
    """values [n][C] and is_prob [C] for the checker, from a trace's arrays: a silent slot is 0."""
    n = len(p)
    v = np.zeros((n, len(cols)), np.float32)
    is_prob = np.zeros(len(cols), np.uint8)
    for c, (kind, i) in enumerate(cols):
        if kind == INPUT:
            v[:, c] = pred[:, i] if act is None else np.where(act[:, i] != 0, pred[:, i], np.float32(0))
        elif kind == MIXER:
            v[:, c] = outputs[:, i]
        else:
            v[:, c] = p
            is_prob[c] = 1
    return v, is_prob


SPECIALS = [0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0, np.inf, -np.inf]


def operand_records(thr, n_seeded=2000, seed=31):
    """(x [k] float32, bit [k] uint8): the special values and the floats on either side of each clamp threshold with
    both bits, then n_seeded seeded values (logits of every size the mixers produce, some far outside) with seeded bits."""
    xs = [np.float32(v) for v in SPECIALS] + [np.float32(v) for v in thr]
    x = np.array([v for v in xs for _ in (0, 1)], np.float32)
    bit = np.array([b for _ in xs for b in (0, 1)], np.uint8)
    rng = np.random.default_rng(seed)
    scale = rng.choice(np.array([0.05, 1.0, 3.0, 8.0, 40.0], np.float32), n_seeded)
    sx = (rng.standard_normal(n_seeded).astype(np.float32) * scale).astype(np.float32)
    sb = rng.integers(0, 2, n_seeded).astype(np.uint8)
    return np.concatenate([x, sx]), np.concatenate([bit, sb])
