"""Shared by the Match tests: the fixtures the reference produced (tests/golden/match_*.npz, made by
tests/golden/make_match_golden.py) and tests/helpers/match_ref.c, the plain-C restatement, through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

from gmix_amd.match import stream_bits

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
FIXTURES = ["match_stock", "match_tiny", "match_k8"]
# what make_match_golden.py demanded of the reference's own counters (see there for the one exemption: with this
# stream generator the tiny tables never keep a pointer far enough behind the history's end for 255 matching bits)
NEED = dict(not_pushed=200, eoh_resets=1, bits_at_255=400, same_entry=20)
EXEMPT = {("match_tiny", "bits_at_255")}
_cache = {}


def slot_hash(u):
    """FNV-1a over the K 32-bit patterns of every bit's slots: u [T][K] uint32 -> [T] uint32."""
    h = np.full(len(u), 2166136261, np.uint64)
    for k in range(u.shape[1]):
        h = ((h ^ u[:, k].astype(np.uint64)) * np.uint64(16777619)) & np.uint64(0xffffffff)
    return h.astype(np.uint32)


class Fixture:
    def __init__(self, name):
        z = np.load(os.path.join(GOLD, name + ".npz"))
        self.name = name
        self.data = z["data"]
        self.tables = [int(t) for t in z["tables"]]
        self.limit = int(z["limit"])
        self.K = len(self.tables)
        self.T = 8 * len(self.data)
        self.ctx = np.repeat(z["ctx_bytes"], 8, axis=0)  # [T][K]: the variables do not move within a byte
        self.bits, self.bc = stream_bits(self.data)
        self.slot_hash = z["slot_hash"]
        self.act = np.unpackbits(z["act"])[:self.T * self.K].reshape(self.T, self.K)
        self.lm = z["lm"].astype(np.uint32)
        self.long = z["long"].tobytes()
        self.short = z["short"].tobytes()
        self.usage = [int(u) for u in z["usage"]]
        self.dense = [int(d) for d in z["dense"]]
        self.meta = {str(k): int(v) for k, v in zip(z["meta_keys"], z["meta_vals"])}

    def models(self):
        return [(t, self.limit) for t in self.tables]


def fixture(name):
    if name not in _cache:
        _cache[name] = Fixture(name)
    return _cache[name]


def ref_lib():
    """tests/helpers/match_ref.c, built like test_oracle.py builds a3_single.c."""
    if "lib" in _cache:
        return _cache["lib"]
    src = os.path.join(HERE, "helpers", "match_ref.c")
    out = os.path.join(HERE, "helpers", "match_ref.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out, "-lm"])
    L = C.CDLL(out)
    vp, u64 = C.c_void_p, C.c_uint64
    L.mref_create.restype = vp
    L.mref_create.argtypes = [C.c_int, vp, vp]
    L.mref_destroy.argtypes = [vp]
    L.mref_destroy.restype = None
    L.mref_run.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
    L.mref_run.restype = None
    L.mref_history_size.argtypes = [vp]
    L.mref_history_size.restype = u64
    L.mref_slots_get.argtypes = [vp, vp, C.POINTER(C.c_int)]
    L.mref_slots_get.restype = None
    L.mref_slots_set.argtypes = [vp, vp, C.c_int]
    L.mref_slots_set.restype = None
    L.mref_export_long.argtypes = [vp, vp]
    L.mref_export_long.restype = u64
    L.mref_export_short.argtypes = [vp, vp]
    L.mref_export_short.restype = None
    L.mref_import.argtypes = [vp, vp, u64, vp, u64]
    L.mref_memory_usage.argtypes = [vp, C.c_int]
    L.mref_memory_usage.restype = u64
    _cache["lib"] = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Ref:
    """One stream of K Match models in match_ref.c."""

    def __init__(self, models):
        self.L = ref_lib()
        self.K = len(models)
        t = np.array([m[0] for m in models], np.uint32)
        l = np.array([m[1] for m in models], np.int32)
        self.h = self.L.mref_create(self.K, _p(t), _p(l))
        assert self.h

    def __del__(self):
        if getattr(self, "h", None):
            self.L.mref_destroy(self.h)
            self.h = None

    def run(self, ctx, bc, bits):
        """-> (slots [T][K] as uint32 patterns, active [T][K], longest [T])"""
        T = len(bits)
        ctx = np.ascontiguousarray(ctx, np.uint32)
        bc = np.ascontiguousarray(bc, np.uint32)
        bits = np.ascontiguousarray(bits, np.uint8)
        assert ctx.shape == (T, self.K)
        pred = np.zeros((T, self.K), np.float32)
        act = np.zeros((T, self.K), np.uint8)
        lm = np.zeros(T, np.uint32)
        if T:
            self.L.mref_run(self.h, T, _p(ctx), _p(bc), _p(bits), _p(pred), _p(act), _p(lm))
        return pred.view(np.uint32), act, lm

    def export(self):
        n = self.L.mref_export_long(self.h, None)
        lb = np.zeros(max(1, n), np.uint8)
        self.L.mref_export_long(self.h, _p(lb))
        sb = np.zeros(11 * self.K, np.uint8)
        self.L.mref_export_short(self.h, _p(sb))
        return lb[:n].tobytes(), sb.tobytes()

    def import_(self, long_bytes, short_bytes):
        lb, sb = np.frombuffer(long_bytes, np.uint8), np.frombuffer(short_bytes, np.uint8)
        assert self.L.mref_import(self.h, _p(lb), len(lb), _p(sb), len(sb)) == 0

    def slots(self):
        v = np.zeros(self.K, np.float32)
        nb = C.c_int(0)
        self.L.mref_slots_get(self.h, _p(v), C.byref(nb))
        return v, nb.value

    def set_slots(self, v, new_bit):
        v = np.ascontiguousarray(v, np.float32)
        self.L.mref_slots_set(self.h, _p(v), int(new_bit))

    def history_size(self):
        return self.L.mref_history_size(self.h)

    def memory_usage(self, k):
        return self.L.mref_memory_usage(self.h, k)
