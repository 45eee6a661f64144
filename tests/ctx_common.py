"""Shared by the context-bank tests: the fixtures the reference produced (tests/golden/ctx_*.npz, made by
tests/golden/make_ctx_golden.py) and tests/helpers/ctx_ref.c, the plain-C restatement, through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

from gmix_amd._lib import CtxBlackboard, CtxDesc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
FIXTURES = ["ctx_stock", "ctx_tiny"]
PER_BIT_KINDS = (1, 3)   # BIT_CONTEXT, BYTE_PLUS_RECENT: they move within a byte
BOARD_BYTES = C.sizeof(CtxBlackboard)
_cache = {}


def bit_contexts(data):
    """[8n] bit_context of every bit of a byte stream (MSB first)."""
    b = np.unpackbits(np.asarray(data, np.uint8)).reshape(-1, 8).astype(np.uint32)
    bc = np.zeros_like(b)
    for i in range(1, 8):
        bc[:, i] = ((bc[:, i - 1] + 1) << 1 | b[:, i - 1]) - 1
    return bc.reshape(-1)


def descs_from_bytes(raw):
    n = len(raw) // C.sizeof(CtxDesc)
    arr = (CtxDesc * n).from_buffer_copy(bytes(raw))
    return [arr[i] for i in range(n)]


def board_from_bytes(raw):
    return CtxBlackboard.from_buffer_copy(bytes(raw))


def board_bytes(bb):
    return bytes(bb)


class Fixture:
    def __init__(self, name):
        z = np.load(os.path.join(GOLD, name + ".npz"))
        self.name = name
        self.data = z["data"]
        self.bits = np.unpackbits(self.data)
        self.T = len(self.bits)
        self.descs = descs_from_bytes(z["descs"].tobytes())
        self.names = [str(n) for n in z["names"]]
        self.V = len(self.descs)
        self.kinds = [d.kind for d in self.descs]
        self.hash_vars = [i for i, k in enumerate(self.kinds) if k == 6]
        self.H = len(self.hash_vars)
        self.byte_vals = z["byte_vals"]              # [n_bytes][V]; per-bit kinds hold their value at the byte's first bit
        self.positions = [int(p) for p in z["positions"]]
        sec, off = z["sections"].tobytes(), z["section_off"]   # [P][H + 1] offsets into sec
        self.sections = [[sec[off[p][h]:off[p][h + 1]] for h in range(self.H)] for p in range(len(self.positions))]
        self.boards = [board_from_bytes(b.tobytes()) for b in z["boards"]]
        self.boundary = {str(k): int(v) for k, v in zip(z["boundary_keys"], z["boundary_vals"])}
        self.meta = {str(k): int(v) for k, v in zip(z["meta_keys"], z["meta_vals"])}

    def values(self):
        """[T][V]: the variables at Predict of every bit, rebuilt from the per-byte rows."""
        if not hasattr(self, "_values"):
            v = np.repeat(self.byte_vals, 8, axis=0)
            bc = bit_contexts(self.data)
            for i, k in enumerate(self.kinds):
                if k in PER_BIT_KINDS:
                    v[:, i] += bc
            v.setflags(write=False)
            self._values = v
        return self._values

    def section(self, p):
        return b"".join(self.sections[p])


def fixture(name):
    if name not in _cache:
        _cache[name] = Fixture(name)
    return _cache[name]


def ref_lib():
    """tests/helpers/ctx_ref.c, built like match_common.py builds match_ref.c."""
    if "lib" in _cache:
        return _cache["lib"]
    src = os.path.join(HERE, "helpers", "ctx_ref.c")
    out = os.path.join(HERE, "helpers", "ctx_ref.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", src, "-o", out])
    L = C.CDLL(out)
    vp, u64 = C.c_void_p, C.c_uint64
    L.cref_create.restype = vp
    L.cref_create.argtypes = [C.c_int, vp]
    L.cref_destroy.argtypes = [vp]
    L.cref_destroy.restype = None
    L.cref_run.argtypes = [vp, u64, vp, vp]
    L.cref_run.restype = None
    L.cref_board_get.argtypes = [vp, C.POINTER(CtxBlackboard)]
    L.cref_board_get.restype = None
    L.cref_board_set.argtypes = [vp, C.POINTER(CtxBlackboard)]
    L.cref_board_set.restype = None
    L.cref_export.argtypes = [vp, vp, vp]
    L.cref_export.restype = u64
    L.cref_import.argtypes = [vp, vp, u64]
    _cache["lib"] = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Ref:
    """One stream of V context variables in ctx_ref.c."""

    def __init__(self, descs):
        self.L = ref_lib()
        self.V = len(descs)
        self.H = sum(1 for d in descs if d.kind == 6)
        arr = (CtxDesc * self.V)(*descs)
        self.h = self.L.cref_create(self.V, C.cast(arr, C.c_void_p))
        assert self.h

    def __del__(self):
        if getattr(self, "h", None):
            self.L.cref_destroy(self.h)
            self.h = None

    def run(self, bits, values=True):
        """-> [T][V] uint32 (or None)"""
        bits = np.ascontiguousarray(bits, np.uint8)
        out = np.zeros((len(bits), self.V), np.uint32) if values else None
        if len(bits):
            self.L.cref_run(self.h, len(bits), _p(bits), _p(out) if values else None)
        return out

    def board(self):
        bb = CtxBlackboard()
        self.L.cref_board_get(self.h, C.byref(bb))
        return bb

    def set_board(self, bb):
        self.L.cref_board_set(self.h, C.byref(bb))

    def export(self):
        """(bytes, offsets [H + 1])"""
        off = np.zeros(self.H + 1, np.uint64)
        n = self.L.cref_export(self.h, None, _p(off))
        buf = np.zeros(max(1, n), np.uint8)
        self.L.cref_export(self.h, _p(buf), _p(off))
        return buf[:n].tobytes(), [int(o) for o in off]

    def import_(self, data):
        buf = np.frombuffer(data or b"\0", np.uint8)
        assert self.L.cref_import(self.h, _p(buf), len(data)) == 0
