"""Shared by the tests of the PPMd bank (gmx_ppmd, include/gmxmix_ppmd.h): the seeded inputs of
tests/golden/ppmd_trace.npz, the fixture's layout, and the host build of gmix_amd/csrc/gmx_ppmd.h
(tests/cpp/test_ppmd.cpp) that the CPU tests check against the fixture and the GPU tests check the kernel against."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ppmd_trace.npz")
SEED = 88172645463325252
M64 = (1 << 64) - 1
ORDER, ARENA_MB = 20, 1
HEAD, WINDOW, HASH_EVERY = 256, 64, 256
FLUSH_DROP = 65536        # a model flush: `used` falls by more than this within one byte (no other step frees 1/16 MiB)

# name -> (generator, bytes, order, whether the fixture must show a flush)
CASES = {
    "sym3": ("sym3", 46000, 20, True),
    "rand256": ("rand256", 50000, 20, True),
    "abcd": ("abcd", 56000, 20, True),
    "noisy500": ("noisy500", 60000, 20, False),
    "e-run": ("e-run", 20000, 20, False),
    "rand256_o4": ("rand256", 8000, 4, False),
    "sym3_o64": ("sym3", 8000, 64, False),
}


class Xorshift:
    def __init__(self):
        self.x = SEED

    def __call__(self):
        x = self.x
        x ^= (x << 13) & M64
        x ^= x >> 7
        x ^= (x << 17) & M64
        self.x = x
        return (x >> 24) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _gen(kind, n):
    r = Xorshift()
    if kind == "sym3":
        d = [(r() & 255) % 3 for _ in range(n)]
    elif kind == "rand256":
        d = [r() & 255 for _ in range(n)]
    elif kind == "abcd":
        d = [97 + r() % 4 for _ in range(n)]
    elif kind == "noisy500":
        block = [r() & 255 for _ in range(500)]
        d = []
        for i in range(n):
            v = block[i % 500]
            if (r() & 63) == 0:
                v = r() & 255
            d.append(v)
    elif kind == "e-run":
        d = [(97 + r() % 26) if r() % 50 == 0 else 101 for _ in range(n)]
    else:
        raise KeyError(kind)
    a = np.array(d, np.uint8)
    a.setflags(write=False)
    return a


def case_bytes(name, n=None):
    kind, full, _, _ = CASES[name]
    return _gen(kind, full)[:full if n is None else n]


def flushes(used):
    """Indices i at which used[i] fell by more than FLUSH_DROP from used[i - 1]."""
    u = np.asarray(used, np.int64)
    return [int(i) + 1 for i in np.nonzero(u[:-1] - u[1:] > FLUSH_DROP)[0]]


def full_rows(n, fl):
    """The byte indices whose whole distribution the fixture holds."""
    rows = set(range(min(HEAD, n)))
    for f in fl:
        rows |= set(range(max(0, f - WINDOW), min(n, f + WINDOW)))
    return np.array(sorted(rows), np.int64)


# ---- the host build of the header ----
@functools.lru_cache(maxsize=None)
def host_lib(census=False):
    out = tempfile.mkdtemp(prefix="gmx_ppmd_host_")
    so = os.path.join(out, "libppmd_host%s.so" % ("_census" if census else ""))
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC",
           "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "cpp", "test_ppmd.cpp")]
    if census:
        cmd.insert(1, "-DGMX_PPMD_CENSUS")
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    shutil.rmtree(out)
    L.ppmd_host_create.restype = C.c_void_p
    L.ppmd_host_create.argtypes = [C.c_int, C.c_int]
    L.ppmd_host_destroy.argtypes = [C.c_void_p]
    L.ppmd_host_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int] + [C.c_void_p] * 5
    L.ppmd_host_restores.restype = C.c_uint32
    L.ppmd_host_restores.argtypes = [C.c_void_p]
    L.ppmd_host_memory_usage.restype = C.c_uint64
    L.ppmd_host_memory_usage.argtypes = [C.c_void_p]
    L.ppmd_host_census.restype = C.c_int
    L.ppmd_host_census.argtypes = [C.c_void_p, C.c_void_p]
    return L


class HostModel:
    """One stream of the restatement.  run(bytes): every byte is handed in as the byte coded last (ModPPMD::Predict at a
    byte boundary; the bank's gmx_ppmd_step); records(bytes): the bank's batch records (the bytes are the bytes being
    coded).  Both -> dict(ppm [n][256] uint32, pred [n][8] uint32 (run: the slot at bit 0 alone), active [n][8] uint8,
    used [n] uint64, hash [n] uint64 (the running FNV-1a over every ppm byte since create))."""

    def __init__(self, order=ORDER, arena_mb=ARENA_MB, census=False):
        self.L = host_lib(census)
        self.h = self.L.ppmd_host_create(order, arena_mb)
        assert self.h

    def run(self, data, want_ppm=True, records=False):
        d = np.ascontiguousarray(data, np.uint8)
        n = len(d)
        ppm = np.empty((n, 256), np.uint32) if want_ppm else None
        pred, active = np.empty((n, 8), np.uint32), np.empty((n, 8), np.uint8)
        used, h = np.empty(n, np.uint64), np.empty(n, np.uint64)
        self.L.ppmd_host_run(self.h, d.ctypes.data, n, 1 if records else 0, ppm.ctypes.data if want_ppm else None,
                             pred.ctypes.data, active.ctypes.data, used.ctypes.data, h.ctypes.data)
        return dict(ppm=ppm, pred=pred, active=active, used=used, hash=h)

    def records(self, data, want_ppm=True):
        return self.run(data, want_ppm, records=True)

    @property
    def restores(self):
        return int(self.L.ppmd_host_restores(self.h))

    @property
    def memory_usage(self):
        return int(self.L.ppmd_host_memory_usage(self.h))

    def close(self):
        if self.h:
            self.L.ppmd_host_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


CENSUS_NAMES = ("restore", "cutoff", "cut_free", "cut_fold", "cut_rescale", "cut_bin_free", "move_up", "glue", "rare_null",
                "split", "shift_rare", "rescale", "rescale_zero", "rescale_fold", "full_order", "bin_update", "reduce_order",
                "expand", "bin_to_two", "text_full")


def census():
    """The census build's counters since it was loaded: (dict by CENSUS_NAMES, contexts scanned by symbol count [257])."""
    L = host_lib(True)
    c = np.zeros(len(CENSUS_NAMES), np.uint64)
    ns = np.zeros(257, np.uint64)
    assert L.ppmd_host_census(c.ctypes.data, ns.ctypes.data) == len(CENSUS_NAMES)
    return dict(zip(CENSUS_NAMES, (int(v) for v in c))), ns
