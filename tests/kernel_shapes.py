"""Shared helpers for the tests that reach every route of the batched dispatcher (kernel_for() and
gmx_pick_bank_kernel in gmix_amd/csrc): seeded topology generators per route, synthetic-stream patterns
whose contexts exceed the gate tables, the route probe, and a runner for the reference's own Mixer
(oracle/_ref/ref_mixer_harness, present where the reference was built)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from gmix_amd import topology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_mixer_harness")

# gmx_debug_kernel_kind: kernel_for()'s kind, + 4 x the bank build (0 run-time, 1 / 2 unrolled 24/8/1)
SINGLE, WIDE, STOCK, BANK = 0, 1, 2, 3
BANK_UNROLLED_128 = BANK + 4   # gmx_bank_kernel<..., 24, 8, 1, 1, 32, 1>: stride0 65..128
BANK_UNROLLED_512 = BANK + 8   # gmx_bank_kernel<..., 24, 8, 1, 1, 64, 2>: stride0 257..512
MODE_PREDICT, MODE_LEARN = 1, 2

# gate-table sizes that are not powers of two, beside a few that are
ODD_TABLES = [1, 3, 5, 7, 1000, 4097, 65537]
POW2_TABLES = [1, 2, 8, 256, 4096, 65536]
# the large ones cost 4 x stride x table bytes per mixer and stream: a few per topology
LARGE = 4000


def kernel_kind(g, mode=MODE_PREDICT | MODE_LEARN):
    g.L.gmx_debug_kernel_kind.argtypes = [C.c_void_p, C.c_uint]
    g.L.gmx_debug_kernel_kind.restype = C.c_int
    k = g.L.gmx_debug_kernel_kind(g.h, mode)
    assert k >= 0, k
    return k


def learning_rate(rng):
    """About 1e-5..0.05, log-uniform, as the float the reference's Mixer receives."""
    return float(np.float32(10.0 ** rng.uniform(-5.0, np.log10(0.05))))


def _tables(rng, count, pow2, max_large, small=False):
    pool = POW2_TABLES if pow2 else ODD_TABLES + POW2_TABLES[:3]
    if small:
        pool = [t for t in pool if t <= 8]
    out = []
    for _ in range(count):
        t = int(rng.choice(pool))
        while t > LARGE and sum(x > LARGE for x in out) >= max_large:
            t = int(rng.choice([x for x in pool if x <= LARGE]))
        out.append(t)
    if not pow2 and all(t & (t - 1) == 0 for t in out):
        out[int(rng.integers(0, count))] = 3
    return out


def skip_index(seed, n):
    """0, 1, a middle index, n-1 -- by seed."""
    return [0, 1, n // 2, n - 1][seed % 4]


def topo_24_8_1(n, seed, pow2=False, max_large=3, skip=None, small=False):
    """24/8/1 with one skip input: mixed table sizes, random learning rates, the skip input moved (`small`:
    tables of at most 8 rows)."""
    rng = np.random.default_rng(7000 + 31 * n + seed)
    t0 = _tables(rng, 24, pow2, max_large, small)
    t1 = _tables(rng, 8, pow2, 1, small)
    tf = int(rng.choice([1, 2, 3, 5])) if not pow2 else int(rng.choice([1, 2, 4]))
    mixers = ([(0, t, learning_rate(rng)) for t in t0] + [(1, t, learning_rate(rng)) for t in t1] +
              [(2, tf, learning_rate(rng))])
    return topology.Topology(n, mixers, skip=(skip_index(seed, n) if skip is None else skip,))


def stock_like(seed, pow2=False):
    """The stock route's shape (90 inputs, 24/8/1, one skip input) with tables, rates and skip of its own."""
    return topo_24_8_1(90, seed, pow2=pow2)


def wide_like(seed):
    """The wide route's 256-input 24/8/1 shape."""
    return topo_24_8_1(256, seed, max_large=2)


def single_like(n, table, seed):
    rng = np.random.default_rng(9000 + n + seed)
    return topology.Topology(n, [(0, table, learning_rate(rng))], skip=() if n < 2 else (n - 1,))


def random_topology(rng):
    """test_gpu_random_topologies' generator: odd input counts, several skip inputs, missing layers."""
    n = int(rng.choice([1, 2, 3, 7, 31, 64, 90, 129, 200, 256]))
    l0 = int(rng.integers(1, 7))
    l1 = int(rng.integers(0, 4))
    fin = bool(rng.integers(0, 2)) if l1 else bool(rng.integers(0, 2))
    n_skip = int(rng.integers(0, min(n, 3) + 1)) if (l1 or fin) else 0
    skip = sorted(rng.choice(n, size=n_skip, replace=False).tolist()) if n_skip else []
    sizes = [1, 2, 3, 5, 8, 100, 257, 1000, 4096]
    mixers = [(0, int(rng.choice(sizes)), float(rng.choice([0.0005, 0.003, 0.02]))) for _ in range(l0)]
    mixers += [(1, int(rng.choice(sizes)), float(rng.choice([0.0005, 0.003]))) for _ in range(l1)]
    if fin:
        mixers += [(2, int(rng.choice([1, 3, 64])), 0.001)]
    return topology.Topology(n, mixers, skip=skip)


def random_case(seed):
    """(topology, T, synth kwargs, rng) of test_gpu_random_topologies' case `seed`; the rng goes on to
    draw that test's mask choice and cuts."""
    rng = np.random.default_rng(1000 + seed)
    topo = random_topology(rng)
    T = int(rng.integers(300, 900))
    kw = dict(ctx_mode=int(rng.integers(0, 4)), ctx_mod=int(rng.choice([1, 2, 7, 300])),
              zero_mod=int(rng.choice([0, 0, 3, 9])), bit_mode=int(rng.integers(0, 2)))
    if seed >= 12:
        kw["ctx_mode"] = 4 + (seed & 1)   # byte-held contexts with a few that move every bit
    return topo, T, kw, rng


# Synthetic-stream patterns (oracle/gmx_synth.h).  Contexts larger than every table come first: below the
# table size ctx % t and ctx & (t-1) agree on more rows than not, and the row-index branch goes untested.
PATTERNS = [
    dict(ctx_mode=0),                                       # 32-bit contexts, every row changes every bit
    dict(ctx_mode=1, ctx_mod=200003, zero_mod=5, bit_mode=1),  # above every table, silent inputs
    dict(ctx_mode=3, ctx_mod=70001, zero_mod=7, bit_mode=1),   # byte-held, rows persist
    dict(ctx_mode=4, zero_mod=11, bit_mode=1),              # a real run's pattern: 4 rows move every bit
    dict(ctx_mode=5, ctx_mod=3, bit_mode=1),                # a handful of rows: write-back, refetch
    dict(ctx_mode=1, ctx_mod=2, bit_mode=1),                # >1024 visits per row: shrink
]


def pattern(seed):
    return dict(PATTERNS[seed % len(PATTERNS)])


def have_reference():
    return os.path.exists(HARNESS)


def topo_spec(topo):
    return ",".join(f"{l}:{t}:{lr!r}" for l, t, lr in topo.mixers)


def reference_run(topo, T, seed, synth_kw, dump, nolearn_from=None):
    """The reference's own Mixer over the synthetic stream (seed, synth_kw): read_dump()'s dict.
    The command line is tests/golden/make_golden.py's."""
    from oracle import gmxo
    args = [HARNESS, "--n", str(topo.n_inputs), "--topo", topo_spec(topo),
            "--skip", ",".join(map(str, topo.skip)) if topo.skip else "none", "--bits", str(T),
            "--dump", str(dump), "--seed", str(seed)]
    for k, flag in (("ctx_mode", "--ctx-mode"), ("ctx_mod", "--ctx-mod"), ("zero_mod", "--zero-mod"),
                    ("bit_mode", "--bit-mode")):
        if k in synth_kw:
            args += [flag, str(synth_kw[k])]
    if nolearn_from is not None:
        args += ["--nolearn-from", str(nolearn_from)]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "d.bin")
        subprocess.run(args + ["--out", out], check=True, stdout=subprocess.DEVNULL)
        return gmxo.read_dump(out)


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def oracle_run(oracle, topo, T, seed, synth_kw, nolearn_from=None):
    """(bank, p, outs, records) of the oracle over the same stream."""
    rec = oracle.synth(topo.n_inputs, topo.n_mixers, T, seed=seed, **synth_kw)
    ob = oracle.Bank(topo.n_inputs, topo.skip, topo.mixers)
    p, outs = ob.run(*rec, nolearn_from=nolearn_from)
    return ob, p, outs, rec


def assert_oracle_is_reference(ob, p, outs, d, tag):
    """The oracle's run against the reference's dump of the same stream, bit for bit."""
    m = ob.m
    assert np.array_equal(u32(outs), u32(d["outs"])), (tag, "outputs")
    assert np.array_equal(u32(p), u32(d["p"])), (tag, "p")
    assert ob.export_short() == d["short"], (tag, "short")
    assert ob.export_long() == d["long"], (tag, "long")
    assert [ob.memory_usage(j) for j in range(m)] == [int(x) for x in d["mem"]], (tag, "memory_usage")


# Input counts of the 24/8/1 bank around the unrolled builds' stride0 ranges (stride0 = round_up(n + 23, 32)):
# inside them (away from the folded 90 / 256) and just outside.
BANK_UNROLLED_N = {42: BANK_UNROLLED_128, 73: BANK_UNROLLED_128, 74: BANK_UNROLLED_128, 100: BANK_UNROLLED_128,
                   105: BANK_UNROLLED_128, 234: BANK_UNROLLED_512, 300: BANK_UNROLLED_512, 489: BANK_UNROLLED_512}
BANK_RUNTIME_N = [41, 106, 233, 490]


def route_cases():
    """id -> (topology factory, expected route, T, first stream seed, synth kwargs, nolearn_from) of every route,
    the ones the CPU test pins to the reference and the GPU test runs through the kernels."""
    cases = {}
    for s in range(8):
        cases[f"stock_odd{s}"] = (lambda s=s: stock_like(s), STOCK, 500 + 37 * s, 301 + s, pattern(s),
                                  None if s % 2 else 440 + 37 * s)
    for s in range(2):
        cases[f"stock_pow2_{s}"] = (lambda s=s: stock_like(10 + s, pow2=True), STOCK, 600, 401 + s,
                                    pattern(s), None)
    for s in range(4):
        cases[f"wide{s}"] = (lambda s=s: wide_like(s), WIDE, 400 + 50 * s, 501 + s, pattern(s + 1),
                             None if s % 2 else 350 + 50 * s)
    for i, (n, route) in enumerate(BANK_UNROLLED_N.items()):
        cases[f"bank24_n{n}"] = (lambda n=n, i=i: topo_24_8_1(n, i, max_large=2), route, 400, 601 + i, pattern(i),
                                 None if i % 3 else 360)
    for i, n in enumerate(BANK_RUNTIME_N):
        cases[f"bank24_n{n}"] = (lambda n=n, i=i: topo_24_8_1(n, i, max_large=2), BANK, 400, 701 + i,
                                 pattern(i + 2), None)
    for i, (n, table) in enumerate([(1, 1), (2, 3), (255, 1), (256, 4097)]):
        cases[f"single_n{n}_t{table}"] = (lambda n=n, table=table, i=i: single_like(n, table, i), SINGLE, 700,
                                          801 + i, pattern(i), None)
    return cases
