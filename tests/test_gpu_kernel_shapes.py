"""Every route of the batched dispatcher (kernel_for(), gmx_pick_bank_kernel) at shapes the reference does not
use: the stock and wide kernels with gate tables that are not powers of two (the `ctx % t` row index, the
stock kernel's build with the mode tests), the skip input moved off index 1 and learning rates of their own;
the 24/8/1 bank at input counts whose layout does not fold the row-step counter into the row, inside and just
outside the unrolled builds' ranges; single mixers of 1..256 inputs.  Each case asserts its route through
gmx_debug_kernel_kind, runs launches cut at random places, and compares p, outputs, export() and memory_usage
bit for bit with the oracle -- and with the reference's own Mixer where oracle/_ref was built."""
import ctypes as C

import numpy as np
import pytest

import kernel_shapes as ks
from kernel_shapes import u32

pytestmark = pytest.mark.gpu

CASES = ks.route_cases()


def debug(g, staged=None, exact=None, pairs=None, variant=None):
    L = g.L
    for name in ("gmx_debug_stock_staged", "gmx_debug_stock_exact", "gmx_debug_stock_pairs",
                 "gmx_debug_single_variant"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int]
    if staged is not None:
        assert L.gmx_debug_stock_staged(g.h, staged) == 0
    if exact is not None:
        assert L.gmx_debug_stock_exact(g.h, 1 if exact else 0) == 0
    if pairs is not None:
        assert L.gmx_debug_stock_pairs(g.h, 1 if pairs else 0) == 0
    if variant is not None:
        assert L.gmx_debug_single_variant(g.h, variant) == 0


def cuts_for(rng, T, nolearn):
    """Launch boundaries: two random cuts, and the start of the forward-only tail."""
    c = {0, T} | set(rng.integers(1, T, size=2).tolist())
    if nolearn is not None:
        c.add(nolearn)
    return sorted(c)


def run_batched(gpu, topo, recs, cuts, nolearn, route, mask=True, outputs=True, last_outputs=False, **dbg):
    """The streams' records through g.run in the launches `cuts` gives; learning stops at `nolearn`.
    Returns (group, p[S,T], outputs[S,T,M] or None, [(t_last, last_outputs[S,M])])."""
    S, T, M = len(recs), len(recs[0][3]), topo.n_mixers
    g = gpu.MixerGroup(topo, S)
    debug(g, **dbg)
    assert ks.kernel_kind(g) == route, (ks.kernel_kind(g), route, topo.n_inputs, dbg)
    chunk = max(b - a for a, b in zip(cuts, cuts[1:]))
    b = gpu.Batch(g, chunk, outputs=outputs, mask=mask, last_outputs=last_outputs)
    P = np.zeros((S, T), np.float32)
    O = np.zeros((S, T, M), np.float32) if outputs else None
    lasts = []
    for t0, t1 in zip(cuts, cuts[1:]):
        n = t1 - t0
        for s, (pred, act, ctx, bits) in enumerate(recs):
            b.set_records(s, pred[t0:t1], act[t0:t1], ctx[t0:t1], bits[t0:t1])
        b.upload(n)
        learn = nolearn is None or t1 <= nolearn
        if not learn:
            assert ks.kernel_kind(g, ks.MODE_PREDICT) == route
        g.run(b, n, learn=learn)
        b.download(n)
        b.wait()
        P[:, t0:t1] = b.p[:, :n]
        if outputs:
            O[:, t0:t1] = b.outputs[:, :n]
        if last_outputs:
            lasts.append((t1 - 1, b.last_outputs.copy()))
    b.close()
    return g, P, O, lasts


def oracle_refs(oracle, topo, T, seeds, kw, nolearn):
    return [ks.oracle_run(oracle, topo, T, sd, kw, nolearn) for sd in seeds]


def check(g, topo, refs, P, O, lasts, tag):
    for s, (ob, p_ref, o_ref, _) in enumerate(refs):
        assert np.array_equal(u32(P[s]), u32(p_ref)), (tag, s, "p")
        if O is not None:
            assert np.array_equal(u32(O[s]), u32(o_ref)), (tag, s, "outputs")
        for t, lo in lasts:
            assert np.array_equal(u32(lo[s]), u32(o_ref[t])), (tag, s, t, "last_outputs")
        assert g.export(s) == (ob.export_long(), ob.export_short()), (tag, s, "export")
        assert [g.memory_usage(j, stream=s) for j in range(topo.n_mixers)] == \
            [ob.memory_usage(j) for j in range(topo.n_mixers)], (tag, s, "memory_usage")


def check_reference(g, topo, T, seed, kw, nolearn, P, O):
    """Stream 0 against the reference's own Mixer, where it was built."""
    if not ks.have_reference():
        return
    d = ks.reference_run(topo, T, seed, kw, T, nolearn)
    assert np.array_equal(u32(P[0]), u32(d["p"]))
    if O is not None:
        assert np.array_equal(u32(O[0]), u32(d["outs"]))
    assert g.export(0) == (d["long"], d["short"])
    assert [g.memory_usage(j, stream=0) for j in range(topo.n_mixers)] == [int(x) for x in d["mem"]]


def setup(oracle, cid, S=3):
    mk, route, T, seed, kw, nolearn = CASES[cid]
    topo = mk()
    seeds = [seed + 1000 * k for k in range(S)]
    refs = oracle_refs(oracle, topo, T, seeds, kw, nolearn)
    recs = [r[3] for r in refs]
    rng = np.random.default_rng(seed)
    return topo, route, T, seed, kw, nolearn, refs, recs, rng


STOCK_IDS = [c for c in CASES if c.startswith("stock_odd")]


@pytest.mark.parametrize("cid", STOCK_IDS)
def test_stock_route_odd_tables(gpu, oracle, cid):
    """The stock kernel's `ctx % t` rows and its build with the mode tests, skip input moved, rates of its own:
    mask on / off, outputs on / off, rows staged through LDS / lane-private, the masked forward chains, the
    lane-pair kernel at 90 inputs, outputs of the last bit only, a forward-only tail."""
    topo, route, T, seed, kw, nolearn, refs, recs, rng = setup(oracle, cid)
    assert any(t & (t - 1) for _, t, _ in topo.mixers)
    can_unmask = kw.get("zero_mod", 0) == 0   # without a mask a silent slot reads 0, not its stale value
    runs = [
        dict(staged=0, mask=True, outputs=True),
        dict(staged=1, mask=not can_unmask, outputs=False),
        dict(staged=1, mask=True, outputs=True, exact=True),
        dict(staged=0, mask=not can_unmask, outputs=False, last_outputs=True),
        dict(staged=1, mask=True, outputs=False, last_outputs=True),
        dict(pairs=True, mask=not can_unmask, outputs=True),
    ]
    for i, r in enumerate(runs):
        r = dict(r)
        mask, outputs, last = r.pop("mask"), r.pop("outputs"), r.pop("last_outputs", False)
        rt = ks.WIDE if r.get("pairs") else route
        g, P, O, lasts = run_batched(gpu, topo, recs, cuts_for(rng, T, nolearn), nolearn, rt, mask=mask,
                                     outputs=outputs, last_outputs=last, **r)
        check(g, topo, refs, P, O, lasts, (cid, i))
        if i == 0:
            check_reference(g, topo, T, seed, kw, nolearn, P, O)
        g.close()


@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("stock_pow2")])
def test_stock_route_other_pow2_tables(gpu, oracle, cid):
    """Power-of-two tables that are not the reference's: Predict + Learn with probabilities only is the
    kernel's compile-time `plain` build (rows through LDS and lane-private), with its tables, rates and skip."""
    topo, route, T, seed, kw, nolearn, refs, recs, rng = setup(oracle, cid)
    assert all(t & (t - 1) == 0 for _, t, _ in topo.mixers)
    for staged in (0, 1):
        g, P, O, _ = run_batched(gpu, topo, recs, cuts_for(rng, T, nolearn), nolearn, route, mask=True,
                                 outputs=False, staged=staged)
        check(g, topo, refs, P, O, [], (cid, staged))
        g.close()
    g, P, O, _ = run_batched(gpu, topo, recs, cuts_for(rng, T, nolearn), nolearn, route)
    check(g, topo, refs, P, O, [], cid)
    check_reference(g, topo, T, seed, kw, nolearn, P, O)
    g.close()


@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("wide")])
def test_wide_route(gpu, oracle, cid):
    topo, route, T, seed, kw, nolearn, refs, recs, rng = setup(oracle, cid)
    g, P, O, _ = run_batched(gpu, topo, recs, cuts_for(rng, T, nolearn), nolearn, route)
    check(g, topo, refs, P, O, [], cid)
    check_reference(g, topo, T, seed, kw, nolearn, P, O)
    g.close()
    g, P, O, _ = run_batched(gpu, topo, recs, cuts_for(rng, T, nolearn), nolearn, route,
                             mask=kw.get("zero_mod", 0) != 0, outputs=False)
    check(g, topo, refs, P, O, [], (cid, "p only"))
    g.close()


@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("bank24")])
def test_bank_24_8_1_builds(gpu, oracle, cid):
    """The unrolled 24/8/1 builds with the row-step counters in their own table (only n = 90 / 256 fold them
    into the rows), and the run-time build just outside their stride ranges."""
    topo, route, T, seed, kw, nolearn, refs, recs, rng = setup(oracle, cid)
    for outputs in (True, False):
        g, P, O, lasts = run_batched(gpu, topo, recs, cuts_for(rng, T, nolearn), nolearn, route, outputs=outputs,
                                     last_outputs=not outputs)
        check(g, topo, refs, P, O, lasts, (cid, outputs))
        if outputs:
            check_reference(g, topo, T, seed, kw, nolearn, P, O)
        g.close()


@pytest.mark.parametrize("cid", [c for c in CASES if c.startswith("single")])
@pytest.mark.parametrize("variant", [0, 16, 32])
def test_single_route(gpu, oracle, cid, variant):
    topo, route, T, seed, kw, nolearn, refs, recs, rng = setup(oracle, cid)
    g, P, O, _ = run_batched(gpu, topo, recs, cuts_for(rng, T, nolearn), nolearn, route,
                             mask=kw.get("zero_mod", 0) != 0 or variant == 16, variant=variant)
    check(g, topo, refs, P, O, [], (cid, variant))
    if variant == 0:
        check_reference(g, topo, T, seed, kw, nolearn, P, O)
    g.close()


def test_stock_route_many_streams_auto_staged(gpu, oracle):
    """One launch of 512 streams at the default staging choice (-1: rows through the LDS images from 512
    streams on), non-power-of-two tables kept small so the banks stay small; a sample of streams against the
    oracle."""
    S, T = 512, 96
    topo = ks.topo_24_8_1(90, 5, small=True)
    kw = dict(ctx_mode=0)
    g = gpu.MixerGroup(topo, S)
    assert ks.kernel_kind(g) == ks.STOCK
    b = gpu.Batch(g, T, outputs=False, mask=True)
    recs = {}
    for s in range(S):
        rec = oracle.synth(90, 33, T, seed=90000 + s, **kw)
        b.set_records(s, *rec)
        recs[s] = rec
    cut = 41
    for t0, t1 in ((0, cut), (cut, T)):
        if t0:
            for s in range(S):
                b.set_records(s, *[a[t0:t1] for a in recs[s]])
        b.upload(t1 - t0)
        g.run(b, t1 - t0, learn=True)
        b.download(t1 - t0)
        b.wait()
        if not t0:
            P0 = b.p[:, :cut].copy()
    P = np.concatenate([P0, b.p[:, :T - cut]], axis=1)
    for s in (0, 1, 63, 64, 255, 300, 510, 511):
        ob = oracle.Bank(90, topo.skip, topo.mixers)
        p_ref, _ = ob.run(*recs[s])
        assert np.array_equal(u32(P[s]), u32(p_ref)), s
        assert g.export(s) == (ob.export_long(), ob.export_short()), s
    b.close()
    g.close()
