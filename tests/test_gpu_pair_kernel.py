"""The opt-in register-resident kernel for any three-layer bank (gmx_pair.hip, MixerGroup.set_register_rows) on
pair_shapes' set: each case asserts its route through gmx_debug_kernel_kind, runs launches cut at random places
plus a forward-only tail, and compares p, outputs, export() and memory_usage with the oracle as bit patterns --
and with the reference's own Mixer where oracle/_ref was built (tests/test_oracle_pair_shapes.py pins the oracle
to it on the same shapes).  Then the mask / outputs / last-outputs variants, ragged runs, switching between this
kernel, the general kernel and the per-bit path on the same banks, the two specialised shapes through it, one
launch at scale, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import goldenlib
import kernel_shapes as ks
import pair_shapes
from gmix_amd import topology
from kernel_shapes import u32

pytestmark = pytest.mark.gpu

CASES = pair_shapes.cases()
PAIR = pair_shapes.PAIR


def group(gpu, topo, S):
    g = gpu.MixerGroup(topo, S)
    before = ks.kernel_kind(g)
    g.set_register_rows(True)
    assert ks.kernel_kind(g) == PAIR, (ks.kernel_kind(g), before, topo.n_inputs)
    assert ks.kernel_kind(g, ks.MODE_PREDICT) == PAIR
    return g


def cuts_for(rng, T, nolearn):
    c = {0, T} | set(rng.integers(1, T, size=2).tolist())
    if nolearn is not None:
        c.add(nolearn)
    return sorted(c)


def run_cuts(gpu, g, topo, recs, cuts, nolearn, mask=True, outputs=True, last_outputs=False, before_launch=None):
    S, T, M = len(recs), len(recs[0][3]), topo.n_mixers
    b = gpu.Batch(g, max(b - a for a, b in zip(cuts, cuts[1:])), outputs=outputs, mask=mask, last_outputs=last_outputs)
    P = np.zeros((S, T), np.float32)
    O = np.zeros((S, T, M), np.float32) if outputs else None
    lasts = []
    for k, (t0, t1) in enumerate(zip(cuts, cuts[1:])):
        n = t1 - t0
        for s, (pred, act, ctx, bits) in enumerate(recs):
            b.set_records(s, pred[t0:t1], act[t0:t1], ctx[t0:t1], bits[t0:t1])
        b.upload(n)
        if before_launch:
            before_launch(k)
        g.run(b, n, learn=nolearn is None or t1 <= nolearn)
        b.download(n)
        b.wait()
        P[:, t0:t1] = b.p[:, :n]
        if outputs:
            O[:, t0:t1] = b.outputs[:, :n]
        if last_outputs:
            lasts.append((t1 - 1, b.last_outputs.copy()))
    b.close()
    return P, O, lasts


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


def setup(oracle, cid, S=3):
    mk, T, seed, kw, nolearn = CASES[cid]
    topo = mk()
    seeds = [seed + 1000 * k for k in range(S)]
    refs = [ks.oracle_run(oracle, topo, T, sd, kw, nolearn) for sd in seeds]
    return topo, T, seed, kw, nolearn, refs, [r[3] for r in refs], np.random.default_rng(seed)


def test_shape_set_covers_what_it_claims():
    ns = {n for n, _, _ in pair_shapes.SHAPES}
    assert ns >= {4, 5, 6, 7, 33, 89, 90, 91, 92, 93, 127, 128, 129, 200, 255, 256, 39, 40, 103, 104, 167, 168}
    assert {l0 for _, l0, _ in pair_shapes.SHAPES} >= {1, 2, 7, 23, 24}
    assert {l1 for _, _, l1 in pair_shapes.SHAPES} >= {1, 3, 8}
    assert len(CASES) >= 24
    topos = [mk() for mk, *_ in CASES.values()]
    assert {(t.skip[0] == 0, t.skip[0] == 1, t.skip[0] == t.n_inputs - 1) for t in topos} >= \
        {(True, False, False), (False, True, False), (False, False, True), (False, False, False)}
    assert any(all(x & (x - 1) == 0 for _, x, _ in t.mixers) for t in topos)
    assert any(any(x & (x - 1) for _, x, _ in t.mixers) for t in topos)


@pytest.mark.parametrize("cid", list(CASES))
def test_pair_kernel_equals_oracle(gpu, oracle, cid):
    topo, T, seed, kw, nolearn, refs, recs, rng = setup(oracle, cid)
    g = group(gpu, topo, 3)
    P, O, _ = run_cuts(gpu, g, topo, recs, cuts_for(rng, T, nolearn), nolearn)
    check(g, topo, refs, P, O, [], cid)
    if ks.have_reference():
        d = ks.reference_run(topo, T, seed, kw, T, nolearn)
        assert np.array_equal(u32(P[0]), u32(d["p"]))
        assert np.array_equal(u32(O[0]), u32(d["outs"]))
        assert g.export(0) == (d["long"], d["short"])
        assert [g.memory_usage(j, stream=0) for j in range(topo.n_mixers)] == [int(x) for x in d["mem"]]
    g.close()


@pytest.mark.parametrize("cid", list(CASES)[::3])
def test_mask_outputs_and_last_outputs(gpu, oracle, cid):
    """Mask on / off (off only where no input goes silent: without a mask a silent slot reads 0, not its stale
    value), outputs on / off, the outputs of each launch's last bit."""
    topo, T, seed, kw, nolearn, refs, recs, rng = setup(oracle, cid)
    can_unmask = kw.get("zero_mod", 0) == 0
    for i, (mask, outputs, last) in enumerate([(not can_unmask, False, True), (True, False, False),
                                               (not can_unmask, True, True)]):
        g = gpu.MixerGroup(topo, 3)
        if i == 0:   # the batch asks for the last outputs BEFORE the switch is set
            b0 = gpu.Batch(g, 8, outputs=False, mask=True, last_outputs=True)
            b0.close()
        g.set_register_rows(True)
        assert ks.kernel_kind(g) == PAIR
        P, O, lasts = run_cuts(gpu, g, topo, recs, cuts_for(rng, T, nolearn), nolearn, mask=mask, outputs=outputs,
                               last_outputs=last)
        check(g, topo, refs, P, O, lasts, (cid, i))
        g.close()


@pytest.mark.parametrize("cid", [list(CASES)[k] for k in (0, 6, 9, 15, 21)])
def test_ragged(gpu, oracle, cid):
    """Five streams with 0, 1, 17, T/2 and T bits in one run_ragged; then all of them go on together."""
    mk, _, seed, kw, _ = CASES[cid]
    topo = mk()
    n, m, T = topo.n_inputs, topo.n_mixers, 200
    counts = [0, 1, 17, T // 2, T]
    g = group(gpu, topo, 5)
    b = gpu.Batch(g, T, outputs=True, mask=True)
    bl = gpu.Batch(g, T, outputs=False, mask=True, last_outputs=True)
    banks = [oracle.Bank(n, topo.skip, topo.mixers) for _ in counts]
    for rnd, cnt in enumerate([counts, counts[::-1], [T] * 5]):
        want = []
        for s, k in enumerate(cnt):
            rec = oracle.synth(n, m, T, seed=seed + 100 * rnd + s, **kw)
            (bl if rnd == 1 else b).set_records(s, *rec)
            want.append(banks[s].run(*[a[:k] for a in rec]) if k else None)
        bb = bl if rnd == 1 else b
        bb.upload(T)
        g.run_ragged(bb, cnt)
        bb.download(T)
        bb.wait()
        for s, k in enumerate(cnt):
            if not k:
                continue
            assert np.array_equal(u32(bb.p[s, :k]), u32(want[s][0])), (cid, rnd, s)
            if rnd == 1:
                assert np.array_equal(u32(bb.last_outputs[s]), u32(want[s][1][k - 1])), (cid, rnd, s)
            else:
                assert np.array_equal(u32(bb.outputs[s, :k]), u32(want[s][1])), (cid, rnd, s)
    for s in range(5):
        assert g.export(s) == (banks[s].export_long(), banks[s].export_short()), (cid, s)
    b.close()
    bl.close()
    g.close()


@pytest.mark.parametrize("cid", [list(CASES)[k] for k in (4, 6, 12, 15, 19)])
def test_switching_kernels_on_the_same_banks(gpu, oracle, cid):
    """Launch 1 through this kernel, launch 2 through the general kernel, launch 3 through this kernel, then a
    stretch bit by bit through gmx_bank_forward / gmx_bank_learn: the layouts are everybody's."""
    mk, _, seed, kw, _ = CASES[cid]
    topo = mk()
    T, per_bit = 330, 24
    refs = [ks.oracle_run(oracle, topo, T + per_bit, seed + 1000 * k, kw) for k in range(2)]
    recs = [tuple(a[:T] for a in r[3]) for r in refs]
    g = gpu.MixerGroup(topo, 2)
    default = ks.kernel_kind(g)

    def flip(k):
        g.set_register_rows(k != 1)
        assert ks.kernel_kind(g) == (PAIR if k != 1 else default)
    P, O, _ = run_cuts(gpu, g, topo, recs, [0, 120, 210, T], None, before_launch=flip)
    for s, (ob, p_ref, o_ref, rec) in enumerate(refs):
        assert np.array_equal(u32(P[s]), u32(p_ref[:T])), (cid, s)
        assert np.array_equal(u32(O[s]), u32(o_ref[:T])), (cid, s)
        pred, act, ctx, bits = rec
        for t in range(T, T + per_bit):
            p, outs = g.forward(pred[t], np.flatnonzero(act[t]), ctx[t], stream=s)
            assert np.float32(p).view(np.uint32) == u32(p_ref[t:t + 1])[0], (cid, s, t)
            assert np.array_equal(u32(outs), u32(o_ref[t])), (cid, s, t)
            g.learn(int(bits[t]), stream=s)
        assert g.export(s) == (ob.export_long(), ob.export_short()), (cid, s)
    g.close()


@pytest.mark.parametrize("shape", ["stock90", "n256"])
def test_specialised_shapes_through_the_family_kernel(gpu, oracle, shape):
    """stock(90) and 256 x 24/8/1 with the switch on equal the same streams with it off."""
    topo = topology.stock(90) if shape == "stock90" else topology.synth3(256)
    T, kw = 500, ks.pattern(3 if shape == "stock90" else 2)
    refs = [ks.oracle_run(oracle, topo, T, 4100 + k, kw) for k in range(3)]
    recs = [r[3] for r in refs]
    res = []
    for on in (False, True):
        g = gpu.MixerGroup(topo, 3)
        assert ks.kernel_kind(g) == (ks.STOCK if shape == "stock90" else ks.WIDE)
        if on:
            g.set_register_rows(True)
            assert ks.kernel_kind(g) == PAIR
        P, O, _ = run_cuts(gpu, g, topo, recs, [0, 133, 401, T], None)
        res.append((u32(P).copy(), u32(O).copy(), [g.export(s) for s in range(3)]))
        if on:
            check(g, topo, refs, P, O, [], shape)
        g.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


@pytest.mark.parametrize("name", ["stock90_learnable", "a3_synth3_n256"])
def test_goldens_replay_through_the_family_kernel(gpu, oracle, name):
    """The reference's recorded vectors of the two specialised shapes, through this kernel."""
    meta, z = goldenlib.load(name)
    topo = goldenlib.topo_of(meta)
    kw, nolearn = goldenlib.synth_kwargs(meta)
    assert nolearn is None
    T, chunk = meta["T"], 20000
    st = oracle.Stream(topo.n_inputs, topo.n_mixers, **kw)
    g = group(gpu, topo, 1)
    b = gpu.Batch(g, min(chunk, T), outputs=True, mask=True)
    h, outs_d, p_d = 0, [], []
    for t0 in range(0, T, chunk):
        n = min(chunk, T - t0)
        b.set_records(0, *st.next(n))
        b.upload(n)
        g.run(b, n, learn=True)
        b.download(n)
        b.wait()
        h = oracle.fnv64(b.outputs[0, :n], b.p[0, :n], h0=h)
        if t0 < meta["dump"]:
            outs_d.append(b.outputs[0, :n].copy())
            p_d.append(b.p[0, :n].copy())
    assert h == meta["h64"], name
    d = meta["dump"]
    if d:
        assert np.array_equal(np.concatenate(outs_d)[:d].view(np.uint32), z["outs"])
        assert np.array_equal(np.concatenate(p_d)[:d].view(np.uint32), z["p"])
    lb, sb = g.export(0)
    assert sb.hex() == meta["short_hex"]
    assert len(lb) == meta["long_len"] and goldenlib.sha256(lb) == meta["long_sha256"]
    assert [g.memory_usage(j) for j in range(len(meta["mixers"]))] == list(z["mem"])
    b.close()
    g.close()


def test_one_launch_at_scale(gpu, oracle):
    """1 024 streams x 256 bits of a 128-input 24/8/1 bank with small tables in one launch: every CU, as many
    waves per SIMD as the kernel gets; a sample of eight streams against the oracle."""
    S, T = 1024, 256
    topo = pair_shapes.scale_topology()
    kw = dict(ctx_mode=0)
    g = group(gpu, topo, S)
    b = gpu.Batch(g, T, outputs=False, mask=True)
    recs = {}
    for s in range(S):
        recs[s] = oracle.synth(128, 33, T, seed=70000 + s, **kw)
        b.set_records(s, *recs[s])
    b.upload(T)
    g.run(b, T, learn=True)
    b.download(T)
    b.wait()
    for s in (0, 1, 63, 64, 255, 511, 1022, 1023):
        ob = oracle.Bank(128, topo.skip, topo.mixers)
        p_ref, _ = ob.run(*recs[s])
        assert np.array_equal(u32(b.p[s, :T]), u32(p_ref)), s
        assert g.export(s) == (ob.export_long(), ob.export_short()), s
    b.close()
    g.close()


@pytest.mark.parametrize("what", ["single", "l0=25"])
def test_refusal(gpu, what):
    topo = topology.single(64, 256, 0.005) if what == "single" else \
        topology.Topology(90, [(0, 8, .01)] * 25 + [(1, 5, .01)] * 8 + [(2, 3, .01)], skip=(1,))
    assert not gpu.bank.register_rows_eligible(topo)
    g = gpu.MixerGroup(topo, 2)
    before = ks.kernel_kind(g)
    g.L.gmx_group_set_register_rows.argtypes = [C.c_void_p, C.c_int]
    assert g.L.gmx_group_set_register_rows(g.h, 1) == -1
    with pytest.raises(gpu.GmxError):
        g.set_register_rows(True)
    assert ks.kernel_kind(g) == before and before != PAIR
    g.close()
