"""The analysis averages on the device (gmx_analysis, include/gmxmix_analysis.h) against the checker -- gmx_analysis.h
built for the host (tests/analysis_common.py), never a machine's libm -- and against the fixture recorded from the
reference's own Predictor with analysis on (tests/golden/analysis_trace.npz).  Every comparison is of bit patterns.

The kernel works in tiles of 64 bits and blocks of 64 columns: the counts straddle the tile, C = 70 and C = 124 take a
second block of columns with 6 and 60 live lanes."""
import numpy as np
import pytest

import analysis_common as ac
from gmix_amd import GmxError, topology

pytestmark = pytest.mark.gpu
TILE = ac.TILE
f32 = np.float32


def same(got, streams, what=""):
    """A take's result against the checker's streams (which it takes, too)."""
    for s, st in enumerate(streams):
        ema, seen, rows, labels = st.take()
        g_ema, g_seen, g_rows, g_labels = got[s]
        assert g_seen == seen, (what, "bits_seen", s, g_seen, seen)
        assert np.array_equal(ac.u64(g_ema), ac.u64(ema)), (what, "ema", s, np.argwhere(ac.u64(g_ema) != ac.u64(ema))[:4])
        assert list(g_labels) == list(labels), (what, "labels", s, list(g_labels)[:8], list(labels)[:8])
        assert g_rows.shape == rows.shape and np.array_equal(ac.u64(g_rows), ac.u64(rows)), (what, "rows", s)


def seeded(n_streams, n_bits, n_columns, seed, prob_columns=()):
    """values [S][T][C]: logits of every size, probabilities (some outside [0, 1]) in prob_columns; bits [S][T]."""
    rng = np.random.default_rng(seed)
    scale = rng.choice(np.array([0.05, 1.0, 3.0, 8.0, 40.0], f32), (n_streams, n_bits, n_columns))
    v = (rng.standard_normal((n_streams, n_bits, n_columns)).astype(f32) * scale).astype(f32)
    for c in prob_columns:
        v[:, :, c] = rng.uniform(-0.05, 1.05, (n_streams, n_bits)).astype(f32)
    return v, rng.integers(0, 2, (n_streams, n_bits)).astype(np.uint8)


def plain_columns(n_columns, prob_columns=()):
    return [(ac.FINAL_P, 0) if c in prob_columns else (ac.INPUT, c) for c in range(n_columns)]


def checkers(n_streams, n_columns, prob_columns=(), **kw):
    is_prob = np.array([c in prob_columns for c in range(n_columns)], np.uint8)
    return [ac.Stream(n_columns, is_prob, **kw) for _ in range(n_streams)]


def feed(an, streams, v, bits, n):
    an.update(v, bits, n)
    for s, st in enumerate(streams):
        st.run(v[s, :int(n[s])], bits[s, :int(n[s])])


# ---- the fixture through the chain ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def english(gpu):
    """The stock 24/8/1 group, S = 3, every stream on the fixture's records, run once (learning); the batch's device
    arrays stay as the run left them."""
    t = ac.fixture()
    pred, act = t["english_pred"].view(f32), t["english_act"]
    n = len(t["english_bits"])
    g = gpu.MixerGroup(topology.stock(), 3)
    b = gpu.Batch(g, n, outputs=True, mask=True)
    for s in range(3):
        b.set_records(s, pred, act, t["english_ctx"], t["english_bits"])
    b.upload()
    g.run(b)
    b.download()
    b.wait()
    yield t, g, b, n
    b.close()
    g.close()


def test_the_run_reproduces_the_fixture(english):
    t, _, b, n = english
    for s in range(3):
        assert np.array_equal(b.p[s].view(np.uint32), t["english_p"]), s
        assert np.array_equal(b.outputs[s].view(np.uint32), t["english_out"]), s


@pytest.mark.parametrize("case", ["english", "all_columns"])
def test_fixture_through_the_chain(gpu, english, case):
    t, _, b, n = english
    cols = ac.stock_columns(t[case + "_cols"])
    if case == "all_columns":
        cols.append((ac.FINAL_P, 0))            # C = 124; the last two columns are the final mixer twice
    C = len(cols)
    an = gpu.Analysis(3, cols, n)
    try:
        an.reset(-1, np.full(C, ac.START), 0)
        an.set_frequency(1)
        an.update_batch(b, n)
        got = an.take()
    finally:
        an.close()
    kept, want = t[case + "_kept"], t[case + "_ema"]
    k = len(t[case + "_cols"])
    for s in range(3):
        ema, seen, rows, labels = got[s]
        assert seen == n and list(labels) == [int(v) for v in t["english_seen"][1:]], s
        # the row labelled bits_seen = t holds the averages after bit t (none at bit 0, where bits_seen is 0)
        assert np.array_equal(ac.u64(rows[kept[1:] - 1, :k]), want[1:]), (s, case)
        assert np.array_equal(ac.u64(ema[:k]), want[-1]) and kept[-1] == n - 1
        if case == "all_columns":
            assert np.array_equal(ac.u64(rows[:, C - 1]), ac.u64(rows[:, C - 2])), s
            assert ac.u64(ema[C - 1:])[0] == ac.u64(ema[C - 2:C - 1])[0]
    # ... and the first bit's averages, which no row holds, through a run of one bit
    an = gpu.Analysis(3, cols, 0)
    try:
        an.reset(-1, np.full(C, ac.START), 0)
        an.update_batch(b, 1)
        got = an.take()
    finally:
        an.close()
    for s in range(3):
        assert np.array_equal(ac.u64(got[s][0][:k]), want[0]) and got[s][1] == 1 and len(got[s][3]) == 0


# ---- host arrays ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 70])
def test_operands(gpu, C):
    t = ac.fixture()
    x, xb = t["operands_x"].view(f32), t["operands_bits"]
    T = len(x)
    prob = (C - 1,)
    v, bits = seeded(5, T, C, 41, prob)
    for c in range(C - 1):
        v[0, :, c] = np.roll(x, c)
    bits[0] = xb
    n = np.array([T, 777, 1, 0, 300], np.uint64)
    an = gpu.Analysis(5, plain_columns(C, prob), 0)
    exp = checkers(5, C, prob)
    try:
        feed(an, exp, v, bits, n)
        got = an.take()
        assert np.array_equal(ac.u64(got[0][0][:1]), t["operands_chain"][-1:])   # the reference's own running chain
        assert got[3][1] == 0 and not got[3][0].any()
        same(got, exp)
    finally:
        an.close()


COUNTS = np.array([0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 200], np.uint64)


@pytest.mark.parametrize("between", [False, True], ids=["one-round", "take-between"])
@pytest.mark.parametrize("cuts", [(), (37,), (TILE, 100)], ids=str)
def test_counts_and_splits(gpu, cuts, between):
    S, C, T = len(COUNTS), 5, 200
    v, bits = seeded(S, T, C, 7, (4,))
    an = gpu.Analysis(S, plain_columns(C, (4,)), T)
    exp = checkers(S, C, (4,), frequency=7)
    try:
        an.set_frequency(7)
        edges = (0,) + cuts + (T,)
        acc = None
        for a, b in zip(edges[:-1], edges[1:]):
            n = np.clip(COUNTS.astype(np.int64) - a, 0, b - a).astype(np.uint64)
            an.update(v[:, a:b], bits[:, a:b], n)
            if between:
                part = an.take()
                acc = part if acc is None else [(p[0], p[1], np.concatenate([q[2], p[2]]), np.concatenate([q[3], p[3]]))
                                                for q, p in zip(acc, part)]
        if not between:
            acc = an.take()
        for s, st in enumerate(exp):            # the checker: one call
            st.run(v[s, :int(COUNTS[s])], bits[s, :int(COUNTS[s])])
        assert acc[0][1] == 0 and not acc[0][0].any() and len(acc[0][3]) == 0   # the stream that sat every call out
        assert [len(a[3]) for a in acc] == [int(max(int(c) - 1, 0)) // 7 for c in COUNTS]
        same(acc, exp, str(cuts))
    finally:
        an.close()


def test_samples(gpu):
    S, C, T = 6, 3, 150
    freq = [1, 7, TILE, 1000, 7, 1]
    v, bits = seeded(S, T, C, 9)
    an = gpu.Analysis(S, plain_columns(C), T)
    exp = checkers(S, C)
    try:
        for s, f in enumerate(freq):
            an.set_frequency(f, s)
            exp[s].F = f
        an.reset(4, None, 6)                    # bits_seen = 6, F = 7: captures at its second bit
        exp[4].bits_seen = 6
        n = np.full(S, 2, np.uint64)
        feed(an, exp, v, bits, n)
        got = an.take()
        assert [list(g[3]) for g in got] == [[1], [], [], [], [7], [1]]          # F = 1, bits_seen = 0: nothing at bit 0
        same(got, exp, "two bits")
        n[:] = T
        feed(an, exp, v, bits, n)
        got = an.take()
        assert [len(g[3]) for g in got] == [T, (T + 1) // 7, (T + 1) // TILE, 0, (T + 8 - 1) // 7 - 1, T]
        assert list(got[2][3]) == [TILE, 2 * TILE] and list(got[4][3])[:2] == [14, 21]
        same(got, exp, "whole run")
    finally:
        an.close()


def test_rows_capacity(gpu):
    S, C = 2, 3
    v, bits = seeded(S, 40, C, 10)
    an = gpu.Analysis(S, plain_columns(C), 10)
    exp = checkers(S, C, frequency=1)
    try:
        an.set_frequency(1)
        n = np.array([11, 5], np.uint64)        # bits_seen 0..10: ten rows, the area is full
        feed(an, exp, v, bits, n)
        one = np.array([1, 0], np.uint64)
        with pytest.raises(GmxError) as ei:
            an.update(v, bits, one)
        assert ei.value.status == -1
        with pytest.raises(GmxError):
            an.update(v, bits, np.array([0, 30], np.uint64))
        same(an.take(), exp, "after the refusals")   # nothing changed
        feed(an, exp, v[:, 11:], bits[:, 11:], np.array([10, 10], np.uint64))   # after a take there is room again
        same(an.take(), exp, "next round")
    finally:
        an.close()


def test_state(gpu):
    S, C, T = 3, 70, 180
    v, bits = seeded(S, T, C, 11, (69,))
    start = np.random.default_rng(12).standard_normal(C) - 1.0
    an = gpu.Analysis(S, plain_columns(C, (69,)), T)
    exp = checkers(S, C, (69,), frequency=5)
    try:
        an.set_frequency(5)
        an.reset(-1, start, 1000)
        for st in exp:
            st.ema[:] = start
            st.bits_seen = 1000
        n = np.full(S, 100, np.uint64)
        feed(an, exp, v, bits, n)
        got = an.take()
        assert list(got[0][3])[:2] == [1000, 1005]
        same(got, exp, "from given averages")
        # take -> reset(ema, bits_seen) -> continue equals the uninterrupted run; stream 1 is reset to zeros instead
        for s in (0, 2):
            an.reset(s, got[s][0], got[s][1])
        an.reset(1, None, 0)
        exp[1].ema[:] = 0
        exp[1].bits_seen = 0
        feed(an, exp, v[:, 100:], bits[:, 100:], np.full(S, T - 100, np.uint64))
        same(an.take(), exp, "continued")
    finally:
        an.close()


# ---- from batches of other shapes -----------------------------------------------------------------------------------
GENERAL = topology.Topology(40, [(0, 64, 0.004)] * 5 + [(1, 16, 0.003)] * 3 + [(2, 1, 0.0005)], skip=(1,))


def fill(oracle, batch, topo, n_streams, n_bits, seed):
    recs = []
    for s in range(n_streams):
        rec = oracle.synth(topo.n_inputs, topo.n_mixers, n_bits, seed=seed + s, ctx_mode=3, ctx_mod=6, zero_mod=8, bit_mode=1)
        batch.set_records(s, *rec)
        recs.append(rec)
    return recs


def test_single_mixer_batch_without_a_mask(gpu, oracle):
    topo, S, T = topology.single(256), 4, 130
    cols = [(ac.INPUT, 0), (ac.INPUT, 5), (ac.INPUT, 255), (ac.MIXER, 0), (ac.FINAL_P, 0)]
    g = gpu.MixerGroup(topo, S)
    b = gpu.Batch(g, T, outputs=True, mask=False)
    an = gpu.Analysis(S, cols, T)
    exp = checkers(S, len(cols), (4,), frequency=TILE)
    try:
        assert b.n_pad == 256
        an.set_frequency(TILE)
        first = fill(oracle, b, topo, S, T, 600)
        b.upload()
        b.wait()                                # (the host array is the upload's source: it is rewritten below)
        g.run(b)
        an.update_batch(b, T)
        second = fill(oracle, b, topo, S, T, 700)   # the same batch again, behind the update, without a host wait
        b.upload()
        g.run(b)
        n2 = np.array([T, 0, 77, TILE + 1], np.uint64)
        an.update_batch(b, n2)
        got = an.take()
        for s in range(S):
            ob = oracle.Bank(topo.n_inputs, topo.skip, topo.mixers)
            for (pred, act, ctx, bits), k in ((first[s], T), (second[s], int(n2[s]))):
                p, outs = ob.run(pred, act, ctx, bits)
                v, _ = ac.column_values(cols, pred, act, outs, p)   # (without a mask the silent slots were zeroed)
                exp[s].run(v[:k], bits[:k])
        same(got, exp)
    finally:
        an.close()
        b.close()
        g.close()


def test_refusals(gpu, oracle):
    topo, S, T = GENERAL, 3, 64
    g = gpu.MixerGroup(topo, S)
    b = gpu.Batch(g, T, outputs=True, mask=True)
    plain = gpu.Batch(g, T, outputs=False, mask=True)
    cols = [(ac.INPUT, 39), (ac.MIXER, 8), (ac.FINAL_P, 0)]
    made = {
        "streams": gpu.Analysis(S + 1, cols, 8),
        "input": gpu.Analysis(S, [(ac.INPUT, 40)], 8),
        "mixer": gpu.Analysis(S, [(ac.MIXER, 9)], 8),
    }
    an = gpu.Analysis(S, cols, 8)
    exp = checkers(S, len(cols), (2,), frequency=8)
    try:
        recs = fill(oracle, b, topo, S, T, 800)
        for s in range(S):
            plain.set_records(s, *recs[s])
        b.upload()
        plain.upload()
        g.run(b)
        b.download()
        b.wait()
        an.set_frequency(8)
        an.update_batch(b, 40)
        for s in range(S):
            pred, act, _, bits = recs[s]
            v, _ = ac.column_values(cols, pred, act, b.outputs[s], b.p[s])
            exp[s].run(v[:40], bits[:40])
        for name, x in made.items():
            with pytest.raises(GmxError) as ei:
                x.update_batch(b, 1)
            assert ei.value.status == -1, name
        with pytest.raises(GmxError):
            an.update_batch(b, T + 1)                        # beyond the batch's max_bits
        with pytest.raises(GmxError):
            an.update_batch(plain, 1)                        # a MIXER column, a batch without outputs
        with pytest.raises(GmxError):
            an.update_batch(b, np.array([0, 0, T], np.uint64))   # 40 + 64 bits at F = 8: rows beyond the 8 of the area
        with pytest.raises(GmxError):
            an.update(np.zeros((S, 4, 3), f32), np.zeros((S, 4), np.uint8), 5)   # a count beyond the pitch
        if gpu.device_count() > 1:
            other = gpu.Analysis(S, cols, 8, device=1)
            try:
                with pytest.raises(GmxError):
                    other.update_batch(b, 1)
            finally:
                other.close()
        with pytest.raises(GmxError):
            gpu.Analysis(S, [(3, 0)], 8)                     # no such kind
        with pytest.raises(GmxError):
            gpu.Analysis(S, [(ac.INPUT, 0)] * 513, 8)
        g.close()                                            # the batch is a shell from now on
        with pytest.raises(GmxError) as ei:
            an.update_batch(b, 1)
        assert ei.value.status == -1
        same(an.take(), exp, "after every refusal")          # the averages of the one accepted call
        for name, x in made.items():
            got = x.take()
            assert all(not e.any() and seen == 0 and len(lab) == 0 for e, seen, _, lab in got), name
    finally:
        for x in list(made.values()) + [an]:
            x.close()
        plain.close()
        b.close()
        g.close()


def test_what_crosses_the_link(gpu):
    S, C = 5, 70
    v, bits = seeded(S, 600, C, 13)
    an = gpu.Analysis(S, plain_columns(C), 64)
    try:
        sizes = []
        for n_bits in (100, 600):               # it does not depend on the bits given
            an.update(v, bits, n_bits)
            an.take()
            sizes.append(an.d2h_bytes())
        assert sizes == [16 * S + 8 * C * S] * 2
        an.reset(-1, None, 0)
        for s in range(S):
            an.set_frequency(10 * (s + 1), s)
        an.update(v, bits, 600)
        got = an.take()
        rows = [len(g[3]) for g in got]
        assert rows == [599 // (10 * (s + 1)) for s in range(S)]
        assert an.d2h_bytes() == 16 * S + sum(8 * C + 8 * (C + 1) * r for r in rows)
        assert an.d2h_bytes() * 5 < S * 600 * (4 * C + 5)   # far below the values and bits themselves
    finally:
        an.close()
