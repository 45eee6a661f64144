"""The arithmetic encoder on the device (gmx_encoder, include/gmxmix_encoder.h) against PyEncoder, the fixture recorded
from the reference's own Encoder, and oracle.encode on whole outputs.  Every comparison is exact.

S = 70 is two waves of the kernel, the second with six live lanes; the per-stream counts straddle every power-of-two
tile up to 256; the operands are the mixture of tests/encoder_common.py (tests/test_encoder_census.py checks what they
hold)."""
import os

import numpy as np
import pytest

import encoder_common as ec
from gmix_amd import GmxError, topology

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S, T = ec.S, ec.T


class Expect:
    """S PyEncoders driven as the device object is."""

    def __init__(self, n_streams):
        self.e = [ec.PyEncoder() for _ in range(n_streams)]
        self.taken = [0] * n_streams
        self.bad = [-1] * n_streams
        self.coded = [0] * n_streams

    def reset(self, s, state=None):
        self.e[s] = ec.PyEncoder(state)
        self.taken[s], self.bad[s], self.coded[s] = 0, -1, 0

    def encode(self, p, bits, n):
        for s, e in enumerate(self.e):
            if self.bad[s] >= 0:
                continue
            k = int(n[s])
            t = e.run(bits[s, :k], p[s, :k])
            if t >= 0:
                self.bad[s] = self.coded[s] + t
            self.coded[s] += k if t < 0 else t

    def flush(self, which=None):
        for s, e in enumerate(self.e):
            if (which is None or which[s]) and self.bad[s] < 0:
                e.flush()

    def take(self):
        out = [bytes(e.out[self.taken[s]:]) for s, e in enumerate(self.e)]
        self.taken = [len(e.out) for e in self.e]
        return out


def same(enc, exp, got):
    want = exp.take()
    for s in range(len(want)):
        assert got[s] == want[s], ("bytes", s, len(got[s]), len(want[s]))
        assert enc.total_bytes(s) == len(exp.e[s].out), ("total", s)
    for s in range(len(want)):
        assert enc.state(s) == exp.e[s].state, ("state", s)


@pytest.fixture(scope="module")
def operands():
    p, bits, n = ec.gpu_operands()
    for a in (p, bits, n):
        a.setflags(write=False)
    return p, bits, n


@pytest.fixture()
def enc(gpu):
    e = gpu.Encoder(S, T)
    yield e
    e.close()


def full(v=T, n_streams=S):
    return np.full(n_streams, v, np.uint64)


def test_counts_straddle_the_tiles(enc, operands):
    p, bits, n = operands
    exp = Expect(S)
    enc.encode(p, bits, n)
    exp.encode(p, bits, n)
    got = enc.take()
    assert enc.L.gmx_encoder_n_bytes(enc.h, 0) == 0 and got[0] == b"" and got[66] == b""   # count 0 keeps everything
    assert enc.state(0) == (0, ec.M32) and enc.total_bytes(66) == 0
    same(enc, exp, got)
    assert sum(len(g) for g in got) > 0


@pytest.mark.parametrize("between", [False, True], ids=["one-round", "take-between"])
@pytest.mark.parametrize("cuts", [(), (1,), (8,), (64,), (65,), (299,), (100, 229)], ids=str)
def test_splits_concatenate(enc, operands, oracle, cuts, between):
    p, bits, _ = operands
    exp = Expect(S)
    edges = (0,) + tuple(cuts) + (T,)
    got = [b""] * S
    for a, b in zip(edges[:-1], edges[1:]):
        enc.encode(p[:, a:b], bits[:, a:b], full(b - a))
        if between:
            got = [g + t for g, t in zip(got, enc.take())]
    got = [g + t for g, t in zip(got, enc.take())]
    exp.encode(p, bits, full())
    same(enc, exp, got)
    which = np.array([s % 3 == 0 for s in range(S)], np.uint8)
    before = [enc.state(s) for s in range(S)]
    enc.flush(which)
    exp.flush(which)
    tail = enc.take()
    for s in range(S):
        if which[s]:
            assert got[s] + tail[s] == oracle.encode(bits[s], p[s]), s
            assert 1 <= len(tail[s]) <= 5
        else:
            assert tail[s] == b"" and enc.state(s) == before[s], s
    same(enc, exp, tail)


def test_resume_from_recorded_states(enc):
    t = np.load(os.path.join(GOLDEN, "encoder_trace.npz"))
    p = np.zeros((S, T), np.float32)
    bits = np.zeros((S, T), np.uint8)
    n = np.zeros(S, np.uint64)
    # the fixture's resumed run, in one stream of each wave, and its mixture run from the state after bit 999
    rp, rb = t["resumed_p"].view(np.float32), t["resumed_bits"]
    for s in (2, 65):
        enc.reset(s, t["resumed_start"])
        p[s], bits[s], n[s] = rp[:T], rb[:T], T
    mp, mb, ms, mc = t["mixture_p"].view(np.float32), t["mixture_bits"], t["mixture_state"], t["mixture_count"]
    enc.reset(7, ms[999])
    p[7], bits[7], n[7] = mp[1000:1300], mb[1000:1300], 300
    enc.encode(p, bits, n)
    got = enc.take()
    out = t["resumed_output"].tobytes()
    for s in (2, 65):
        assert got[s] == out[:int(t["resumed_count"][T - 1])] and got[s][:4] == out[:4]
        assert enc.state(s) == tuple(int(v) for v in t["resumed_state"][T - 1])
    assert got[7] == t["mixture_output"].tobytes()[int(mc[999]):int(mc[1299])]
    assert enc.state(7) == tuple(int(v) for v in ms[1299])
    assert enc.state(3) == (0, ec.M32) and got[3] == b""
    n[:] = 0
    n[2] = n[65] = 100
    for s in (2, 65):
        p[s, :100], bits[s, :100] = rp[T:], rb[T:]
    enc.encode(p[:, :100], bits[:, :100], n)
    enc.flush(n != 0)
    tail = enc.take()
    assert got[2] + tail[2] == out and got[65] + tail[65] == out and tail[7] == b""


def test_constructed_states_emit_one_to_four_bytes(enc):
    exp = Expect(S)
    for s in range(S):
        enc.reset(s, ec.KIN[s % 4])
        exp.reset(s, ec.KIN[s % 4])
    p = np.full((S, 1), 0.5, np.float32)
    bits = np.ones((S, 1), np.uint8)
    enc.encode(p, bits, full(1))
    exp.encode(p, bits, full(1))
    got = enc.take()
    assert [len(g) for g in got] == [s % 4 + 1 for s in range(S)]
    same(enc, exp, got)


def test_capacity_of_a_round(enc):
    exp = Expect(S)
    p = np.zeros((S, T), np.float32)
    bits = np.ones((S, T), np.uint8)
    enc.encode(p, bits, full())
    exp.encode(p, bits, full())
    got = enc.take()
    assert len(got[0]) >= 2 * (T - 2)          # the densest sustained output: two bytes per bit
    same(enc, exp, got)
    # the four-byte bits one behind the other, a reset in front of each (which discards what was not taken)
    half = p[:, :1] + np.float32(0.5)
    for _ in range(25):
        enc.reset(-1, ec.FOUR)
        for s in range(S):
            exp.reset(s, ec.FOUR)
        enc.encode(half, bits[:, :1], full(1))
        exp.encode(half, bits[:, :1], full(1))
        got = enc.take()
        assert all(len(g) == 4 for g in got)
        assert got == exp.take()
    assert enc.state(0) == exp.e[0].state and enc.state(69) == exp.e[69].state
    # a full round, then one more bit: refused, and nothing changes
    enc.reset(-1)
    exp = Expect(S)
    pm, bm, _ = ec.gpu_operands(seed=12)
    enc.encode(pm, bm, full())
    exp.encode(pm, bm, full())
    one = np.zeros(S, np.uint64)
    one[69] = 1
    with pytest.raises(GmxError) as ei:
        enc.encode(pm, bm, one)
    assert ei.value.status == -1
    same(enc, exp, enc.take())
    enc.encode(pm, bm, one)                     # the next round has room again
    exp.encode(pm, bm, one)
    same(enc, exp, enc.take())


BAD = {"nan": np.float32(np.nan), "minus-zero": np.float32(-0.0), "below": np.float32(-1e-9),
       "above": np.float32(1.0) + np.float32(2.0 ** -23), "inf": np.float32(np.inf)}


@pytest.mark.parametrize("where", [0, 37, T - 1], ids=["first", "mid-tile", "last"])
@pytest.mark.parametrize("what", list(BAD))
def test_bad_p(enc, operands, what, where):
    p, bits, _ = operands
    p = p.copy()
    victims = (5, 66)                           # one stream in each wave
    for s in victims:
        p[s, where] = BAD[what]
    exp = Expect(S)
    enc.encode(p, bits, full())
    exp.encode(p, bits, full())
    if what == "minus-zero":                    # accepted: it is 0
        got = enc.take()
        assert all(enc.bad_bit(s) == -1 for s in range(S))
        same(enc, exp, got)
        return
    with pytest.raises(GmxError) as ei:
        enc.take()
    assert ei.value.status == -1
    got = enc.last_taken
    for s in range(S):
        assert enc.bad_bit(s) == (where if s in victims else -1), s
    same(enc, exp, got)                         # the victims up to the bit before, every other stream whole
    # a later call leaves the bad streams alone until a reset
    enc.encode(p[:, :50], bits[:, :50], full(50))
    exp.encode(p[:, :50], bits[:, :50], full(50))
    with pytest.raises(GmxError):
        enc.take()
    got = enc.last_taken
    assert got[5] == b"" and got[66] == b"" and len(got[4]) > 0 and enc.bad_bit(5) == where
    same(enc, exp, got)
    for s in victims:
        enc.reset(s)
        exp.reset(s)
    enc.encode(p[:, 40:90], bits[:, 40:90], full(50))
    exp.encode(p[:, 40:90], bits[:, 40:90], full(50))
    got = enc.take()
    assert len(got[5]) > 0 and enc.bad_bit(5) == -1 and enc.bad_bit(66) == -1
    same(enc, exp, got)


# ---- from a batch ---------------------------------------------------------------------------------------------------
SHAPES = {
    "general": (topology.Topology(40, [(0, 64, 0.004)] * 5 + [(1, 16, 0.003)] * 3 + [(2, 1, 0.0005)], skip=(1,)), 3, 64),
    "single256": (topology.single(256), 70, 130),
}


def fill(oracle, batch, topo, n_streams, n_bits, seed):
    recs = []
    for s in range(n_streams):
        pred, act, ctx, bits = oracle.synth(topo.n_inputs, topo.n_mixers, n_bits, seed=seed + s, ctx_mode=3, ctx_mod=6,
                                            zero_mod=8, bit_mode=1)
        batch.set_records(s, pred, act, ctx, bits)
        recs.append((pred, act, ctx, bits))
    return recs


@pytest.mark.parametrize("ragged", [False, True], ids=["even", "ragged"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_from_a_batch(gpu, oracle, shape, ragged):
    topo, ns, nb = SHAPES[shape]
    g = gpu.MixerGroup(topo, ns)
    b = gpu.Batch(g, nb)
    e = gpu.Encoder(ns, nb)
    try:
        recs = fill(oracle, b, topo, ns, nb, 100)
        n = full(nb, ns)
        if ragged:
            n = np.random.default_rng(5).integers(0, nb + 1, ns).astype(np.uint64)
            n[0], n[ns - 1] = nb, 0
        b.upload()
        if ragged:
            g.run_ragged(b, n)
        else:
            g.run(b)
        e.encode_batch(b, n if ragged else nb)
        b.download()
        b.wait()
        got = e.take()
        e.flush()
        tail = e.take()
        for s in range(ns):
            k = int(n[s])
            assert got[s] + tail[s] == oracle.encode(recs[s][3][:k], b.p[s, :k]), s
        assert any(len(x) > 1 for x in got)
    finally:
        e.close()
        b.close()
        g.close()


def test_batch_reuse_without_a_host_wait(gpu, oracle):
    topo, ns, nb = SHAPES["general"]
    g = gpu.MixerGroup(topo, ns)
    b = gpu.Batch(g, nb)
    e = gpu.Encoder(ns, 2 * nb)
    try:
        first = fill(oracle, b, topo, ns, nb, 300)
        b.upload()
        b.wait()                                # (the host array is the upload's source: it is rewritten below)
        g.run(b)
        e.encode_batch(b, nb)
        second = fill(oracle, b, topo, ns, nb, 400)
        b.upload()
        g.run(b)
        e.encode_batch(b, nb)
        got = e.take()
        e.flush()
        tail = e.take()
        for s in range(ns):
            ob = oracle.Bank(topo.n_inputs, topo.skip, topo.mixers)
            p1, _ = ob.run(*first[s])
            p2, _ = ob.run(*second[s])
            bits = np.concatenate([first[s][3], second[s][3]])
            assert got[s] + tail[s] == oracle.encode(bits, np.concatenate([p1, p2])), s
    finally:
        e.close()
        b.close()
        g.close()


def test_batch_refusals(gpu, oracle):
    topo, ns, nb = SHAPES["general"]
    g = gpu.MixerGroup(topo, ns)
    b = gpu.Batch(g, nb)
    fill(oracle, b, topo, ns, nb, 500)
    b.upload()
    g.run(b)
    wrong, small, e = gpu.Encoder(ns + 1, nb), gpu.Encoder(ns, nb - 1), gpu.Encoder(ns, 2 * nb)
    try:
        for enc_, n in ((wrong, nb), (small, nb), (e, nb + 1)):
            with pytest.raises(GmxError) as ei:
                enc_.encode_batch(b, n)
            assert ei.value.status == -1
        e.encode_batch(b, nb)
        assert sum(len(x) for x in e.take()) > 0
        g.close()                               # the batch is a shell from now on
        with pytest.raises(GmxError) as ei:
            e.encode_batch(b, 1)
        assert ei.value.status == -1
        assert e.take() == [b""] * ns
    finally:
        for x in (wrong, small, e):
            x.close()
        b.close()
        g.close()


def test_what_crosses_the_link(gpu):
    z = np.load(os.path.join(GOLDEN, "trace_english.npz"))
    bits1, p1 = np.unpackbits(z["bits"]), z["p"].view(np.float32)
    nb = len(bits1)
    e = gpu.Encoder(S, nb)
    try:
        e.encode(np.tile(p1, (S, 1)), np.tile(bits1, (S, 1)), nb)
        e.flush()
        got = e.take()
        d2h = e.d2h_bytes()
        assert all(len(x) == len(got[0]) and len(x) > 100 for x in got)
        assert 0 < d2h <= sum((len(x) + 63) // 64 * 64 for x in got) + 64 * S
        assert d2h < S * (4 * nb + 5)           # not the areas' capacity
        assert d2h * 10 < 5 * nb * S            # far below the 5 bytes per bit that p and bits take
    finally:
        e.close()
