"""gmx_ctx_run's targets: the stock context bank writes the gate contexts of the mixers' records and the contexts,
bit_contexts and bits of the Indirect and the Match models' records on the device, and the existing chain
(Match -> Indirect models -> mixers) behind it computes what it computes from records the host filled from
tests/helpers/ctx_ref.c.  Stock shape, 2 streams x 130 bytes.  Tolerance 0: everything is compared as bit patterns.

The batches' context columns cannot be downloaded, so "the unrouted columns still hold what the host put there" is
checked through what reads them: column 22 of the mixers and column 16 of the Indirect models carry a fixed pattern
standing for lstm_prediction_context in both runs, and 0xFFFFFFFF anywhere in them would change the mixers' rows and the
Indirect models' table entries; columns 6 and 30 are gmx_match_run's."""
import numpy as np
import pytest

import ctx_common as cc
import goldenlib
from gmix_amd import GmxError, topology

pytestmark = pytest.mark.gpu

GMX_ERR_INVALID = -1
S, NBYTES = 2, 130
T = 8 * NBYTES
OFFSETS = (0, 700)     # where in ctx_stock's data each stream begins
FILL = 0xFFFFFFFF
_cache = {}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stock():
    if "stock" not in _cache:
        descs, mixer_route, ind_route, match_route = topology.stock_contexts()
        f = cc.fixture("ctx_stock")
        assert [d[0] for d in descs] == f.names
        vals = []
        for o in OFFSETS:
            v = cc.Ref(f.descs).run(f.bits[8 * o:8 * o + T])
            v.setflags(write=False)
            vals.append(v)
        rng = np.random.default_rng(17)
        pred = (rng.standard_normal((S, T, 90)) * 2).astype(np.float32)
        act = (rng.integers(0, 4, (S, T, 90)) != 0).astype(np.uint8)
        lstm_ctx = ((np.arange(T) // 8) * 37 % 256).astype(np.uint32)   # stands for lstm_prediction_context
        _cache["stock"] = dict(f=f, descs=descs, mr=np.array(mixer_route), ir=np.array(ind_route),
                               xr=np.array(match_route), vals=vals, pred=pred, act=act, lstm_ctx=lstm_ctx)
    return _cache["stock"]


class Chain:
    """The three downstream banks of the stock shape and n_sets sets of their batches."""

    def __init__(self, gpu, max_bits, n_sets=1, with_ctx=False):
        st = stock()
        _, z = goldenlib.load("ind_stock41")
        islots = [(2 + 2 * i, 3 + 2 * i) for i in range(32)] + [(72 + 2 * j, 73 + 2 * j) for j in range(9)]
        self.topo = topology.stock(90)
        self.mg = gpu.MixerGroup(self.topo, S)
        self.ig = gpu.IndirectGroup(topology.stock_indirect(), z["ns_next"], z["rm_next"], S, slots=islots)
        self.xg = gpu.MatchGroup(topology.stock_match(), NBYTES + 64, S)
        self.cg = gpu.CtxGroup(st["descs"], S) if with_ctx else None
        self.dev_slots = list(topology.STOCK_MATCH_SLOTS) + [i for ab in islots for i in ab]
        self.sets = []
        for _ in range(n_sets):
            self.sets.append(dict(mb=gpu.Batch(self.mg, max_bits, outputs=True, mask=True),
                                  ib=gpu.IndirectBatch(self.ig, max_bits), xb=gpu.MatchBatch(self.xg, max_bits),
                                  cb=gpu.CtxBatch(self.cg, max_bits, values=False) if with_ctx else None))

    def fill(self, k, t0, n, from_ref):
        """Host records of bits [t0, t0 + n) into set k: the contexts from ctx_ref.c, or FILL wherever gmx_ctx_run is
        to write."""
        st, bs = stock(), self.sets[k]
        for s in range(S):
            f = st["f"]
            bits = f.bits[8 * OFFSETS[s] + t0:8 * OFFSETS[s] + t0 + n]
            v = st["vals"][s][t0:t0 + n]
            lstm = st["lstm_ctx"][t0:t0 + n]
            bc = v[:, f.names.index("bit_context")]

            def columns(route, foreign):
                out = np.full((n, len(route)), FILL, np.uint32)
                for c, r in enumerate(route):
                    if r < 0:
                        out[:, c] = foreign
                    elif from_ref:
                        out[:, c] = v[:, r]
                return out
            act = st["act"][s, t0:t0 + n].copy()
            act[:, self.dev_slots] = 0
            # (columns 6 and 30 of the mixers are written by gmx_match_run in both runs: the same pattern under them)
            bs["mb"].set_records(s, st["pred"][s, t0:t0 + n], act, columns(st["mr"], lstm), bits)
            fill1 = np.full(n, FILL, np.uint32)
            bs["ib"].set_records(s, columns(st["ir"], lstm), bc if from_ref else fill1,
                                 bits if from_ref else np.full(n, 0xFF, np.uint8))
            bs["xb"].set_records(s, columns(st["xr"], lstm), bc if from_ref else fill1,
                                 bits if from_ref else np.full(n, 0xFF, np.uint8))
            if bs["cb"] is not None:
                bs["cb"].bits[s, :n] = bits

    def targets(self, k):
        st, bs = stock(), self.sets[k]
        return self.cg.targets(mixers=bs["mb"], mixer_route=st["mr"], indirect=bs["ib"], ind_route=st["ir"],
                               match=bs["xb"], match_route=st["xr"])

    def step(self, k, n, use_ctx):
        bs = self.sets[k]
        for x in ("mb", "ib", "xb"):
            bs[x].upload(n)
        if use_ctx:
            bs["cb"].upload(n)
            self.cg.run(bs["cb"], n, targets=self.targets(k))
        self.xg.run(bs["xb"], n, into=bs["mb"], ctx_columns=topology.stock_longest_match_columns())
        self.ig.run(bs["ib"], n, into=bs["mb"])
        self.mg.run(bs["mb"], n, learn=True)
        bs["mb"].download(n)

    def collect(self, k, n):
        bs = self.sets[k]
        for x in bs.values():   # (every host array of the set may be refilled after this)
            if x is not None:
                x.wait()
        return u32(bs["mb"].p[:, :n]).copy(), u32(bs["mb"].outputs[:, :n]).copy()

    def exports(self):
        return [(self.mg.export(s), self.ig.export(s), self.xg.export(s)) for s in range(S)]

    def close(self):
        for bs in self.sets:
            for x in bs.values():
                if x is not None:
                    x.close()
        for g in (self.mg, self.ig, self.xg, self.cg):
            if g is not None:
                g.close()


def host_run(gpu, chunks):
    """Run A, shared by the cases: the host fills every context from ctx_ref.c, one synchronous step per chunk."""
    key = ("A", tuple(chunks))
    if key not in _cache:
        a = Chain(gpu, max(chunks))
        res, t0 = [], 0
        for n in chunks:
            a.fill(0, t0, n, from_ref=True)
            a.step(0, n, use_ctx=False)
            res.append(a.collect(0, n))
            t0 += n
        _cache[key] = (res, a.exports())
        a.close()
    return _cache[key]


def test_one_launch_feeds_all_three_batches(gpu):
    (want,), want_exports = host_run(gpu, [T])
    b = Chain(gpu, T, with_ctx=True)
    b.fill(0, 0, T, from_ref=False)
    b.step(0, T, use_ctx=True)
    p, out = b.collect(0, T)
    assert np.array_equal(p, want[0]) and np.array_equal(out, want[1])
    assert b.exports() == want_exports
    st = stock()
    for s in range(S):   # and the bank itself stands where ctx_ref.c stands
        r = cc.Ref(st["f"].descs)
        r.run(st["f"].bits[8 * OFFSETS[s]:8 * OFFSETS[s] + T], values=False)
        assert b.cg.export(s)[0] == r.export()[0] and cc.board_bytes(b.cg.blackboard(s)) == cc.board_bytes(r.board())
    b.close()


def test_three_steps_two_alternating_batch_sets(gpu):
    """Nothing is waited for between a step's launches and the next step's uploads into the other set: the writes of
    gmx_ctx_run are ordered against the targets' own uploads and their owners' kernels by events alone."""
    chunks = [347, 347, 346]   # runs begin and end inside bytes
    want, want_exports = host_run(gpu, chunks)
    b = Chain(gpu, max(chunks), n_sets=2, with_ctx=True)
    got, t0 = [], 0
    for i, n in enumerate(chunks):
        k = i % 2
        if i >= 2:
            got.append(b.collect(k, chunks[i - 2]))   # the set's host arrays are free again
        b.fill(k, t0, n, from_ref=False)
        b.step(k, n, use_ctx=True)
        t0 += n
    got.append(b.collect(1, chunks[1]))
    got.append(b.collect(0, chunks[2]))
    for i in range(3):
        assert np.array_equal(got[i][0], want[i][0]) and np.array_equal(got[i][1], want[i][1]), i
    assert b.exports() == want_exports
    b.close()


def test_targets_are_validated_before_anything_is_queued(gpu):
    st = stock()
    b = Chain(gpu, 64, with_ctx=True)
    bs = b.sets[0]
    before = cc.board_bytes(b.cg.blackboard(0))
    mk = b.cg.targets
    bad = [
        mk(mixers=bs["mb"], mixer_route=st["mr"][:-1]),                       # a route of the wrong length
        mk(indirect=bs["ib"], ind_route=np.append(st["ir"], 0)),
        mk(match=bs["xb"], match_route=np.where(np.arange(6) == 2, 52, st["xr"])),   # an entry == V
        mk(mixers=bs["mb"], mixer_route=np.where(np.arange(33) == 0, -2, st["mr"])),  # an entry below -1
    ]
    for t in bad:
        with pytest.raises(GmxError) as e:
            b.cg.run(bs["cb"], 64, targets=t)
        assert e.value.status == GMX_ERR_INVALID
    small = gpu.MatchBatch(b.xg, 32)                                              # fewer bits than the run
    with pytest.raises(GmxError):
        b.cg.run(bs["cb"], 64, targets=mk(match=small, match_route=st["xr"]))
    one = gpu.MatchGroup(topology.stock_match(), 64, 1)                           # another stream count
    ob = gpu.MatchBatch(one, 64)
    with pytest.raises(GmxError):
        b.cg.run(bs["cb"], 64, targets=mk(match=ob, match_route=st["xr"]))
    assert cc.board_bytes(b.cg.blackboard(0)) == before
    for x in (small, ob, one):
        x.close()
    b.close()
