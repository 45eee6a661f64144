"""gmx_indirect_attach_match / gmx_chain_forward_match: the Match models of a stream ride in lanes 56..63 of the
Indirect models' per-bit session wave, which hands everything to the mixers' wave -- one command and one wait per bit.
Expected values: tests/helpers/match_ref.c for the Match models, the oracle's Indirect and mixer banks on the merged
records behind them, bit by bit.  Tolerance 0 everywhere: floats are compared as bit patterns.

Which records a case replays is chosen so that match_ref.c alone reaches the regimes the case is there for; every
case asserts that of its own records before it looks at the device."""
import ctypes as C
import time

import numpy as np
import pytest

import goldenlib
import match_common as mc
from gmix_amd import GmxError, topology
from test_gpu_chainstep_match import IND_MODELS, IND_SLOTS, MSLOTS, ref_stream, u32

pytestmark = pytest.mark.gpu

GMX_ERR_INVALID, GMX_ERR_STATE = -1, -5
STALE = 123.0            # what the caller leaves in the device-side models' slots: must not matter
GARBAGE = 0xDEADBEEF     # ... and in the gate-context columns that are longest_match
_refs = {}


def shape(kind):
    """-> fixture name, Match slots, longest_match columns, Indirect models, their slots, the next-state tables"""
    if kind == "stock":
        _, z = goldenlib.load("ind_stock41")
        models = topology.stock_indirect()
        return ("match_stock", [2, 3, 4, 5, 6, 7], [6, 30], models, [(8 + 2 * i, 9 + 2 * i) for i in range(len(models))],
                (z["ns_next"], z["rm_next"]))
    _, z = goldenlib.load("ind_tiny_dense")
    name, mslots = ("match_k8", MSLOTS) if kind == "k8" else ("match_tiny", MSLOTS[:3])
    return name, list(mslots), [6, 30, 32], IND_MODELS, IND_SLOTS, (z["ns_next"], z["rm_next"])


def match_reference(name, offset, T):
    """match_ref.c over bits [0, T) of the fixture from byte `offset` (shared by the cases; never modified)."""
    key = (name, offset, T)
    if key not in _refs:
        f = mc.fixture(name)
        o = 8 * offset
        _refs[key] = ref_stream(f.models(), f.ctx[o:o + T], f.bc[o:o + T], f.bits[o:o + T])
    return _refs[key]


class Env:
    """The three device banks of a chain, the oracle's banks beside them, and the records of every stream."""

    def __init__(self, gpu, oracle, kind, T, S=1, offsets=(0,), topo=None, attach=True, history_capacity=None,
                 seed=11):
        self.gpu, self.oracle, self.kind, self.T, self.S = gpu, oracle, kind, T, S
        name, self.mslots, self.cols, self.imodels, self.islots, self.tabs = shape(kind)
        self.f = f = mc.fixture(name)
        self.topo = topo or topology.stock(90)
        self.N, self.M = self.topo.n_inputs, self.topo.n_mixers
        self.mmodels = [(t, f.limit, sl) for t, sl in zip(f.tables, self.mslots)]
        self.ig = gpu.IndirectGroup(self.imodels, *self.tabs, S, slots=self.islots)
        self.mg = gpu.MixerGroup(self.topo, S)
        self.mt = gpu.MatchGroup(self.mmodels, history_capacity or (T // 8 + 64), S)
        if attach:
            self.ig.attach_match(self.mt, self.cols)
        self.dev = list(self.mslots) + [i for ab in self.islots for i in ab]
        self.offsets = list(offsets)
        self.rec, self.ob, self.om, self.at = [], [], [], [0] * S
        rng = np.random.default_rng(seed)
        KI = len(self.imodels)
        for s in range(S):
            o = 8 * self.offsets[s]
            other, act_o, mctx, _ = oracle.synth(self.N, self.M, T, seed=seed + 7 * s, ctx_mode=4, zero_mod=4)
            act_o = act_o.copy()
            act_o[:, self.dev] = 0
            ictx = np.repeat(rng.integers(0, 1 << 20, (T // 8 + 1, KI)).astype(np.uint32), 8, axis=0)[:T]
            self.rec.append(dict(ctx=f.ctx[o:o + T], bc=f.bc[o:o + T], bits=f.bits[o:o + T], other=other, act=act_o,
                                 mctx=mctx, ictx=ictx, m=match_reference(name, self.offsets[s], T)))
            self.ob.append(oracle.IndirectBank(self.imodels, *self.tabs))
            self.om.append(oracle.Bank(self.N, self.topo.skip, self.topo.mixers))

    def expect(self, s, t):
        """the oracle chain's Predict of bit t of stream s on the reference's Match outputs"""
        r = self.rec[s]
        ip, ia = self.ob[s].predict(r["ictx"][t], r["bc"][t])
        pred, act, mctx = r["other"][t].copy(), r["act"][t].copy(), r["mctx"][t].copy()
        pred[self.mslots] = r["m"]["p"][t].view(np.float32)
        act[self.mslots] = r["m"]["a"][t]
        mctx[self.cols] = r["m"]["lm"][t]
        for i, (a, b_) in enumerate(self.islots):
            pred[a], pred[b_] = ip[2 * i], ip[2 * i + 1]
            act[a], act[b_] = ia[2 * i], ia[2 * i + 1]
        p_ref, o_ref = self.om[s].predict(pred, np.flatnonzero(act), mctx)
        return ip, ia, p_ref, o_ref

    def inputs(self, s, t):
        r = self.rec[s]
        stale = r["other"][t].copy()
        stale[self.dev] = STALE
        mctx = r["mctx"][t].copy()
        mctx[self.cols] = GARBAGE
        return stale, np.flatnonzero(r["act"][t]).astype(np.int32), mctx

    def forward(self, s, t, two_calls=False):
        """one Predict of the chain on the device, compared with the reference"""
        r = self.rec[s]
        ip, ia, p_ref, o_ref = self.expect(s, t)
        stale, host_active, mctx = self.inputs(s, t)
        if two_calls:   # the caller's own gmx_match_forward + gmx_chain_forward
            mp, ma, lm = self.mt.forward(r["ctx"][t], r["bc"][t], stream=s)
            stale[self.mslots] = mp
            act = r["act"][t].copy()
            act[self.mslots] = ma
            mctx[self.cols] = lm
            p, out, gp, ga = self.ig.chain_forward(self.mg, r["ictx"][t], r["bc"][t], stale,
                                                   np.flatnonzero(act).astype(np.int32), mctx, stream=s)
        else:
            p, out, gp, ga, mp, ma, lm = self.ig.chain_forward_match(self.mg, r["ictx"][t], r["ctx"][t], r["bc"][t],
                                                                     stale, host_active, mctx, stream=s)
        assert np.array_equal(u32(mp), r["m"]["p"][t]) and np.array_equal(ma, r["m"]["a"][t]), (s, t)
        assert lm == r["m"]["lm"][t], (s, t)
        assert np.array_equal(u32(gp), u32(ip)) and np.array_equal(ga, ia), (s, t)
        assert np.array_equal(u32(out), u32(o_ref)), (s, t)
        assert np.float32(p).view(np.uint32) == np.float32(p_ref).view(np.uint32), (s, t)

    def learn(self, s, t):
        bit = int(self.rec[s]["bits"][t])
        self.ig.learn(bit, stream=s)
        self.mg.learn(bit, stream=s)
        self.mt.learn(bit, stream=s)
        self.ob[s].learn(bit)
        self.om[s].learn(bit)
        self.at[s] = t + 1

    def bits(self, s, t0, t1, **kw):
        for t in range(t0, t1):
            self.forward(s, t, **kw)
            self.learn(s, t)

    def check_exports(self, s, t_end=None):
        """all three banks against the references, which stand behind bit t_end (the Match reference: behind T)"""
        assert self.ig.export(s) == self.ob[s].export(), s
        assert self.mg.export(s) == (self.om[s].export_long(), self.om[s].export_short()), s
        if t_end is None or t_end == self.T:
            ref = self.rec[s]["m"]["ref"]
        else:
            f, o = self.f, 8 * self.offsets[s]
            ref = mc.Ref(f.models())
            ref.run(f.ctx[o:o + t_end], f.bc[o:o + t_end], f.bits[o:o + t_end])
        assert self.mt.export(s) == ref.export(), s
        want, nb = ref.slots()
        got, gnb = self.mt.slot_values(s)
        assert np.array_equal(u32(got), u32(want)) and gnb == nb, s

    def exports(self):
        return [(self.ig.export(s), self.mg.export(s), self.mt.export(s), self.mt.slot_values(s)[0].tobytes(), self.mt.slot_values(s)[1])
                for s in range(self.S)]

    def close(self):
        for x in (self.ig, self.mg, self.mt):
            x.close()


def debug_sessions(E, indirect, mixers):
    E.ig.L.gmx_debug_indirect_use_sessions.argtypes = [C.c_void_p, C.c_int]
    E.mg.L.gmx_debug_use_sessions.argtypes = [C.c_void_p, C.c_int]
    assert E.ig.L.gmx_debug_indirect_use_sessions(E.ig.h, 1 if indirect else 0) == 0
    assert E.mg.L.gmx_debug_use_sessions(E.mg.h, 1 if mixers else 0) == 0


def test_stock_shape_fused(gpu, oracle):
    """The six stock Match models (slots 2..7, columns 6 and 30) behind the 41 stock Indirect models and the stock
    mixers: stream 1 of two, its Match bank brought to bit 3 000 by gmx_match_run, then 2 000 bits of Predict + Learn
    through gmx_chain_forward_match.  Stream 0 is never touched and exports as constructed."""
    T0, T = 3000, 5000
    m = match_reference("match_stock", 0, T)
    assert (m["lm"][T0:] > 0).any() and m["a"][T0:].any(axis=0).all()  # longest_match moves, every model speaks
    E = Env(gpu, oracle, "stock", T, S=2, offsets=(0, 0))
    fresh = Env(gpu, oracle, "stock", 8, S=1)
    constructed = fresh.exports()[0]
    fresh.close()
    r = E.rec[1]
    b = gpu.MatchBatch(E.mt, T0)
    b.set_records(1, r["ctx"][:T0], r["bc"][:T0], r["bits"][:T0])
    b.upload()
    E.mt.run_ragged(b, [0, T0])
    E.mt.sync()
    b.close()
    # the oracle's Indirect and mixer banks start at bit 3 000 as the device's do: constructed
    E.bits(1, T0, T)
    E.mg.sync()
    E.check_exports(1)
    assert E.exports()[0] == constructed
    E.close()


K8_OFFSET = 0   # byte 0 of match_k8 gives a single stream every regime below (asserted)


def k8_reference(T):
    m = match_reference("match_k8", K8_OFFSET, T)
    return m


def test_the_whole_lane_group(gpu, oracle):
    """K = 8: every lane of the group 56..63 carries a model.  4 000 bits of match_k8 behind five small Indirect
    models, slots in both mask words of the 90 inputs."""
    T = 4000
    m = k8_reference(T)
    assert m["unpushed"] >= 100 and m["seven"] >= 1 and m["handover"] >= 1, (m["unpushed"], m["seven"], m["handover"])
    E = Env(gpu, oracle, "k8", T, offsets=(K8_OFFSET,))
    E.bits(0, 0, T)
    E.check_exports(0)
    E.close()


def test_three_models_idle_lanes_reduce_and_touch_nothing(gpu, oracle):
    """K = 3: lanes 59..63 take part in the group's reductions and touch no memory."""
    T = 2000
    m = match_reference("match_tiny", 0, T)
    assert m["handover"] >= 1 and m["a"].any(axis=0).all()
    E = Env(gpu, oracle, "tiny", T)
    E.bits(0, 0, T)
    E.check_exports(0)
    E.close()


@pytest.mark.parametrize("route", ["sessions", "no_indirect_session", "no_sessions", "detached", "wide_mixers"])
def test_same_floats_on_every_route(gpu, oracle, route):
    """The first 600 bits of the K = 8 case with the one-command path, with either side on a launch per call, with no
    bank attached (the caller's own two calls) and with mixers that are not the stock shape."""
    T = 600
    topo = topology.synth3(256, table0=1 << 8) if route == "wide_mixers" else None
    E = Env(gpu, oracle, "k8", T, offsets=(K8_OFFSET,), topo=topo, attach=route != "detached")
    if route in ("no_indirect_session", "no_sessions"):
        debug_sessions(E, indirect=False, mixers=route != "no_sessions")
    E.bits(0, 0, T, two_calls=route == "detached")
    E.check_exports(0)
    E.close()


def test_idle_exits_and_replay(gpu, oracle):
    """Both waves leave on their idle timers between a forward and its learn (the restarted Indirect wave recomputes
    its forward from the mailbox: the Match lanes must not step a second time), and again between a learn and the next
    forward."""
    T = 400
    E = Env(gpu, oracle, "k8", T, offsets=(K8_OFFSET,))
    E.bits(0, 0, 131)
    E.forward(0, 131)
    time.sleep(0.06)
    E.learn(0, 131)
    E.bits(0, 132, 196)
    time.sleep(0.06)
    E.bits(0, 196, 260)
    E.check_exports(0, 260)
    E.close()


def test_two_streams_share_the_session_slots(gpu, oracle):
    """Streams 0 and 1 alternately: four sessions are wanted and three may be open, so every call evicts or is
    declined and takes another route -- the same floats."""
    T = 128
    E = Env(gpu, oracle, "k8", T, S=2, offsets=(K8_OFFSET, 100))
    for t in range(T):
        for s in (0, 1):
            E.forward(s, t)
            E.learn(s, t)
    for s in (0, 1):
        E.check_exports(s)
    E.close()


def test_between_surfaces_inside_a_byte(gpu, oracle):
    """333 bits chained; an export while a learn is noted (it includes that learn); 402 bits by gmx_match_run; 100 by
    gmx_match_forward / _learn; chained again to 2 000: the Match bank is the reference's at the end."""
    T = 2000
    E = Env(gpu, oracle, "k8", T, offsets=(K8_OFFSET,))
    r, f = E.rec[0], E.f
    E.bits(0, 0, 333)
    ref = mc.Ref(f.models())
    ref.run(r["ctx"][:333], r["bc"][:333], r["bits"][:333])
    assert E.mt.export(0) == ref.export()
    b = gpu.MatchBatch(E.mt, 402)
    b.set_records(0, r["ctx"][333:735], r["bc"][333:735], r["bits"][333:735])
    b.upload()
    E.mt.run(b, 402)
    b.download()
    b.wait()
    assert np.array_equal(u32(b.predictions[0]), r["m"]["p"][333:735])
    b.close()
    for t in range(735, 835):
        mp, ma, lm = E.mt.forward(r["ctx"][t], r["bc"][t])
        assert np.array_equal(u32(mp), r["m"]["p"][t]) and lm == r["m"]["lm"][t], t
        E.mt.learn(int(r["bits"][t]))
    # (the Indirect models and the mixers have their own history here: only the Match bank is followed to the end)
    stale, host_active, mctx = E.inputs(0, 0)
    for t in range(835, T):
        out = E.ig.chain_forward_match(E.mg, r["ictx"][t], r["ctx"][t], r["bc"][t], stale, host_active, mctx)
        assert np.array_equal(u32(out[4]), r["m"]["p"][t]) and np.array_equal(out[5], r["m"]["a"][t]), t
        assert out[6] == r["m"]["lm"][t], t
        for x in (E.ig, E.mg, E.mt):
            x.learn(int(r["bits"][t]))
    assert E.mt.export(0) == r["m"]["ref"].export()
    assert np.array_equal(u32(E.mt.slot_values(0)[0]), u32(r["m"]["ref"].slots()[0]))
    E.close()


def test_generation(gpu, oracle):
    """Every 40th bit is perceived, not learned (gmx_match_slots_set hands new_bit over, tester.cpp:296-302): against
    gmx_match_forward + gmx_chain_forward on twin banks."""
    T = 400
    A = Env(gpu, oracle, "k8", T, offsets=(K8_OFFSET,))
    B = Env(gpu, oracle, "k8", T, offsets=(K8_OFFSET,), attach=False)
    r = A.rec[0]
    for t in range(T):
        stale, host_active, mctx = A.inputs(0, t)
        p, out, gp, ga, mp, ma, lm = A.ig.chain_forward_match(A.mg, r["ictx"][t], r["ctx"][t], r["bc"][t], stale,
                                                              host_active, mctx)
        mp2, ma2, lm2 = B.mt.forward(r["ctx"][t], r["bc"][t])
        pr, act, cx = stale.copy(), r["act"][t].copy(), mctx.copy()
        pr[B.mslots], act[B.mslots], cx[B.cols] = mp2, ma2, lm2
        p2, out2, gp2, ga2 = B.ig.chain_forward(B.mg, r["ictx"][t], r["bc"][t], pr, np.flatnonzero(act).astype(np.int32),
                                                cx)
        assert np.array_equal(u32(mp), u32(mp2)) and np.array_equal(ma, ma2) and lm == lm2, t
        assert np.array_equal(u32(gp), u32(gp2)) and np.array_equal(ga, ga2), t
        assert np.array_equal(u32(out), u32(out2)) and np.float32(p).view(np.uint32) == np.float32(p2).view(np.uint32), t
        bit = int(r["bits"][t])
        for X in (A, B):
            if t % 40 == 39:
                X.mt.set_slot_values(X.mt.slot_values(0)[0], bit)
            else:
                X.ig.learn(bit)
                X.mg.learn(bit)
                X.mt.learn(bit)
    assert A.exports() == B.exports()
    A.close()
    B.close()


def test_protocol_and_validation(gpu, oracle):
    T = 64
    E = Env(gpu, oracle, "k8", T, offsets=(K8_OFFSET,), attach=False)
    L, r = E.ig.L, E.rec[0]
    i32p = C.POINTER(C.c_int32)

    def attach(ig, mt, cols):
        c = np.ascontiguousarray(cols, np.int32)
        return L.gmx_indirect_attach_match(ig.h, mt.h if mt else None, c.ctypes.data_as(i32p), len(c))

    def refused(code, fn, between_bits=True):
        """(between a forward and its learn the banks are not exported: what follows shows that none has moved)"""
        before = E.exports() if between_bits else None
        with pytest.raises(GmxError) as e:
            fn()
        assert e.value.status == code, e.value
        assert not between_bits or E.exports() == before

    # ---- at attach
    _, z = goldenlib.load("ind_tiny_dense")
    many = gpu.IndirectGroup([(3, 0.1)] * 57, z["ns_next"], z["rm_next"], 1,
                             slots=[(100 + 2 * i, 101 + 2 * i) for i in range(57)])
    assert attach(many, E.mt, [6]) == GMX_ERR_INVALID          # more than 56 models: no idle lane group
    many.close()
    two = gpu.MatchGroup(E.mmodels, 64, 2)
    assert attach(E.ig, two, [6]) == GMX_ERR_INVALID            # stream counts differ
    two.close()
    assert attach(E.ig, E.mt, [6, -1]) == GMX_ERR_INVALID
    assert attach(E.ig, E.mt, list(range(9))) == GMX_ERR_INVALID
    clash = gpu.MatchGroup([(16, 5, IND_SLOTS[1][1])], 64, 1)
    assert attach(E.ig, clash, [6]) == GMX_ERR_INVALID          # a Match slot that is an Indirect model's
    clash.close()
    before = E.exports()
    stale, host_active, mctx = E.inputs(0, 0)
    call = lambda: E.ig.chain_forward_match(E.mg, r["ictx"][0], r["ctx"][0], r["bc"][0], stale, host_active, mctx)
    E.ig.match = E.mt
    refused(GMX_ERR_STATE, call)                                # nothing attached
    # ---- a column beyond the group's gate contexts: refused by the call, before either bank moves
    assert attach(E.ig, E.mt, [6, 33]) == 0
    refused(GMX_ERR_INVALID, call)
    # ---- a bank that steps in a gmx_chainstep cannot ride in the sessions as well, and the other way round
    cs = gpu.ChainStep(E.mg, E.ig)
    assert L.gmx_chainstep_attach_match(cs.h, E.mt.h, np.zeros(1, np.int32).ctypes.data_as(i32p), 1) == GMX_ERR_STATE
    assert attach(E.ig, None, []) == 0                          # detach ...
    assert L.gmx_chainstep_attach_match(cs.h, E.mt.h, np.zeros(1, np.int32).ctypes.data_as(i32p), 1) == 0
    assert attach(E.ig, E.mt, E.cols) == GMX_ERR_STATE
    cs.close()
    assert attach(E.ig, E.mt, E.cols) == 0                      # ... and re-attach
    assert E.exports() == before
    # ---- a second forward without a learn
    E.forward(0, 0)
    refused(GMX_ERR_STATE, call, between_bits=False)
    E.learn(0, 0)
    E.bits(0, 1, 16)
    E.check_exports(0, 16)
    E.close()
    # ---- the history one byte short: the learn that would push byte `need` is refused when it is noted -- nothing
    # is published, no bank moves
    m = match_reference("match_k8", K8_OFFSET, T)
    need = int(m["ref"].history_size())
    assert need >= 2
    E = Env(gpu, oracle, "k8", T, offsets=(K8_OFFSET,), history_capacity=need - 1)
    t = 0
    while True:
        E.forward(0, t)
        if r["bc"][t] >= 127 and E.mt.history_size(0) == need - 1:
            break
        E.learn(0, t)
        t += 1
    refused(GMX_ERR_INVALID, lambda: E.mt.learn(int(r["bits"][t])), between_bits=False)
    refused(GMX_ERR_INVALID, lambda: E.mt.learn(int(r["bits"][t])), between_bits=False)   # (nothing was noted)
    assert E.mt.history_size(0) == need - 1
    E.close()
    # ---- destroy order: the Match bank first, then the Indirect bank; the reverse on a second set
    for first in ("match", "indirect"):
        E = Env(gpu, oracle, "k8", T, offsets=(K8_OFFSET,))
        E.bits(0, 0, 9)
        E.forward(0, 9)
        order = (E.mt, E.ig) if first == "match" else (E.ig, E.mt)
        for x in order:
            x.close()
        E.mg.close()
