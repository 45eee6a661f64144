"""gmx_indirect_attach_ctx / gmx_chain_forward_ctx: the context variables of a stream step at the head of a chained
forward in the Indirect models' per-bit session wave and feed the Match lanes, the Indirect models and the mixers of
the same command -- the host sends one bit.  Expected values: tests/helpers/ctx_ref.c for the variables,
tests/helpers/match_ref.c for the Match models on the routed context words, the oracle's Indirect and mixer banks on
the merged records, bit by bit.  Tolerance 0 everywhere: floats and values are compared as bit patterns, banks as
exported bytes.  Routed places hold 0xDEADBEEF and the device-side models' slots a stale float: neither may matter.

Every case asserts on ctx_ref.c alone, before it looks at the device, that its bits reach what it is there for."""
import ctypes as C
import time

import numpy as np
import pytest

import ctx_common as cc
import ctx_shapes
import goldenlib
import match_common as mc
import test_gpu_chainstep_match as tm
from gmix_amd import GmxError, topology
from test_gpu_chain_match import debug_sessions
from test_gpu_chainstep_ctx import IND_ROUTE, MATCH_ROUTE, Source, columns, same_entry_openings, tiny_source

pytestmark = pytest.mark.gpu

GMX_ERR_INVALID, GMX_ERR_STATE = -1, -5
STALE, GARBAGE = 123.0, 0xDEADBEEF
COLS = [6, 30, 32]          # the mixers' gate contexts that are longest_match
u32 = tm.u32
_src = {}


def mixer_route(M, V):
    """M columns over V variables: every fourth column, and the longest_match columns, stay the caller's."""
    return [-1 if (c % 4 == 3 or c in COLS) else (5 * c + 1) % V for c in range(M)]


def source_streams(src, offsets, T):
    """ctx_ref.c over the T bits of src from every byte offset: (bits, values, same-entry openings per table); shared
    between the cases, never modified."""
    out = []
    for o in offsets:
        key = (src.name, o, T)
        if key not in _src:
            bits = src.bits[8 * o:8 * o + T]
            assert len(bits) == T
            vals = cc.Ref(src.descs).run(bits)
            vals.setflags(write=False)
            _src[key] = (bits, vals, same_entry_openings(src, bits))
        out.append(_src[key])
    return out


class Env:
    """The four device banks of a chain, the references beside them, and the records of every stream."""

    def __init__(self, gpu, oracle, T, S=1, offsets=(3,), match=True, topo=None, attach=True, src=None, ind_route=None,
                 match_route=None, seed=31):
        self.gpu, self.T, self.S, self.match = gpu, T, S, match
        self.src = src or tiny_source()
        V = len(self.src.descs)
        self.topo = topo or topology.stock(90)
        self.N, self.M = self.topo.n_inputs, self.topo.n_mixers
        _, z = goldenlib.load("ind_tiny_dense")
        self.tabs = (z["ns_next"], z["rm_next"])
        self.fm = fm = mc.fixture("match_k8")
        self.mslots = list(tm.MSLOTS) if match else []
        self.cols = COLS if match else []
        self.mroute = mixer_route(self.M, V)
        self.iroute = list(ind_route or IND_ROUTE)
        self.xroute = list(match_route or MATCH_ROUTE)
        self.cg = gpu.CtxGroup(self.src.descs, S)
        self.ig = gpu.IndirectGroup(tm.IND_MODELS, *self.tabs, S, slots=tm.IND_SLOTS)
        self.mg = gpu.MixerGroup(self.topo, S)
        self.mt = gpu.MatchGroup([(t, fm.limit, sl) for t, sl in zip(fm.tables, self.mslots)], T // 8 + 64, S) if match else None
        if attach:
            self.attach()
        self.dev = self.mslots + [i for ab in tm.IND_SLOTS for i in ab]
        self.offsets = list(offsets)
        self.rec, self.ob, self.om = [], [], []
        rng = np.random.default_rng(seed)
        KI = len(tm.IND_MODELS)
        for s, (bits, vals, same) in enumerate(source_streams(self.src, self.offsets, T)):
            bc = vals[:, self.src.bit_context_var]
            other, act_o, pat, _ = oracle.synth(self.N, self.M, T, seed=seed + 7 * s, ctx_mode=4, zero_mod=4)
            act_o = act_o.copy()
            act_o[:, self.dev] = 0
            mctx_true, mctx_host = columns(self.mroute, vals, pat)
            mctx_host[:, self.cols] = GARBAGE
            ipat = np.repeat(rng.integers(0, 1 << 20, (T // 8 + 1, KI)).astype(np.uint32), 8, axis=0)[:T]
            ictx_true, ictx_host = columns(self.iroute, vals, ipat)
            xctx_true, xctx_host = columns(self.xroute, vals, np.zeros((T, len(self.xroute)), np.uint32))
            m = tm.ref_stream(fm.models(), xctx_true, bc, bits) if match else None
            self.rec.append(dict(bits=bits, vals=vals, bc=bc, same=same, other=other, act=act_o, mctx_true=mctx_true,
                                 mctx_host=mctx_host, ictx_true=ictx_true, ictx_host=ictx_host, xctx_true=xctx_true,
                                 xctx_host=xctx_host, m=m))
            self.ob.append(oracle.IndirectBank(tm.IND_MODELS, *self.tabs))
            self.om.append(oracle.Bank(self.N, self.topo.skip, self.topo.mixers))

    def attach(self):
        if self.match:
            self.ig.attach_match(self.mt, self.cols)
        self.ig.attach_ctx(self.cg, self.mroute, self.iroute, self.xroute if self.match else None)

    def expect(self, s, t):
        r = self.rec[s]
        ip, ia = self.ob[s].predict(r["ictx_true"][t], r["bc"][t])
        pred, act, mctx = r["other"][t].copy(), r["act"][t].copy(), r["mctx_true"][t].copy()
        if self.match:
            pred[self.mslots] = r["m"]["p"][t].view(np.float32)
            act[self.mslots] = r["m"]["a"][t]
            mctx[self.cols] = r["m"]["lm"][t]
        for i, (a, b_) in enumerate(tm.IND_SLOTS):
            pred[a], pred[b_] = ip[2 * i], ip[2 * i + 1]
            act[a], act[b_] = ia[2 * i], ia[2 * i + 1]
        p_ref, o_ref = self.om[s].predict(pred, np.flatnonzero(act), mctx)
        return ip, ia, p_ref, o_ref

    def call(self, s, t):
        r = self.rec[s]
        stale = r["other"][t].copy()
        stale[self.dev] = STALE
        return self.ig.chain_forward_ctx(self.mg, stale, np.flatnonzero(r["act"][t]).astype(np.int32), r["mctx_host"][t],
                                         contexts=r["ictx_host"][t],
                                         match_contexts=r["xctx_host"][t] if self.match else None, stream=s)

    def forward(self, s, t, against_oracle=True):
        """one Predict of the chain on the device, compared with the references"""
        r = self.rec[s]
        if against_oracle:
            ip, ia, p_ref, o_ref = self.expect(s, t)
        g = self.call(s, t)
        assert np.array_equal(g["values"], r["vals"][t]), (s, t, np.flatnonzero(g["values"] != r["vals"][t]))
        assert g["bit_context"] == r["bc"][t], (s, t)
        if self.match:
            assert np.array_equal(u32(g["mpred"]), r["m"]["p"][t]) and np.array_equal(g["mact"], r["m"]["a"][t]), (s, t)
            assert g["lm"] == r["m"]["lm"][t], (s, t)
        if against_oracle:
            assert np.array_equal(u32(g["pred"]), u32(ip)) and np.array_equal(g["act"], ia), (s, t)
            assert np.array_equal(u32(g["out"]), u32(o_ref)), (s, t)
            assert np.float32(g["p"]).view(np.uint32) == np.float32(p_ref).view(np.uint32), (s, t)
        return g

    def learn(self, s, t, oracle_too=True):
        bit = int(self.rec[s]["bits"][t])
        for x in (self.cg, self.ig, self.mg) + ((self.mt,) if self.match else ()):
            x.learn(bit, stream=s)
        if oracle_too:
            self.ob[s].learn(bit)
            self.om[s].learn(bit)

    def bits(self, s, t0, t1):
        for t in range(t0, t1):
            self.forward(s, t)
            self.learn(s, t)

    def ctx_ref(self, s, t_end):
        ref = cc.Ref(self.src.descs)
        ref.run(self.rec[s]["bits"][:t_end], values=False)
        return ref

    def check_ctx(self, s, t_end):
        ref = self.ctx_ref(s, t_end)
        assert self.cg.export(s)[0] == ref.export()[0], s
        assert cc.board_bytes(self.cg.blackboard(s)) == cc.board_bytes(ref.board()), s

    def check_exports(self, s, t_end):
        """all four banks against the references, which stand behind bit t_end"""
        self.check_ctx(s, t_end)
        assert self.ig.export(s) == self.ob[s].export(), s
        assert self.mg.export(s) == (self.om[s].export_long(), self.om[s].export_short()), s
        if self.match:
            r = self.rec[s]
            ref = mc.Ref(self.fm.models())
            ref.run(r["xctx_true"][:t_end], r["bc"][:t_end], r["bits"][:t_end])
            assert self.mt.export(s) == ref.export(), s
            want, nb = ref.slots()
            got, gnb = self.mt.slot_values(s)
            assert np.array_equal(u32(got), u32(want)) and gnb == nb, s

    def exports(self):
        out = []
        for s in range(self.S):
            out.append((self.cg.export(s)[0], cc.board_bytes(self.cg.blackboard(s)), self.ig.export(s), self.mg.export(s))
                       + ((self.mt.export(s), self.mt.slot_values(s)[0].tobytes()) if self.match else ()))
        return out

    def close(self):
        for x in (self.ig, self.mg, self.cg) + ((self.mt,) if self.match else ()):
            x.close()


def bit_launches(E):
    """launches of gmx_ctx_bit_kernel on the context bank so far: a bit that went through the session wave adds none"""
    E.cg.L.gmx_debug_ctx_bit_launches.argtypes = [C.c_void_p]
    n = E.cg.L.gmx_debug_ctx_bit_launches(E.cg.h)
    assert n >= 0
    return n


def assert_reaches_the_regimes(E, s=0):
    src, r = E.src, E.rec[s]
    sizes = [d.table_size for d in src.descs if d.kind == 6]
    assert all(n >= 1 for n, size in zip(r["same"], sizes) if size > 1), (r["same"], sizes)   # old index == new index
    assert cc.Ref(src.descs).board().first_prediction == 1        # bit 0 opens a byte on the first Predict
    assert any(c >= 0 for c in E.mroute) and any(c < 0 for c in E.mroute) and any(c < 0 for c in E.iroute)


@pytest.mark.parametrize("match", [True, False])
def test_one_command_path(gpu, oracle, match):
    """ctx_tiny's 17 variables into 33 stock-shape mixer columns, five Indirect models and (match) the eight models of
    match_k8: 2 000 bits, everything a bit returns at every bit, all banks and the board at the end."""
    T = 2000
    E = Env(gpu, oracle, T, match=match)
    assert_reaches_the_regimes(E)
    E.bits(0, 0, T)
    assert bit_launches(E) == 0          # every bit, and every learn, was a command of the wave
    E.check_exports(0, T)
    E.close()


@pytest.mark.parametrize("route", ["sessions", "no_indirect_session", "no_mixer_session", "no_sessions", "wide_mixers"])
def test_same_floats_on_every_route(gpu, oracle, route):
    """600 bits with the one-command path, with either side on a launch per call, with neither on sessions, and with
    mixers that are not the stock shape."""
    T = 600
    topo = topology.synth3(256, table0=1 << 8) if route == "wide_mixers" else None
    E = Env(gpu, oracle, T, topo=topo)
    assert_reaches_the_regimes(E)
    if route in ("no_indirect_session", "no_mixer_session", "no_sessions"):
        debug_sessions(E, indirect=route == "no_mixer_session", mixers=route == "no_indirect_session")
    E.bits(0, 0, T)
    # the one-command path launches nothing; every other route steps the bank with a launch per bit (the learn in it)
    assert bit_launches(E) == (0 if route == "sessions" else T)
    E.check_exports(0, T)
    E.close()


@pytest.mark.parametrize("how", ["mixers_off", "all_active"])
def test_idle_exit_then_a_change_of_route(gpu, oracle, how):
    """Chained bits with their learns noted, both waves gone on their idle timers, then a bit that takes the launch
    route (the mixers' sessions switched off, or n_active < 0): the Indirect learn of the bit before must be run on the
    board as it stood -- a wave restarted for it afterwards would recompute that forward from the board the launch has
    moved.  At a byte opening and inside a byte; the banks at the end."""
    T = 200
    E = Env(gpu, oracle, T)
    r = E.rec[0]
    at = [80, 117]
    assert r["bc"][80] == 0 and r["bc"][117] != 0
    assert all((r["ictx_true"][t] != r["ictx_true"][t - 1]).any() or r["bc"][t] != r["bc"][t - 1] for t in at)
    t = 0
    for stop in at:
        E.bits(0, t, stop)
        time.sleep(0.06)
        before = bit_launches(E)
        if how == "mixers_off":
            # (the mixers' switch alone: gmx_debug_indirect_use_sessions would stop the Indirect waves, and a stop runs
            # the noted learn by itself)
            E.mg.L.gmx_debug_use_sessions.argtypes = [C.c_void_p, C.c_int]
            assert E.mg.L.gmx_debug_use_sessions(E.mg.h, 0) == 0
            E.bits(0, stop, stop + 1)
            assert E.mg.L.gmx_debug_use_sessions(E.mg.h, 1) == 0
        else:   # every input active: the call takes the launches one after the other
            pred, mctx = r["other"][stop].copy(), r["mctx_true"][stop].copy()
            ip, ia = E.ob[0].predict(r["ictx_true"][stop], r["bc"][stop])
            pred[E.mslots] = r["m"]["p"][stop].view(np.float32)
            mctx[E.cols] = r["m"]["lm"][stop]
            act = np.ones(E.N, np.uint8)    # (the Indirect models' slots keep their own flags, as in gmx_chain_forward)
            for i, (a, b_) in enumerate(tm.IND_SLOTS):
                pred[a], pred[b_] = ip[2 * i], ip[2 * i + 1]
                act[a], act[b_] = ia[2 * i], ia[2 * i + 1]
            p_ref, o_ref = E.om[0].predict(pred, np.flatnonzero(act), mctx)
            stale = r["other"][stop].copy()
            stale[E.dev] = STALE
            E.ig.L.gmx_chain_forward_ctx.restype = C.c_int
            g = dict(out=np.zeros(E.M, np.float32), pred=np.zeros(2 * E.ig.K, np.float32))
            p = C.c_float()
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            rc = E.ig.L.gmx_chain_forward_ctx(E.ig.h, E.mg.h, 0, vp(r["ictx_host"][stop]), vp(r["xctx_host"][stop]),
                                              vp(stale), None, -1, vp(r["mctx_host"][stop]), C.byref(p), vp(g["out"]),
                                              vp(g["pred"]), None, None, None, None, None, None)
            assert rc == 0
            assert np.array_equal(u32(g["pred"]), u32(ip)) and np.array_equal(u32(g["out"]), u32(o_ref)), stop
            assert np.float32(p.value).view(np.uint32) == np.float32(p_ref).view(np.uint32), stop
            E.learn(0, stop)
        assert bit_launches(E) > before
        t = stop + 1
    E.bits(0, t, T)
    E.check_exports(0, T)
    E.close()


def test_idle_exits_and_replay(gpu, oracle):
    """Both waves leave on their idle timers between a forward and its learn -- the restarted wave recomputes its
    forward from the board and must not step the bank again -- and again between a learn and the next forward."""
    T = 400
    E = Env(gpu, oracle, T)
    assert E.rec[0]["bc"][131] != 0 and E.rec[0]["bc"][196] != 0     # both pauses fall inside a byte
    E.bits(0, 0, 131)
    E.forward(0, 131)
    time.sleep(0.06)
    E.learn(0, 131)
    E.bits(0, 132, 196)
    time.sleep(0.06)
    E.bits(0, 196, 260)
    # ... and at a byte opening
    E.forward(0, 260)
    assert E.rec[0]["bc"][264] == 0
    E.learn(0, 260)
    E.bits(0, 261, 264)
    E.forward(0, 264)
    time.sleep(0.06)
    E.learn(0, 264)
    E.bits(0, 265, 300)
    E.check_exports(0, 300)
    E.close()


def test_two_streams_share_the_session_slots(gpu, oracle):
    """Streams 0 and 1 alternately: four sessions are wanted and three may be open, so calls evict or are declined and
    take another route -- the same floats, and a wave that comes back reads the board again."""
    T = 128
    E = Env(gpu, oracle, T, S=2, offsets=(3, 61))
    for t in range(T):
        for s in (0, 1):
            E.forward(s, t)
            E.learn(s, t)
    for s in (0, 1):
        E.check_exports(s, T)
    E.close()


def test_between_surfaces_inside_a_byte(gpu, oracle):
    """333 bits chained; an export while a learn is noted (it includes that learn); 402 bits by gmx_ctx_run; 100 by
    gmx_ctx_forward / _learn; chained again to 1 200: values at every bit, the context bank the reference's at the end.
    (The other banks have a history of their own here: only the context bank is followed.)"""
    T = 1200
    E = Env(gpu, oracle, T, match=False)
    r = E.rec[0]
    assert r["bc"][333] != 0 and r["bc"][735] != 0 and r["bc"][835] != 0
    E.bits(0, 0, 333)
    E.check_ctx(0, 333)
    b = gpu.CtxBatch(E.cg, 402)
    b.bits[0] = r["bits"][333:735]
    b.upload()
    E.cg.run(b)
    b.download()
    b.wait()
    assert np.array_equal(b.values[0], r["vals"][333:735])
    b.close()
    for t in range(735, 835):
        got, bc = E.cg.forward(0)
        assert np.array_equal(got, r["vals"][t]) and bc == r["bc"][t], t
        E.cg.learn(int(r["bits"][t]))
    for t in range(835, T):
        E.forward(0, t, against_oracle=False)
        E.learn(0, t, oracle_too=False)
    E.check_ctx(0, T)
    E.close()


def test_generation(gpu, oracle):
    """Every 40th bit is perceived, not learned: gmx_ctx_learn is the Perceive of the context variables, the Match
    bank takes new_bit through its slots, the Indirect models and the mixers learn nothing.  Against the same calls on
    twin banks with the contexts filled by the host from ctx_ref.c."""
    T = 400
    A = Env(gpu, oracle, T)
    B = Env(gpu, oracle, T, attach=False)
    B.ig.attach_match(B.mt, B.cols)
    r = A.rec[0]
    for t in range(T):
        g = A.call(0, t)   # (the Match reference learns every bit: the twin banks are what holds here)
        assert np.array_equal(g["values"], r["vals"][t]) and g["bit_context"] == r["bc"][t], t
        stale = r["other"][t].copy()
        stale[B.dev] = STALE
        mctx = r["mctx_true"][t].copy()
        mctx[B.cols] = GARBAGE
        h = B.ig.chain_forward_match(B.mg, r["ictx_true"][t], r["xctx_true"][t], r["bc"][t], stale,
                                     np.flatnonzero(r["act"][t]).astype(np.int32), mctx)
        assert np.float32(g["p"]).view(np.uint32) == np.float32(h[0]).view(np.uint32), t
        assert np.array_equal(u32(g["out"]), u32(h[1])) and np.array_equal(u32(g["pred"]), u32(h[2])), t
        assert np.array_equal(g["act"], h[3]) and np.array_equal(u32(g["mpred"]), u32(h[4])), t
        assert np.array_equal(g["mact"], h[5]) and g["lm"] == h[6], t
        bit = int(r["bits"][t])
        A.cg.learn(bit)
        for X in (A, B):
            if t % 40 == 39:
                X.mt.set_slot_values(X.mt.slot_values(0)[0], bit)
            else:
                X.ig.learn(bit)
                X.mg.learn(bit)
                X.mt.learn(bit)
    assert A.exports()[0][2:] == tuple(x for x in (B.ig.export(0), B.mg.export(0), B.mt.export(0),
                                                   B.mt.slot_values(0)[0].tobytes()))
    A.check_ctx(0, T)
    A.close()
    B.close()


def test_64_variables_16_hash_tables(gpu, oracle):
    """ctx_shapes' v64_h16 list: every lane of the wave a variable for the phase, sixteen of them a hash table."""
    name = ctx_shapes.LONG_RUN_CASE
    named = ctx_shapes.descs(name)
    kinds = [k for _, k, _ in named]
    assert (len(named), kinds.count("indirect_hash")) == (64, 16)
    src = Source(name, ctx_shapes.as_descs(named), np.unpackbits(ctx_shapes.stream(name)), kinds.index("bit_context"))
    T = 800
    vals = source_streams(src, (3,), T)[0][1]
    moved = [v for v in range(64) if len(np.unique(vals[:, v])) > 1]
    # the variables move at all (a hash variable of a large, nearly empty table may keep hashing a fresh entry)
    assert len(moved) >= 48 and sum(kinds[v] == "indirect_hash" for v in moved) >= 10, moved
    # routed: variables that move -- byte-level ones for the Match models, a hash table first among the Indirect models'
    byte_level = [v for v in moved if kinds[v] in ("indirect_hash", "interval", "skip", "recent_byte")]
    iroute = [[v for v in moved if kinds[v] == "indirect_hash"][0], kinds.index("byte_plus_recent"), -1,
              [v for v in moved if kinds[v] == "skip"][0], 63]
    assert len(byte_level) >= 11 and 63 in moved
    E = Env(gpu, oracle, T, src=src, ind_route=iroute, match_route=byte_level[3:11])
    E.bits(0, 0, T)
    E.check_exports(0, T)
    E.close()


def test_stock_shape(gpu, oracle):
    """The 52 stock variables and the three stock routes behind the 41 stock Indirect models, the six stock Match models
    and the stock mixers: one stream, 40 bytes, against the same chain with every context filled by the host."""
    descs, mroute, iroute, xroute = topology.stock_contexts()
    assert len(descs) == 52 and len(mroute) == 33 and len(iroute) == 41 and len(xroute) == 6
    T = 320
    data = np.random.default_rng(5).integers(0, 256, T // 8, dtype=np.uint8)
    data[8:16] = data[0:8]                     # a repeat for the Match models
    bits = np.unpackbits(data)
    from gmix_amd.ctx import desc_array
    arr = desc_array(descs)
    vals = cc.Ref([arr[i] for i in range(52)]).run(bits)
    bc = vals[:, [n for n, _, _ in descs].index("bit_context")]
    assert (bc[::8] == 0).all() and len(np.unique(vals[:, iroute[-1]])) > 4
    _, z = goldenlib.load("ind_stock41")
    imodels = topology.stock_indirect()
    islots = [(8 + 2 * i, 9 + 2 * i) for i in range(len(imodels))]
    mslots, cols = [2, 3, 4, 5, 6, 7], topology.stock_longest_match_columns()
    mmodels = [(t, topology.STOCK_MATCH_LIMIT, sl) for (_, t), sl in zip(topology.STOCK_MATCH, mslots)]
    topo = topology.stock(90)
    N, M = topo.n_inputs, topo.n_mixers
    other, act_o, pat, _ = oracle.synth(N, M, T, seed=77, ctx_mode=4, zero_mod=4)
    dev = mslots + [i for ab in islots for i in ab]
    act_o = act_o.copy()
    act_o[:, dev] = 0
    lstm_col = iroute.index(-1)
    banks = []
    for attach in (True, False):
        ig = gpu.IndirectGroup(imodels, z["ns_next"], z["rm_next"], 1, slots=islots)
        mg = gpu.MixerGroup(topo, 1)
        mt = gpu.MatchGroup(mmodels, 64, 1)
        ig.attach_match(mt, cols)
        cg = gpu.CtxGroup(descs, 1) if attach else None
        if attach:
            ig.attach_ctx(cg, mroute, iroute, xroute)
        banks.append((ig, mg, mt, cg))
    (ia_, ma_, ta_, cg), (ib_, mb_, tb_, _) = banks
    mixer_true, mixer_host = columns(mroute, vals, pat)
    ind_true, ind_host = columns(iroute, vals, np.full((T, 41), 7, np.uint32))
    x_true, x_host = columns(xroute, vals, np.zeros((T, 6), np.uint32))
    assert (ind_host[:, lstm_col] == 7).all()
    for t in range(T):
        stale = other[t].copy()
        stale[dev] = STALE
        act = np.flatnonzero(act_o[t]).astype(np.int32)
        g = ia_.chain_forward_ctx(ma_, stale, act, mixer_host[t], contexts=ind_host[t], match_contexts=x_host[t])
        h = ib_.chain_forward_match(mb_, ind_true[t], x_true[t], bc[t], stale, act, mixer_true[t])
        assert np.array_equal(g["values"], vals[t]) and g["bit_context"] == bc[t], t
        assert np.float32(g["p"]).view(np.uint32) == np.float32(h[0]).view(np.uint32), t
        assert np.array_equal(u32(g["out"]), u32(h[1])) and np.array_equal(u32(g["pred"]), u32(h[2])), t
        assert np.array_equal(g["act"], h[3]) and np.array_equal(u32(g["mpred"]), u32(h[4])), t
        assert np.array_equal(g["mact"], h[5]) and g["lm"] == h[6], t
        bit = int(bits[t])
        for x in (cg, ia_, ma_, ta_, ib_, mb_, tb_):
            x.learn(bit)
    assert ia_.export(0) == ib_.export(0) and ma_.export(0) == mb_.export(0) and ta_.export(0) == tb_.export(0)
    ref = cc.Ref([arr[i] for i in range(52)])
    ref.run(bits, values=False)
    assert cg.export(0)[0] == ref.export()[0]
    assert cc.board_bytes(cg.blackboard(0)) == cc.board_bytes(ref.board())
    for tup in banks:
        for x in tup:
            if x is not None:
                x.close()


def test_protocol_and_validation(gpu, oracle):
    T = 64
    E = Env(gpu, oracle, T, attach=False)
    L = E.ig.L
    V = len(E.src.descs)

    def attach(ig, cg, mr, ir, xr):
        r = gpu._lib.CtxStepRoutes()
        keep = []
        for name, route in (("mixer", mr), ("ind", ir), ("match", xr)):
            if route is not None:
                a = np.ascontiguousarray(route, np.int32)
                keep.append(a)
                setattr(r, name + "_route", a.ctypes.data_as(C.POINTER(C.c_int32)))
                setattr(r, "n_" + name + "_route", len(a))
        return L.gmx_indirect_attach_ctx(ig.h, cg.h if cg is not None else None, C.byref(r))

    def refused(code, fn, moved_nothing=True):
        before = E.exports() if moved_nothing else None
        with pytest.raises(GmxError) as e:
            fn()
        assert e.value.status == code, e.value
        assert not moved_nothing or E.exports() == before

    before = E.exports()
    E.ig.ctx, E.ig.match = E.cg, E.mt   # (what the Python handle believes; the library knows better)
    refused(GMX_ERR_STATE, lambda: E.call(0, 0))                                    # nothing attached
    E.ig.ctx = E.ig.match = None
    # ---- at attach
    assert attach(E.ig, E.cg, E.mroute, E.iroute, E.xroute) == GMX_ERR_INVALID      # a match_route without a Match bank
    E.ig.attach_match(E.mt, E.cols)
    assert attach(E.ig, E.cg, E.mroute, E.iroute, None) == GMX_ERR_INVALID          # ... and the reverse
    assert attach(E.ig, E.cg, None, E.iroute, E.xroute) == GMX_ERR_INVALID          # no mixer route
    assert attach(E.ig, E.cg, E.mroute, E.iroute[:4], E.xroute) == GMX_ERR_INVALID  # a route of the wrong length
    assert attach(E.ig, E.cg, E.mroute, E.iroute[:4] + [V], E.xroute) == GMX_ERR_INVALID
    assert attach(E.ig, E.cg, E.mroute, [-2] + E.iroute[1:], E.xroute) == GMX_ERR_INVALID
    clash = list(E.mroute)
    clash[E.cols[1]] = 0
    assert attach(E.ig, E.cg, clash, E.iroute, E.xroute) == GMX_ERR_INVALID         # a longest_match column routed
    two = gpu.CtxGroup(E.src.descs, 2)
    assert attach(E.ig, two, E.mroute, E.iroute, E.xroute) == GMX_ERR_INVALID       # stream counts differ
    two.close()
    # ---- a bank that steps in a gmx_chainstep cannot ride in the sessions as well, and the other way round
    import test_gpu_chainstep_ctx as tc
    mg2 = gpu.MixerGroup(tc.TOPO, 1)
    cs = gpu.ChainStep(mg2)
    cs.attach_ctx(E.cg, tc.MIXER_ROUTE)
    assert attach(E.ig, E.cg, E.mroute, E.iroute, E.xroute) == GMX_ERR_STATE
    cs.close()
    assert attach(E.ig, E.cg, E.mroute, E.iroute, E.xroute) == 0
    cs = gpu.ChainStep(mg2)
    with pytest.raises(GmxError) as e:
        cs.attach_ctx(E.cg, tc.MIXER_ROUTE)
    assert e.value.status == GMX_ERR_STATE
    cs.close()
    mg2.close()
    other = gpu.IndirectGroup(tm.IND_MODELS, *E.tabs, 1, slots=tm.IND_SLOTS)
    assert attach(other, E.cg, E.mroute, E.iroute, None) == GMX_ERR_STATE           # attached to another Indirect bank
    other.close()
    with pytest.raises(GmxError) as e:
        E.ig.attach_match(E.mt, E.cols)                                             # Match first, as in the lock step
    assert e.value.status == GMX_ERR_STATE
    assert E.exports() == before
    # ---- at the forward: a mixer route of another length than the group's M; contexts missing for a column routed -1
    assert attach(E.ig, None, None, None, None) == 0
    assert attach(E.ig, E.cg, E.mroute[:-1], E.iroute, E.xroute) == 0
    E.ig.ctx = E.cg                     # (attached through the library directly above)
    refused(GMX_ERR_INVALID, lambda: E.call(0, 0))
    assert attach(E.ig, E.cg, E.mroute, E.iroute, E.xroute) == 0
    r = E.rec[0]
    refused(GMX_ERR_INVALID, lambda: E.ig.chain_forward_ctx(E.mg, r["other"][0], np.zeros(0, np.int32), r["mctx_host"][0],
                                                           contexts=None, match_contexts=r["xctx_host"][0]))
    refused(GMX_ERR_INVALID, lambda: E.ig.chain_forward_ctx(E.mg, r["other"][0], np.array([90], np.int32),
                                                           r["mctx_host"][0], contexts=r["ictx_host"][0],
                                                           match_contexts=r["xctx_host"][0]))
    # ---- a second forward without a learn
    E.forward(0, 0)
    refused(GMX_ERR_STATE, lambda: E.call(0, 0), moved_nothing=False)
    E.learn(0, 0)
    E.bits(0, 1, 16)
    E.check_exports(0, 16)
    E.close()
    # ---- destroy order: the context bank first, then the Indirect bank; the reverse on a second set
    for first in ("ctx", "indirect"):
        E = Env(gpu, oracle, T)
        E.bits(0, 0, 9)
        E.forward(0, 9)
        for x in ((E.cg, E.ig) if first == "ctx" else (E.ig, E.cg)):
            x.close()
        E.mg.close()
        E.mt.close()
