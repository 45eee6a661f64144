"""gmx_chainstep with a context bank attached (gmx_chainstep_attach_ctx): the context variables of every stream step on
the device at the head of every lock step (gmx_ctx_step.h) and feed the Indirect models, the Match models and the mixers
of the same step.  Expected values: tests/helpers/ctx_ref.c for the variables, tests/helpers/match_ref.c for the Match
models, the oracle's Indirect / mixer banks -- or the same chain on records the host filled -- for everything behind
them.  Tolerance 0 everywhere: floats are compared as bit patterns."""
import numpy as np
import pytest

import ctx_common as cc
import goldenlib
import match_common as mc
import test_gpu_chainstep_match as tm
import test_gpu_ctx_targets as tt
from gmix_amd import GmxError, Topology, topology

pytestmark = pytest.mark.gpu

LEARN, PREDICT = 1, 2
GMX_ERR_INVALID, GMX_ERR_STATE = -1, -5
GARBAGE = 0xDEADBEEF
N, M, K = 40, len(tm.MIXERS), len(tm.IND_MODELS)
TOPO = Topology(N, tm.MIXERS, (1,))
# ctx_tiny: hash_1 hash_3 hash_7 hash_100 skip_8 skip_15 skip_0 interval_odd_31 interval_pop_5 interval_xor_20
# interval_zero_1 last_byte recent_bytes[9] bit_context last_byte_plus_recent second_last_plus_recent always_zero.
# Every kind, both per-bit kinds and all four hash tables are routed somewhere; mixer column 2 and Indirect column 3
# stay the caller's.  (The mixers take context % table size, the Indirect models hash theirs: any 32-bit value goes.)
MIXER_ROUTE = [3, 13, -1, 7, 14, 16]
MIXER_ROUTE_MATCH = [-1, 13, -1, -1, 14, 16]   # columns 0, 2, 3 are longest_match (tm.COLS)
IND_ROUTE = [0, 1, 2, -1, 4]
IND_ROUTE_2 = [5, 6, 8, 9, 10]                 # (the refusals' second look at an Indirect route)
# the eight context words of match_k8's models: byte-level variables, as the reference's Match contexts are -- a Match
# model reads its word when a byte opens and keeps it for the byte (Match::Learn would see a per-bit variable move)
MATCH_ROUTE = [4, 11, 3, 5, 12, 2, 9, 7]
_cache = {}
u32 = tm.u32


def tiny():
    return cc.fixture("ctx_tiny")


def same_entry_openings(f, bits):
    """Per hash table: byte openings of the run at which IndirectHash's old and new index are the same entry.  f: a
    fixture, or a Source."""
    ref = cc.Ref(f.descs)
    sizes = [d.table_size for d in f.descs if d.kind == 6]
    H = len(sizes)
    count, prev = [0] * H, None
    for j in range(0, len(bits), 8):
        ref.run(bits[j:j + 8], values=False)
        raw, off = ref.export()
        idx = [int.from_bytes(raw[off[h + 1] - 4:off[h + 1]], "little") % sizes[h] for h in range(H)]
        if prev is not None:
            for h in range(H):
                count[h] += idx[h] == prev[h]
        prev = idx
    return count


def columns(route, vals, pattern):
    """[T][len(route)]: what the records hold in truth, and what the caller stages (GARBAGE in the routed places)."""
    true, host = pattern.copy(), pattern.copy()
    for c, r in enumerate(route):
        if r >= 0:
            true[:, c] = vals[:, r]
            host[:, c] = GARBAGE
    return true, host


class Source:
    """What chain() codes: a descriptor list (its name is the cache key), the bits of its stream, and which variable is
    bit_context."""

    def __init__(self, name, descs, bits, bit_context_var):
        self.name, self.descs, self.bits, self.bit_context_var = name, descs, bits, bit_context_var


def tiny_source():
    f = tiny()
    return Source("ctx_tiny", f.descs, f.bits, f.names.index("bit_context"))


def chain(oracle, S, T, offsets, with_indirect, mixer_route, t0=0, match=False, seed=90, src=None):
    """S streams of tm's 40-input six-mixer topology, stream s coding the bits of src (ctx_tiny unless given) from byte
    offsets[s], records of bits [t0, t0 + T): the caller's staging arrays, the truth from ctx_ref.c (and match_ref.c),
    and the oracle's p / outputs on the merged records.  IND_ROUTE and MATCH_ROUTE index src's variables."""
    f = src or tiny_source()
    key = (S, T, tuple(offsets), with_indirect, tuple(mixer_route), t0, match, seed) + ((f.name,) if src else ())
    if key in _cache:
        return _cache[key]
    _, z = goldenlib.load("ind_tiny_dense")
    tabs = (z["ns_next"], z["rm_next"])
    fm = mc.fixture("match_k8")
    mslots = tm.MSLOTS if match else []
    dev = list(mslots) + ([i for ab in tm.IND_SLOTS for i in ab] if with_indirect else [])
    rng = np.random.default_rng(seed)
    x = dict(tabs=tabs, models=[(t, fm.limit, sl) for t, sl in zip(fm.tables, mslots)], refs=[], m=[],
             bits=[], other=[], maskw=[], mctx_host=[], ictx_host=[], mctx_true=[], ictx_true=[], bc=[], mctxw=[], p=[],
             o=[], vals=[])
    for s in range(S):
        o = 8 * offsets[s]
        ref = cc.Ref(f.descs)
        allbits = f.bits[o:o + t0 + T]
        assert len(allbits) == t0 + T
        vals = ref.run(allbits)[t0:]
        bits = allbits[t0:]
        bc = vals[:, f.bit_context_var].copy()
        other, act_o, pat, _ = oracle.synth(N, M, T, seed=seed + s, ctx_mode=2, zero_mod=4)
        mctx_true, mctx_host = columns(mixer_route, vals, pat)
        ipat = np.repeat(rng.integers(0, 5000, (T // 8 + 2, K)).astype(np.uint32), 8, axis=0)[:T]
        ictx_true, ictx_host = columns(IND_ROUTE, vals, ipat)
        pred, act = other.copy(), act_o.copy()
        mctxw = vals[:, MATCH_ROUTE] if match or src is None else np.zeros((T, len(MATCH_ROUTE)), np.uint32)
        if match:
            if t0:   # (the Match models begin at t0 with the stream: their context words are the routed values)
                raise NotImplementedError
            r = tm.ref_stream(fm.models(), mctxw, bc, bits)
            pred[:, mslots] = r["p"].view(np.float32)
            act[:, mslots] = r["a"]
            mctx_true[:, tm.COLS] = r["lm"][:, None]
            x["m"].append(r)
        if with_indirect:
            ip, ia = oracle.IndirectBank(tm.IND_MODELS, *tabs).run(ictx_true, bc, bits)
            for i, (a, b_) in enumerate(tm.IND_SLOTS):
                pred[:, a], pred[:, b_] = ip[:, 2 * i], ip[:, 2 * i + 1]
                act[:, a], act[:, b_] = ia[:, 2 * i], ia[:, 2 * i + 1]
        p_ref, o_ref = oracle.Bank(N, TOPO.skip, TOPO.mixers).run(pred, act, mctx_true, bits)
        host_act = act_o.copy()
        host_act[:, dev] = 0   # the device-side models' bits are left clear
        x["refs"].append(ref)
        for k, v in (("bits", bits), ("other", other), ("maskw", tm.mask_words(host_act, 2)), ("mctx_host", mctx_host),
                     ("ictx_host", ictx_host), ("mctx_true", mctx_true), ("ictx_true", ictx_true), ("bc", bc),
                     ("mctxw", mctxw), ("p", p_ref), ("o", o_ref), ("vals", vals)):
            x[k].append(v)
    for k in ("bits", "other", "maskw", "mctx_host", "ictx_host", "mctx_true", "ictx_true", "bc", "mctxw", "p", "o"):
        x[k] = np.stack(x[k])
    _cache[key] = x
    return x


def drive(cs, x, start, stop, path="step", pauses=None, check=True, host_ctx=False, ppm=None, log=None, fill=GARBAGE):
    """Bits [start, stop) of every stream of x through cs, the last step a learn alone.  pauses {(stream, bit): n}: at
    that bit -- anywhere in a byte -- the stream learns alone, then sits n - 1 steps out, then predicts; at `start` it
    sits n steps out before it joins.  host_ctx: the caller fills every context (no bank attached); otherwise the
    routed places, bit_contexts and match_contexts hold `fill` on every step."""
    S = x["bits"].shape[0]
    n_in = x["other"].shape[2]
    r = np.arange(S)
    pos = np.full(S, start)
    pending = np.zeros(S, bool)
    pause_left = np.zeros(S, int)
    pauses = dict(pauses or {})
    Tm = x["bits"].shape[1] - 1
    while (pos < stop).any() or pending.any():
        for s in range(S):
            if pos[s] < stop and (s, int(pos[s])) in pauses:
                pause_left[s] = pauses.pop((s, int(pos[s])))
        learn = pending.copy()
        pred = (pos < stop) & (pause_left == 0)
        pause_left[pause_left > 0] -= 1
        i = np.minimum(pos, Tm)
        cs.bits[:] = np.where(learn, x["bits"][r, np.maximum(pos - 1, 0)], 0)
        cs.predictions[:, :n_in] = x["other"][r, i]
        cs.active_mask[:] = x["maskw"][r, i]
        cs.contexts[:] = x["mctx_true" if host_ctx else "mctx_host"][r, i]
        if cs.ind_contexts is not None:
            cs.ind_contexts[:] = x["ictx_true" if host_ctx else "ictx_host"][r, i]
        if cs.bit_contexts is not None:
            cs.bit_contexts[:] = x["bc"][r, i] if host_ctx else fill
        if cs.match_contexts is not None:
            cs.match_contexts[:] = x["mctxw"][r, i] if host_ctx else fill
        if ppm is not None:
            cs.ppm[:] = ppm[r, i // 8]
        cs.what[:] = learn * LEARN + pred * PREDICT
        if path == "commit":
            for s in np.flatnonzero(learn | pred):
                cs.commit(int(s))
            cs.launch()
            cs.wait()
        else:
            cs.step()
        if log is not None:
            log.append((pred.copy(), cs.p.view(np.uint32)[pred].copy(), u32(cs.outputs[pred]).copy()))
        if check and pred.any():
            assert np.array_equal(cs.p[pred].view(np.uint32), x["p"][r[pred], pos[pred]].view(np.uint32)), pos
            assert np.array_equal(u32(cs.outputs[pred]), u32(x["o"][r[pred], pos[pred]])), pos
        pending = pred
        pos = pos + pred


def assert_ctx_state(cg, refs):
    for s, ref in enumerate(refs):
        assert cg.export(s)[0] == ref.export()[0], s
        assert cc.board_bytes(cg.blackboard(s)) == cc.board_bytes(ref.board()), s


@pytest.mark.parametrize("path", ["step", "commit", "device_fetch"])
def test_every_kind_small_chain(gpu, oracle, path, monkeypatch):
    """ctx_tiny (17 variables of every kind, hash tables of 1, 3, 7 and 100 entries) from bytes 0 / 61 / 500, 2 000 bits,
    routed into six mixers and five Indirect models.  Every step's p and outputs; the bank at the end."""
    if path == "device_fetch":
        monkeypatch.setenv("GMX_CS_NO_BAR", "1")
    f = tiny()
    S, T, offsets = 3, 2000, [0, 61, 500]
    x = chain(oracle, S, T, offsets, True, MIXER_ROUTE)
    same = np.sum([same_entry_openings(f, x["bits"][s]) for s in range(S)], axis=0)
    sizes = [f.descs[v].table_size for v in f.hash_vars]
    assert all(n >= 1 for n, size in zip(same, sizes) if size > 1), (same, sizes)
    assert (x["mctx_host"][:, :, 2] != GARBAGE).all() and (x["ictx_host"][:, :, 3] != GARBAGE).all()
    cg = gpu.CtxGroup(f.descs, S)
    ig = gpu.IndirectGroup(tm.IND_MODELS, *x["tabs"], S, slots=tm.IND_SLOTS)
    mg = gpu.MixerGroup(TOPO, S)
    cs = gpu.ChainStep(mg, ig)
    before = cs.commit_bytes
    cs.attach_ctx(cg, MIXER_ROUTE, IND_ROUTE)
    assert cs.commit_bytes == before - 4    # both arrays keep a caller's column: only bit_contexts leaves the slices
    drive(cs, x, 0, T, path)
    cs.close()
    assert_ctx_state(cg, x["refs"])
    for h in (cg, ig, mg):
        h.close()


def test_ring_wrap_general_mixers_alone(gpu, oracle):
    """No Indirect models: the context node in front of the mixers' general kernel, bit_contexts stays NULL.  Nine
    streams, 8 400 bits (the 1 000-byte ring wraps); streams 2 and 7 join late, streams 1, 4 and 8 pause inside bytes
    and at byte boundaries."""
    f = tiny()
    S, T = 9, 8400
    offsets = [150 * s for s in range(S)]
    x = chain(oracle, S, T, offsets, False, MIXER_ROUTE, seed=120)
    cg = gpu.CtxGroup(f.descs, S)
    mg = gpu.MixerGroup(TOPO, S)
    cs = gpu.ChainStep(mg)
    cs.attach_ctx(cg, MIXER_ROUTE)
    assert cs.bit_contexts is None and cs.L.gmx_chainstep_bit_contexts(cs.h) is None
    pauses = {(2, 0): 5, (7, 0): 37, (1, 3): 2, (1, 8): 3, (4, 13): 1, (4, 8005): 4, (8, 4096): 2, (8, 4101): 6,
              (1, 8399): 3}
    drive(cs, x, 0, T, pauses=pauses)
    cs.close()
    assert x["refs"][0].board().rotating_history_pos == 1049 % 1000   # (the ring of 1 000 has taken 1 049 bytes)
    assert_ctx_state(cg, x["refs"])
    cg.close()
    mg.close()


def test_64_variables_16_hash_tables_mixers_alone(gpu, oracle):
    """Every lane of gmx_ctx_step_kernel holds a variable, sixteen of them a hash table: ctx_shapes' v64_h16 list
    (byte_plus_recent and recent_byte at indices beyond 1, random interval maps, skips), three streams of 2 000 bits,
    stream 1 pausing inside a byte, stream 2 joining late.  Six variables reach the mixers (a hash table, an interval,
    a skip, byte_plus_recent at an index the reference does not have, a recent byte, bit_context); all 64 and the
    tables are compared at the end."""
    import ctx_shapes
    name = ctx_shapes.LONG_RUN_CASE
    named = ctx_shapes.descs(name)
    kinds = [k for _, k, _ in named]
    src = Source(name, ctx_shapes.as_descs(named), np.unpackbits(ctx_shapes.stream(name)), kinds.index("bit_context"))
    assert (len(named), kinds.count("indirect_hash")) == (64, 16)
    bpr = [v for v, (_, k, p) in enumerate(named) if k == "byte_plus_recent" and p["index"] > 1][0]
    route = [kinds.index("indirect_hash"), kinds.index("interval"), kinds.index("skip"), bpr,
             kinds.index("recent_byte"), src.bit_context_var]
    S, T, offsets = 3, 2000, [0, 61, 500]
    x = chain(oracle, S, T, offsets, False, route, seed=180, src=src)
    same = np.sum([same_entry_openings(src, x["bits"][s]) for s in range(S)], axis=0)
    sizes = [d.table_size for d in src.descs if d.kind == 6]
    assert any(n >= 1 for n, size in zip(same, sizes) if size > 1), (same, sizes)
    cg = gpu.CtxGroup(src.descs, S)
    mg = gpu.MixerGroup(TOPO, S)
    cs = gpu.ChainStep(mg)
    cs.attach_ctx(cg, route)
    drive(cs, x, 0, T, pauses={(2, 0): 5, (1, 3): 2, (1, 1003): 4, (0, 1992): 1})
    cs.close()
    assert_ctx_state(cg, x["refs"])
    cg.close()
    mg.close()


@pytest.mark.parametrize("with_indirect", [True, False], ids=["fused", "match_step_kernel"])
def test_with_the_match_bank(gpu, oracle, with_indirect):
    """match_k8's eight models attached first, then the context bank with a match_route: the Match lanes (fused into
    the Indirect models' launch, or gmx_match_step_kernel) read the context words and the bit context the context node
    wrote.  Expected slots and longest_match: match_ref.c fed with ctx_ref.c's routed values."""
    f = tiny()
    S, T = 3, 2000
    x = chain(oracle, S, T, [0, 61, 500], with_indirect, MIXER_ROUTE_MATCH, match=True, seed=140)
    assert any(m["a"].any() for m in x["m"]) and any((m["lm"] > 0).any() for m in x["m"])
    cg = gpu.CtxGroup(f.descs, S)
    g = gpu.MatchGroup(x["models"], 1024, S)
    ig = gpu.IndirectGroup(tm.IND_MODELS, *x["tabs"], S, slots=tm.IND_SLOTS) if with_indirect else None
    mg = gpu.MixerGroup(TOPO, S)
    cs = gpu.ChainStep(mg, ig)
    cs.attach_match(g, tm.COLS)
    before = cs.commit_bytes
    cs.attach_ctx(cg, MIXER_ROUTE_MATCH, IND_ROUTE if with_indirect else None, MATCH_ROUTE)
    # bit_contexts, the Match words and the mixers' contexts (three routed columns, three longest_match: none is the
    # caller's) no longer cross the link; ind_contexts keeps the caller's column 3
    assert cs.commit_bytes == before - 4 - 4 * 8 - 4 * M
    drive(cs, x, 0, T)
    cs.close()
    tm.assert_match_state(g, [m["ref"] for m in x["m"]])
    assert_ctx_state(cg, x["refs"])
    for h in (cg, g, ig, mg):
        if h is not None:
            h.close()


def test_hand_over_between_the_surfaces(gpu, oracle):
    """gmx_ctx_run over 1 001 bytes + 5 bits (ctx_tiny's recorded position 8 013: inside a byte, the ring wrapped),
    300 lock steps on the same bank, the object destroyed, 100 more bits by gmx_ctx_run."""
    f = tiny()
    S, T0, T1, T2 = 2, 8013, 300, 100
    assert T0 in f.positions
    offsets = [0, 400]
    x = chain(oracle, S, T1, offsets, True, MIXER_ROUTE, t0=T0, seed=160)
    cg = gpu.CtxGroup(f.descs, S)
    b = gpu.CtxBatch(cg, T0, values=False)
    for s in range(S):
        b.bits[s] = f.bits[8 * offsets[s]:8 * offsets[s] + T0]
    b.upload()
    cg.run(b)
    cg.sync()
    b.close()
    assert cc.board_bytes(cg.blackboard(0)) == cc.board_bytes(f.boards[f.positions.index(T0)])
    ig = gpu.IndirectGroup(tm.IND_MODELS, *x["tabs"], S, slots=tm.IND_SLOTS)
    mg = gpu.MixerGroup(TOPO, S)
    cs = gpu.ChainStep(mg, ig)
    cs.attach_ctx(cg, MIXER_ROUTE, IND_ROUTE)
    drive(cs, x, 0, T1)
    cs.close()
    assert_ctx_state(cg, x["refs"])
    b = gpu.CtxBatch(cg, T2, values=True)
    want = []
    for s in range(S):
        o = 8 * offsets[s] + T0 + T1
        b.bits[s] = f.bits[o:o + T2]
        want.append(x["refs"][s].run(f.bits[o:o + T2]))   # (the cached Ref objects move on: this case owns its key)
    b.upload()
    cg.run(b)
    b.download()
    b.wait()
    for s in range(S):
        assert np.array_equal(b.values[s], want[s]), s
    assert_ctx_state(cg, x["refs"])
    del _cache[(S, T1, tuple(offsets), True, tuple(MIXER_ROUTE), T0, False, 160)]
    for h in (b, cg, ig, mg):
        h.close()


def stock_a_b(gpu, with_lstm):
    """The reference's own shape: topology.stock(90), the 41 stock Indirect models and the six stock Match models, the 52
    stock variables and their three routes; 2 streams x 40 bytes through gmx_stock_step_kernel and the fused models'
    launch.  Run A: the host fills every context from ctx_ref.c.  Run B: the bank attached and 0xFFFFFFFF in every routed
    place.  with_lstm: the LSTM byte model in the same launch, lstm_prediction_context in mixer column 22 and Indirect
    column 16 the device's -- then the caller owns no context column at all."""
    st = tt.stock()
    f, S, T = st["f"], tt.S, 8 * 40
    _, z = goldenlib.load("ind_stock41")
    islots = [(2 + 2 * i, 3 + 2 * i) for i in range(32)] + [(72 + 2 * j, 73 + 2 * j) for j in range(9)]
    dev_slots = list(topology.STOCK_MATCH_SLOTS) + [i for ab in islots for i in ab] + ([1] if with_lstm else [])
    rng = np.random.default_rng(23)
    w0 = ((rng.random((3, 50, 563), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
    ppm = rng.random((S, T // 8, 256), dtype=np.float32)
    ppm /= ppm.sum(axis=2, keepdims=True)
    cols = topology.stock_longest_match_columns()
    mr, ir, xr = st["mr"], st["ir"], st["xr"]
    assert mr[22] < 0 and ir[16] < 0 and all(mr[c] < 0 for c in cols) and (xr >= 0).all()
    lstm = st["lstm_ctx"][:T]
    x = dict(bits=[], other=[], maskw=[], mctx_host=[], ictx_host=[], mctx_true=[], ictx_true=[], bc=[], mctxw=[])
    for s in range(S):
        v = st["vals"][s][:T]
        act = st["act"][s, :T].copy()
        act[:, dev_slots] = 0
        pat_m = np.repeat(lstm[:, None], 33, axis=1)
        pat_i = np.repeat(lstm[:, None], 41, axis=1)
        mt, mh = columns(mr, v, pat_m)
        it, ih = columns(ir, v, pat_i)
        mh[mh == GARBAGE], ih[ih == GARBAGE] = tt.FILL, tt.FILL
        for k, a in (("bits", f.bits[8 * tt.OFFSETS[s]:8 * tt.OFFSETS[s] + T]), ("other", st["pred"][s, :T]),
                     ("maskw", tm.mask_words(act, 3)), ("mctx_host", mh), ("ictx_host", ih), ("mctx_true", mt),
                     ("ictx_true", it), ("bc", v[:, f.names.index("bit_context")]), ("mctxw", v[:, xr])):
            x[k].append(a)
    x = {k: np.stack(v) for k, v in x.items()}
    runs = []
    for attached in (False, True):
        mg = gpu.MixerGroup(topology.stock(90), S)
        ig = gpu.IndirectGroup(topology.stock_indirect(), z["ns_next"], z["rm_next"], S, slots=islots)
        xg = gpu.MatchGroup(topology.stock_match(), 40 + 64, S)
        cg = gpu.CtxGroup(st["descs"], S) if attached else None
        lg = gpu.LstmGroup(S) if with_lstm else None
        for s in range(S if with_lstm else 0):
            lg.set_weights(w0, stream=s)
        cs = gpu.ChainStep(mg, ig, lg, lstm_slot=1, mixer_ctx_col=22, ind_ctx_col=16) if with_lstm else gpu.ChainStep(mg, ig)
        cs.attach_match(xg, cols)
        if attached:
            before = cs.commit_bytes
            cs.attach_ctx(cg, mr, ir, xr)
            # without an LSTM its column of the mixers' and of the Indirect models' words is the caller's: only the Match
            # words and the bit context leave the slices.  With one, every context array does: 33 + 41 + 6 + 1 words
            assert cs.commit_bytes == before - (4 * (33 + 41 + 6 + 1) if with_lstm else 4 * 6 + 4)
        log = []
        drive(cs, x, 0, T, check=False, host_ctx=not attached, log=log, fill=tt.FILL, ppm=ppm if with_lstm else None)
        cs.close()
        exports = [(mg.export(s), ig.export(s), xg.export(s)) for s in range(S)]
        if with_lstm:
            exports.append([tuple(u32(a).tobytes() for a in lg.get_weights(s)) for s in range(S)])
            lg.close()
        if attached:
            for s in range(S):
                r = cc.Ref(f.descs)
                r.run(x["bits"][s], values=False)
                assert cg.export(s)[0] == r.export()[0] and cc.board_bytes(cg.blackboard(s)) == cc.board_bytes(r.board())
        runs.append((log, exports))
        for h in (cg, xg, ig, mg):
            if h is not None:
                h.close()
    (log_a, exp_a), (log_b, exp_b) = runs
    assert len(log_a) == len(log_b) == T + 1
    for t, (a, b) in enumerate(zip(log_a, log_b)):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), t
    assert exp_a == exp_b


def test_stock_shape(gpu):
    """Without the LSTM: mixer column 22 and Indirect column 16 carry the caller's fixed pattern."""
    stock_a_b(gpu, False)


@pytest.mark.parametrize("path", ["host_stores", "device_fetch"])
def test_stock_shape_with_the_lstm(gpu, path, monkeypatch):
    """The LSTM's bit prediction, the Indirect models and the Match lanes in ONE launch behind the context node, which
    is the only writer of contexts, ind_contexts, match_contexts and bit_contexts: no context array crosses the link.
    device_fetch: the fetch of what is left is a node of its own in front of the context node."""
    if path == "device_fetch":
        monkeypatch.setenv("GMX_CS_NO_BAR", "1")
    stock_a_b(gpu, True)


def test_refusals(gpu):
    """Everything gmx_chainstep_attach_ctx refuses, the calls a stream between its Predict and its Learn refuses, and
    steps after the bank is gone: each leaves the board and the object as they were."""
    f = tiny()
    S = 2
    _, z = goldenlib.load("ind_tiny_dense")
    tabs = (z["ns_next"], z["rm_next"])
    cg = gpu.CtxGroup(f.descs, S)
    mg = gpu.MixerGroup(TOPO, S)
    ig = gpu.IndirectGroup(tm.IND_MODELS, *tabs, S, slots=tm.IND_SLOTS)
    xg = gpu.MatchGroup([(16, 5, 0), (16, 5, 39)], 64, S)
    board = cc.board_bytes(cg.blackboard(0))

    def refused(cs, status, what, *a, **kw):
        n = cs.commit_bytes
        with pytest.raises(GmxError) as e:
            cs.attach_ctx(*a, **kw)
        assert e.value.status == status, what
        assert cs.commit_bytes == n and cc.board_bytes(cg.blackboard(0)) == board, what

    plain = gpu.ChainStep(mg)                        # no Indirect models, no Match bank
    other_s = gpu.CtxGroup(f.descs, 3)
    refused(plain, GMX_ERR_INVALID, "streams", other_s, MIXER_ROUTE)
    refused(plain, GMX_ERR_INVALID, "short route", cg, MIXER_ROUTE[:-1])
    refused(plain, GMX_ERR_INVALID, "entry == V", cg, [f.V] + MIXER_ROUTE[1:])
    refused(plain, GMX_ERR_INVALID, "entry < -1", cg, [-2] + MIXER_ROUTE[1:])
    refused(plain, GMX_ERR_INVALID, "no mixer_route", cg, None)
    refused(plain, GMX_ERR_INVALID, "ind_route without Indirect models", cg, MIXER_ROUTE, IND_ROUTE)
    refused(plain, GMX_ERR_INVALID, "match_route without a Match bank", cg, MIXER_ROUTE, None, [0, 1])
    assert plain.L.gmx_chainstep_attach_ctx(plain.h, cg.h, None) == GMX_ERR_INVALID
    plain.close()
    # (a route longer than 128 is always of the wrong length: a group has at most 64 mixers, a bank 64 / 8 models)
    long_route = gpu.ChainStep(mg)
    refused(long_route, GMX_ERR_INVALID, "route longer than 128", cg, [0] * 130)
    long_route.close()   # (before its group goes: the raised error's traceback would keep an unnamed object alive)
    mg2 = gpu.MixerGroup(TOPO, S)
    ig2 = gpu.IndirectGroup(tm.IND_MODELS, *tabs, S, slots=tm.IND_SLOTS)
    full = gpu.ChainStep(mg, ig)
    full.attach_match(xg, [0, 3])
    refused(full, GMX_ERR_INVALID, "a Match bank without a match_route", cg, MIXER_ROUTE_MATCH, IND_ROUTE)
    refused(full, GMX_ERR_INVALID, "Indirect models without an ind_route", cg, MIXER_ROUTE_MATCH, None, [0, 1])
    refused(full, GMX_ERR_INVALID, "a routed longest_match column", cg, MIXER_ROUTE, IND_ROUTE, [0, 1])
    refused(full, GMX_ERR_INVALID, "match_route of the wrong length", cg, MIXER_ROUTE_MATCH, IND_ROUTE, [0, 1, 2])
    # the columns that are the LSTM lanes' (mixer_ctx_col 2, ind_ctx_col 3)
    lg = gpu.LstmGroup(S)
    with_lstm = gpu.ChainStep(mg2, ig2, lg, lstm_slot=11, mixer_ctx_col=2, ind_ctx_col=3)
    refused(with_lstm, GMX_ERR_INVALID, "a routed mixer_ctx_col", cg, [3, 13, 16, 7, 14, 16], IND_ROUTE)
    refused(with_lstm, GMX_ERR_INVALID, "a routed ind_ctx_col", cg, MIXER_ROUTE, [0, 1, 2, 5, 4])
    # a step in flight (the object's first: nothing was waited for yet)
    w0 = ((np.random.default_rng(5).random((3, 50, 563), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
    for s in range(S):
        lg.set_weights(w0, stream=s)
    with_lstm.ppm[:] = 1.0 / 256
    with_lstm.what[:] = PREDICT
    with_lstm.launch()
    refused(with_lstm, GMX_ERR_STATE, "a step in flight", cg, MIXER_ROUTE, IND_ROUTE)
    with_lstm.wait()
    with_lstm.close()
    lg.close()
    # (another device: not testable with one GPU; the comparison stands beside the stream count's)
    full.attach_ctx(cg, MIXER_ROUTE_MATCH, IND_ROUTE, [0, 1])
    refused(full, GMX_ERR_STATE, "twice", cg, MIXER_ROUTE_MATCH, IND_ROUTE_2, [0, 1])
    with pytest.raises(GmxError) as e:               # a Match bank is attached first
        full.attach_match(xg, [0, 3])
    assert e.value.status == GMX_ERR_STATE
    with pytest.raises(GmxError) as e:
        cg.set_cu_mask([0xffffffff])
    assert e.value.status == GMX_ERR_STATE
    second = gpu.ChainStep(mg2)
    refused(second, GMX_ERR_STATE, "the bank is another object's", cg, MIXER_ROUTE)
    cg2 = gpu.CtxGroup(f.descs, S)
    second.what[:] = PREDICT
    second.step()
    n = second.commit_bytes
    with pytest.raises(GmxError) as e:               # after the object's first step
        second.attach_ctx(cg2, MIXER_ROUTE)
    assert e.value.status == GMX_ERR_STATE and second.commit_bytes == n
    second.close()
    # between a stream's Predict and its Learn
    full.what[:] = [PREDICT, 0]
    full.step()
    batch = gpu.CtxBatch(cg, 8, values=False)
    batch.upload()
    for call in (lambda: cg.run(batch, 8), lambda: cg.run_ragged(batch, [3, 0]), lambda: cg.blackboard(0),
                 lambda: cg2.copy_from(cg, 0, 1)):
        with pytest.raises(GmxError) as e:
            call()
        assert e.value.status == GMX_ERR_STATE
    cg.export(0)                                     # the tables alone: allowed
    cg.run_ragged(batch, [0, 0])                     # no bits for the stream
    stream1 = cc.board_bytes(cg.blackboard(1))
    assert stream1 == board                          # stream 1 sat the step out: untouched, and readable
    full.what[:], full.bits[:] = [LEARN, 0], [1, 0]
    full.step()
    r = cc.Ref(f.descs)
    r.run(np.array([1], np.uint8), values=False)
    assert cc.board_bytes(cg.blackboard(0)) == cc.board_bytes(r.board())
    full.what[:] = [PREDICT, PREDICT]
    full.step()
    cg.set_blackboard(r.board(), 0)                  # clears "predict outstanding" of stream 0
    assert cc.board_bytes(cg.blackboard(0)) == cc.board_bytes(r.board())
    with pytest.raises(GmxError) as e:
        cg.blackboard(1)
    assert e.value.status == GMX_ERR_STATE
    full.what[:], full.bits[:] = [PREDICT | LEARN, LEARN], [1, 0]   # stream 0 predicts again, stream 1 only learns
    full.step()
    with pytest.raises(GmxError) as e:
        cg.blackboard(0)
    assert e.value.status == GMX_ERR_STATE
    cg.reset()                                       # clears "predict outstanding" of every stream
    assert cc.board_bytes(cg.blackboard(0)) == board and cc.board_bytes(cg.blackboard(1)) == board
    # the bank destroyed first: the object's steps fail and write nothing
    p_before = full.p.copy()
    batch.close()
    cg.close()
    full.what[:], full.bits[:] = [LEARN, LEARN], [0, 0]
    with pytest.raises(GmxError) as e:
        full.step()
    assert e.value.status == GMX_ERR_STATE and np.array_equal(full.p, p_before)
    full.close()
    for h in (cg2, other_s, xg, ig2, ig, mg2, mg):
        h.close()
