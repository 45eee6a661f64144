"""gmx_chainstep with a Match bank attached (gmx_chainstep_attach_match): the Match models of every stream step on the
device -- in lanes 56..63 of the Indirect models' launch, or in gmx_match_step_kernel where that launch cannot carry
them -- and feed the mixers of the same step.  Expected values: tests/helpers/match_ref.c for the Match models, the
oracle's Indirect / LSTM / mixer banks on the merged records for everything behind them.  Tolerance 0 everywhere:
floats are compared as bit patterns."""
import ctypes as C

import numpy as np
import pytest

import goldenlib
import match_common as mc
from gmix_amd import GmxError, Topology, topology

pytestmark = pytest.mark.gpu

LEARN, PREDICT = 1, 2
GMX_ERR_INVALID, GMX_ERR_STATE = -1, -5
MIXERS = [(0, 8, 0.005), (0, 256, 0.004), (0, 8, 0.0005), (1, 8, 0.0008), (1, 256, 0.003), (2, 1, 0.0005)]
COLS = [0, 2, 3]                           # the gate contexts that are longest_match
MSLOTS = [3, 31, 32, 33, 39, 0, 17, 8]     # both mask words, their first and last bits
IND_MODELS = [(256, 0.02), (3, 0.1), (65536, 0.005), (1000, 0.01), (77, 0.05)]
IND_SLOTS = [(1, 2), (4, 5), (6, 7), (9, 10), (34, 38)]
GARBAGE = 0xDEADBEEF                       # what match_contexts holds on steps that must not read it
_cache = {}


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def ref_stream(models, ctx, bc, bits):
    """One stream through match_ref.c, a bit at a time: slots / active / longest of every bit, the Ref object at the
    end, and what the stream exercised -- bytes kept out of the history, bits at longest_match 7, and steps whose
    Predict reads, as history[cur_match_], the byte the Learn of the same lock step has just pushed."""
    ref = mc.Ref(models)
    T, K = len(bits), len(models)
    wp, wa, wl = np.zeros((T, K), np.uint32), np.zeros((T, K), np.uint8), np.zeros(T, np.uint32)
    sb = np.zeros(11 * K, np.uint8)
    size = np.zeros(T + 1, np.int64)
    unpushed = handover = 0
    for t in range(T):
        p, a, l = ref.run(ctx[t:t + 1], bc[t:t + 1], bits[t:t + 1])
        wp[t], wa[t], wl[t] = p[0], a[0], l[0]
        size[t + 1] = ref.history_size()
        if bc[t] >= 127 and size[t + 1] == size[t]:
            unpushed += 1
        if bc[t] == 0 and t > 0 and size[t] > size[t - 1]:
            ref.L.mref_export_short(ref.h, sb.ctypes.data_as(C.c_void_p))
            cm = sb.reshape(K, 11)[:, :8].copy().view(np.uint64).ravel()
            handover += int((cm == size[t] - 1).any())
    return dict(p=wp, a=wa, lm=wl, ref=ref, unpushed=unpushed, seven=int((wl == 7).sum()), handover=handover)


def mask_words(act, mw):
    """act [T][N] flags -> [T][mw] mask words"""
    T, N = act.shape
    padded = np.zeros((T, mw * 32), np.uint8)
    padded[:, :N] = act != 0
    return np.packbits(padded.reshape(T, mw, 32), axis=2, bitorder="little").view(np.uint32).reshape(T, mw)


def small_chain(oracle, f, S, T, offsets, mslots, with_indirect, seed):
    """S streams of the 40-input six-mixer topology of test_into_a_mixer_batch, stream s replaying the fixture from
    byte offsets[s]: the caller's records (stacked [S][T]...), the Match reference and the oracle's p / outputs on the
    merged records."""
    key = (f.name, S, T, tuple(offsets), tuple(mslots), with_indirect, seed)
    if key in _cache:
        return _cache[key]
    N, M = 40, len(MIXERS)
    topo = Topology(N, MIXERS, (1,))
    _, z = goldenlib.load("ind_tiny_dense")
    tabs = (z["ns_next"], z["rm_next"])
    models = [(t, f.limit, sl) for t, sl in zip(f.tables, mslots)]
    dev = list(mslots) + ([i for ab in IND_SLOTS for i in ab] if with_indirect else [])
    rng = np.random.default_rng(seed)
    x = dict(topo=topo, tabs=tabs, models=models, other=[], maskw=[], mctx=[], ictx=[], bc=[], bits=[], mctxw=[], p=[],
             o=[], m=[])
    for s in range(S):
        o = 8 * offsets[s]
        ctx, bc, bits = f.ctx[o:o + T], f.bc[o:o + T], f.bits[o:o + T]
        r = ref_stream(f.models(), ctx, bc, bits)
        other, act_o, mctx, _ = oracle.synth(N, M, T, seed=seed + s, ctx_mode=2, zero_mod=4)
        pred, act, mc2 = other.copy(), act_o.copy(), mctx.copy()
        pred[:, mslots] = r["p"].view(np.float32)
        act[:, mslots] = r["a"]
        mc2[:, COLS] = r["lm"][:, None]
        ictx = np.repeat(rng.integers(0, 5000, (T // 8 + 1, len(IND_MODELS))).astype(np.uint32), 8, axis=0)[:T]
        if with_indirect:
            ip, ia = oracle.IndirectBank(IND_MODELS, *tabs).run(ictx, bc, bits)
            for i, (a, b_) in enumerate(IND_SLOTS):
                pred[:, a], pred[:, b_] = ip[:, 2 * i], ip[:, 2 * i + 1]
                act[:, a], act[:, b_] = ia[:, 2 * i], ia[:, 2 * i + 1]
        p_ref, o_ref = oracle.Bank(N, topo.skip, topo.mixers).run(pred, act, mc2, bits)
        host_act = act_o.copy()
        host_act[:, dev] = 0   # the device-side models' bits are left clear
        for k, v in (("other", other), ("maskw", mask_words(host_act, 2)), ("mctx", mctx), ("ictx", ictx), ("bc", bc),
                     ("bits", bits), ("mctxw", ctx), ("p", p_ref), ("o", o_ref), ("m", r)):
            x[k].append(v)
    for k in ("other", "maskw", "mctx", "ictx", "bc", "bits", "mctxw", "p", "o"):
        x[k] = np.stack(x[k])
    _cache[key] = x
    return x


def lockstep(gpu, cs, x, start, stop, path="step", pauses=None, check=True, ppm=None):
    """Bits [start, stop) of every stream of x through cs, the last step a learn alone.  pauses {(stream, bit): n}: at
    that bit (a byte's first) the stream learns alone, then sits n - 1 steps out, then predicts.  match_contexts holds
    the real words only where the library says it reads them."""
    S, N = x["bits"].shape[0], x["other"].shape[2]
    r = np.arange(S)
    pos = np.full(S, start)
    pending = np.zeros(S, bool)
    first = np.ones(S, bool)
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
        cs.predictions[:, :N] = x["other"][r, i]
        cs.active_mask[:] = x["maskw"][r, i]
        cs.contexts[:] = x["mctx"][r, i]
        cs.bit_contexts[:] = x["bc"][r, i]
        if cs.ind_contexts is not None:
            cs.ind_contexts[:] = x["ictx"][r, i]
        if ppm is not None:
            cs.ppm[:] = ppm[r, i // 8]
        need = (x["bc"][r, i] == 0) | first
        cs.match_contexts[:] = np.where(need[:, None], x["mctxw"][r, i], GARBAGE)
        cs.what[:] = learn * LEARN + pred * PREDICT
        if path == "commit":
            for s in np.flatnonzero(learn | pred):
                cs.commit(int(s))
            cs.launch()
            cs.wait()
        else:
            cs.step()
        if check and pred.any():
            assert np.array_equal(cs.p[pred].view(np.uint32), x["p"][r[pred], pos[pred]].view(np.uint32)), pos
            assert np.array_equal(u32(cs.outputs[pred]), u32(x["o"][r[pred], pos[pred]])), pos
        first &= ~pred
        pending = pred
        pos = pos + pred


def assert_match_state(g, refs):
    for s, ref in enumerate(refs):
        assert g.export(s) == ref.export(), s
        v, nb = g.slot_values(s)
        assert np.array_equal(u32(v), u32(ref.slots()[0])) and nb == ref.slots()[1], s


@pytest.mark.parametrize("path", ["step", "commit", "device_fetch"])
def test_fixture_through_the_fused_step(gpu, oracle, path, monkeypatch):
    """match_k8 (K = 8: the whole lane group), its first 4 000 bits from byte 0 / 500 / 1000, behind five Indirect
    models: lanes 0..4 are theirs, 5..55 idle, 56..63 the Match models'.  Every step's p and outputs, and the Match
    bank at the end."""
    if path == "device_fetch":
        monkeypatch.setenv("GMX_CS_NO_BAR", "1")
    f = mc.fixture("match_k8")
    S, T = 3, 4000
    x = small_chain(oracle, f, S, T, [500 * s for s in range(S)], MSLOTS, True, 40)
    m0 = x["m"][0]  # the fixture's own prefix
    assert m0["unpushed"] >= 100 and m0["seven"] >= 1 and m0["a"].any(axis=0).all()
    assert sum(m["handover"] for m in x["m"]) >= 1
    g = gpu.MatchGroup(x["models"], 1024, S)
    ig = gpu.IndirectGroup(IND_MODELS, *x["tabs"], S, slots=IND_SLOTS)
    mg = gpu.MixerGroup(x["topo"], S)
    cs = gpu.ChainStep(mg, ig)
    cs.attach_match(g, COLS)
    lockstep(gpu, cs, x, 0, T, path)
    cs.close()
    assert_match_state(g, [m["ref"] for m in x["m"]])
    for h in (g, ig, mg):
        h.close()


def test_stand_alone_kernel(gpu, oracle):
    """No Indirect models: gmx_match_step_kernel in front of the mixers'.  Nine streams -- two waves, the second with
    one stream -- of match_tiny (K = 3: five lanes of every group reduce and touch nothing), 2 000 bits."""
    f = mc.fixture("match_tiny")
    S, T = 9, 2000
    x = small_chain(oracle, f, S, T, [61 * s for s in range(S)], [31, 32, 39], False, 60)
    g = gpu.MatchGroup(x["models"], 1024, S)
    mg = gpu.MixerGroup(x["topo"], S)
    cs = gpu.ChainStep(mg)
    assert cs.match_contexts is None and cs.bit_contexts is None
    cs.attach_match(g, COLS)
    lockstep(gpu, cs, x, 0, T)
    cs.close()
    assert_match_state(g, [m["ref"] for m in x["m"]])
    g.close()
    mg.close()


def test_stock_lanes(gpu, oracle):
    """The reference's own shape: match_stock's six models beside the 41 stock Indirect models and the LSTM in ONE
    launch (gmx_indirect_step_kernel<true, true>), the stock 90-input mixers behind them, longest_match in gate
    contexts 6 and 30.  Bits 3 000..5 000 of the fixture -- where its matches begin -- the streams brought there by
    gmx_match_run."""
    f = mc.fixture("match_stock")
    _, z = goldenlib.load("ind_stock41")
    tabs = (z["ns_next"], z["rm_next"])
    models, topo = topology.stock_indirect(), topology.stock(90)
    K, S, T0, T, N, M = len(models), 2, 3000, 2000, 90, 33
    islots = [(8 + 2 * i, 9 + 2 * i) for i in range(K)]
    mslots, cols, lstm_slot, ind_lstm, mix_lstm = [2, 3, 4, 5, 6, 7], [6, 30], 1, 16, 22
    ctx, bc, bits = f.ctx[T0:T0 + T], f.bc[T0:T0 + T], f.bits[T0:T0 + T]
    data = f.data[T0 // 8:(T0 + T) // 8]
    ref = mc.Ref(f.models())
    ref.run(f.ctx[:T0], f.bc[:T0], f.bits[:T0])
    wp, wa, wl = ref.run(ctx, bc, bits)
    assert (wl > 0).any() and wa.any()
    rng = np.random.default_rng(7)
    x = dict(other=[], maskw=[], mctx=[], ictx=[], p=[], o=[], ppm=[])
    banks = []
    for s in range(S):
        ppm, _ = oracle.lstm_synth(T // 8, seed=70 + s, mask=63)
        ictx = np.repeat(rng.integers(0, 5000, (T // 8, K)).astype(np.uint32), 8, axis=0)
        mctx = np.repeat(rng.integers(0, 1 << 16, (T // 8, M)).astype(np.uint32), 8, axis=0)
        other, act_o, _, _ = oracle.synth(N, M, T, seed=80 + s, zero_mod=3)
        lm = oracle.LstmModel()
        lp, la, lc = lm.run(ppm, data)
        ictx_ref, mctx_ref = ictx.copy(), mctx.copy()
        ictx_ref[:, ind_lstm] = np.repeat(lc, 8)
        mctx_ref[:, mix_lstm] = np.repeat(lc, 8)
        mctx_ref[:, cols] = wl[:, None]
        io = oracle.IndirectBank(models, *tabs)
        ip, ia = io.run(ictx_ref, bc, bits)
        pred, act = other.copy(), np.zeros((T, N), np.uint8)
        act[:, 0] = act_o[:, 0]
        pred[:, lstm_slot], act[:, lstm_slot] = lp.reshape(-1), la.reshape(-1)
        pred[:, mslots], act[:, mslots] = wp.view(np.float32), wa
        for i, (a, b_) in enumerate(islots):
            pred[:, a], pred[:, b_] = ip[:, 2 * i], ip[:, 2 * i + 1]
            act[:, a], act[:, b_] = ia[:, 2 * i], ia[:, 2 * i + 1]
        mo = oracle.Bank(N, topo.skip, topo.mixers)
        p_ref, o_ref = mo.run(pred, act, mctx_ref, bits)
        host_act = np.zeros((T, N), np.uint8)
        host_act[:, 0] = act_o[:, 0]
        for k, v in (("other", other), ("maskw", mask_words(host_act, 3)), ("mctx", mctx), ("ictx", ictx), ("p", p_ref),
                     ("o", o_ref), ("ppm", ppm)):
            x[k].append(v)
        banks.append((mo, io, lm))
    x = {k: np.stack(v) for k, v in x.items()}
    x["bc"], x["bits"], x["mctxw"] = np.stack([bc] * S), np.stack([bits] * S), np.stack([ctx] * S)
    g = gpu.MatchGroup([(t, f.limit, sl) for t, sl in zip(f.tables, mslots)], len(f.data) + 64, S)
    b = gpu.MatchBatch(g, T0)
    for s in range(S):
        b.set_records(s, f.ctx[:T0], f.bc[:T0], f.bits[:T0])
    b.upload(T0)
    g.run(b, T0)
    b.close()
    lg, ig, mg = gpu.LstmGroup(S), gpu.IndirectGroup(models, *tabs, S, slots=islots), gpu.MixerGroup(topo, S)
    for s in range(S):
        lg.set_weights(oracle.LstmModel().weights(), stream=s)
    cs = gpu.ChainStep(mg, ig, lg, lstm_slot=lstm_slot, mixer_ctx_col=mix_lstm, ind_ctx_col=ind_lstm)
    cs.attach_match(g, cols)
    lockstep(gpu, cs, x, 0, T, ppm=x["ppm"])
    cs.close()
    assert_match_state(g, [ref] * S)
    for s, (mo, io, lm) in enumerate(banks):
        assert mg.export(s) == (mo.export_long(), mo.export_short()), s
        assert ig.export(s) == io.export(), s
        w, o = lg.get_weights(s)
        assert np.array_equal(u32(w), u32(lm.weights())) and np.array_equal(u32(o), u32(lm.output_layer())), s
    for h in (g, lg, ig, mg):
        h.close()


def test_streams_move_between_surfaces_inside_a_byte(gpu, oracle):
    """333 bits in lock step, the object destroyed; 402 bits by gmx_match_run and 100 by gmx_match_forward / _learn;
    the rest of 2 000 bits through a new lock-step object on the same banks, whose first Predict falls inside a byte.
    Stream 1 sits steps out between bytes in both lock-step stretches.  Nothing of a stream lives outside the bank:
    the end state is match_ref.c's."""
    f = mc.fixture("match_k8")
    S, T = 2, 2000
    x = small_chain(oracle, f, S, T, [500 * s for s in range(S)], MSLOTS, True, 40)
    g = gpu.MatchGroup(x["models"], 1024, S)
    ig = gpu.IndirectGroup(IND_MODELS, *x["tabs"], S, slots=IND_SLOTS)
    mg = gpu.MixerGroup(x["topo"], S)
    cs = gpu.ChainStep(mg, ig)
    cs.attach_match(g, COLS)
    lockstep(gpu, cs, x, 0, 333, pauses={(1, 8): 3, (1, 160): 1, (1, 320): 5})
    cs.close()
    t = 333
    b = gpu.MatchBatch(g, 402)
    for s in range(S):
        b.set_records(s, x["mctxw"][s, t:t + 402], x["bc"][s, t:t + 402], x["bits"][s, t:t + 402])
    b.upload(402)
    g.run(b, 402)
    b.download(402)
    b.wait()
    for s in range(S):
        assert np.array_equal(u32(b.predictions[s]), x["m"][s]["p"][t:t + 402]), s
        assert np.array_equal(b.longest[s], x["m"][s]["lm"][t:t + 402]), s
    b.close()
    t += 402
    for i in range(t, t + 100):
        for s in range(S):
            p, a, lm = g.forward(x["mctxw"][s, i], x["bc"][s, i], stream=s)
            assert np.array_equal(u32(p), x["m"][s]["p"][i]) and np.array_equal(a, x["m"][s]["a"][i]), (i, s)
            assert lm == x["m"][s]["lm"][i], (i, s)
            g.learn(x["bits"][s, i], stream=s)
    t += 100
    assert t % 8 != 0
    cs = gpu.ChainStep(mg, ig)
    cs.attach_match(g, COLS)
    # (the mixers and the Indirect models sat bits 333..835 out: only the Match bank is compared from here on)
    lockstep(gpu, cs, x, t, T, pauses={(1, 840): 2, (1, 1600): 4}, check=False)
    cs.close()
    assert_match_state(g, [m["ref"] for m in x["m"]])
    for h in (g, ig, mg):
        h.close()


def test_protocol_and_validation(gpu):
    N, M = 40, len(MIXERS)
    topo = Topology(N, MIXERS, (1,))
    mg = gpu.MixerGroup(topo, 2)
    good = gpu.MatchGroup([(16, 5, 0), (16, 5, 39)], 64, 2)
    cs = gpu.ChainStep(mg)
    assert cs.L.gmx_chainstep_match_contexts(cs.h) is None   # nothing attached
    bad = {"streams": (gpu.MatchGroup([(16, 5, 0)], 64, 3), [0]), "slot": (gpu.MatchGroup([(16, 5, N)], 64, 2), [0]),
           "column": (good, [M]), "negative column": (good, [-1]), "nine columns": (good, [0] * 9)}
    for what, (grp, cols) in bad.items():
        with pytest.raises(GmxError) as e:
            cs.attach_match(grp, cols)
        assert e.value.status == GMX_ERR_INVALID, what
        assert cs.L.gmx_chainstep_match_contexts(cs.h) is None, what
    cs.what[:] = [PREDICT, PREDICT]
    cs.step()
    with pytest.raises(GmxError) as e:   # after the object's first step
        cs.attach_match(good, COLS)
    assert e.value.status == GMX_ERR_STATE
    cs.close()
    cs = gpu.ChainStep(mg)
    cs.attach_match(good, COLS)
    with pytest.raises(GmxError) as e:   # once
        cs.attach_match(good, COLS)
    assert e.value.status == GMX_ERR_STATE
    cs.what[:] = [LEARN, 0]
    with pytest.raises(GmxError) as e:   # a learn without an outstanding predict
        cs.step()
    assert e.value.status == GMX_ERR_STATE
    cs.close()
    for grp, _ in bad.values():
        grp.close()
    mg.close()


def test_history_capacity_is_checked_before_the_step_is_queued(gpu):
    """history_capacity 64, 64 different bytes through gmx_match_run, the 65th in lock step: the step whose Learn would
    push it returns GMX_ERR_INVALID -- after the true sizes have been fetched -- and leaves the bank as it was."""
    from gmix_amd.match import stream_bits
    data = ((np.arange(80) * 37 + 11) % 251).astype(np.uint8)  # 80 different bytes: nothing matches, every byte is pushed
    bits, bc = stream_bits(data)
    ctx = np.repeat(np.concatenate(([0], data[:-1])).astype(np.uint32), 8)[:, None]
    topo = Topology(40, MIXERS, (1,))
    mg = gpu.MixerGroup(topo, 1)
    g = gpu.MatchGroup([(256, 400, 5)], 64, 1)
    b = gpu.MatchBatch(g, 512)
    b.set_records(0, ctx[:512], bc[:512], bits[:512])
    b.upload(512)
    g.run(b, 512)
    b.close()
    assert g.history_size(0) == 64
    cs = gpu.ChainStep(mg)
    cs.attach_match(g, [1])
    for t in range(512, 520):
        cs.what[0] = PREDICT | (LEARN if t > 512 else 0)
        cs.bits[0] = bits[t - 1]
        cs.bit_contexts[0] = bc[t]
        cs.match_contexts[0] = ctx[t]
        cs.step()
    before = g.export(0)
    cs.what[0], cs.bits[0] = LEARN, bits[519]
    with pytest.raises(GmxError) as e:
        cs.step()
    assert e.value.status == GMX_ERR_INVALID
    assert g.export(0) == before and g.history_size(0) == 64
    cs.close()
    g.close()
    mg.close()
