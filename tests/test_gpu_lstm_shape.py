"""LSTM banks of any width and horizon (gmx_lstm_create_shaped, gmx_lstm_any.hip) against tests/lstm_shape_ref.c --
which tests/test_lstm_shape_ref.py pins to the reference's own Lstm class and to oracle.LstmModel --, against the
fixtures recorded from the real class (tests/golden/lstm_shapes.npz) and, at the stock shape under GMX_LSTM_BUILD=any,
against oracle.LstmModel.  Tolerance 0 everywhere: floats are compared as uint32, sections byte for byte."""
import os

import numpy as np
import pytest

import goldenlib
import lstm_shape_common as lsc
from gmix_amd import topology
from lstm_shape_common import u32

pytestmark = pytest.mark.gpu


def chunks_for(h, n):
    """Launch lengths that sum to n: the first launch ends inside a horizon, the second exactly on a backward pass
    (the byte whose Perceive finds epoch_ wrapped to 0 is its last), the rest follows."""
    assert n > 2 * h
    return [h - 1, h + 1, n - 2 * h]


def run_gpu(gpu, g, streams, chunks, learn=True):
    S, N = len(streams), sum(chunks)
    b = gpu.LstmBatch(g, max(chunks))
    P = np.zeros((S, N, 8), np.float32)
    A = np.zeros((S, N, 8), np.uint8)
    Cx = np.zeros((S, N), np.uint32)
    n0 = 0
    for n in chunks:
        for s, (ppm, data) in enumerate(streams):
            b.ppm[s, :n] = ppm[n0:n0 + n]
            b.bytes[s, :n] = data[n0:n0 + n]
        b.upload(n)
        g.run(b, n, learn=learn)
        b.download(n)
        b.wait()
        P[:, n0:n0 + n] = b.predictions[:, :n]
        A[:, n0:n0 + n] = b.active[:, :n]
        Cx[:, n0:n0 + n] = b.contexts[:, :n]
        n0 += n
    b.close()
    return P, A, Cx


def make_streams(oracle, S, N, seed):
    """Stream 0: the dense family; stream 1: the sparse / one-hot / uniform family; stream 2: runs of identical bytes."""
    out = []
    for s in range(S):
        ppm, data = oracle.lstm_synth(N, seed=seed + s, mask=255, family=1 if s == 1 else 0)
        if s == 2:
            data = np.repeat(data[::4], 4)[:N].copy()
        out.append((ppm, data))
    return out


def assert_stream_equals_ref(g, s, r, got, want, where):
    P, A, Cx = got
    bad = np.argwhere(u32(P) != u32(want["pred"]))
    assert len(bad) == 0, (where, s, "bit predictions", bad[:4])
    assert np.array_equal(A, want["act"]), (where, s, "active flags")
    assert np.array_equal(Cx, want["ctx"]), (where, s, "contexts")
    assert_state_equals_ref(g, s, r, where)


def assert_state_equals_ref(g, s, r, where):
    w, o = g.get_weights(s)
    assert np.array_equal(u32(w), u32(r.weights())), (where, s, "gate weights")
    assert np.array_equal(u32(o), u32(r.output_layer())), (where, s, "output layer")
    lng, sh = g.export(s)
    assert lng == r.export_long(), (where, s, ".long")
    rs = r.export_short()
    assert len(sh) == len(rs), (where, s, ".short size")
    if sh != rs:
        a, b = np.frombuffer(sh, np.uint8), np.frombuffer(rs, np.uint8)
        assert False, (where, s, ".short differs first at byte", int(np.argmax(a != b)))


# cells, horizon, learning_rate, gradient_clip, streams
SHAPES = [(1, 2, 0.03, 10.0, 3), (3, 3, 0.03, 10.0, 3), (50, 7, 0.03, 10.0, 3), (64, 5, 0.03, 10.0, 3),
          (65, 5, 0.01, 0.05, 3), (130, 4, 0.05, 2.5, 3), (256, 3, 0.03, 10.0, 2)]


@pytest.mark.parametrize("cells,horizon,lr,clip,S", SHAPES, ids=lambda v: str(v))
def test_kernel_equals_restatement(gpu, oracle, cells, horizon, lr, clip, S):
    """3 x horizon + 1 bytes (three backward passes) in three launches: every bit prediction, flag and context, the gate weights, the output
    layer and both export sections."""
    shape = (cells, horizon, lr, clip)
    N = 3 * horizon + 1
    streams = make_streams(oracle, S, N, seed=300 + cells)
    g = gpu.LstmGroup(S, shape=shape)
    assert tuple(g.shape[:2]) == (cells, horizon) and g.shape[2] == np.float32(lr) and g.shape[3] == np.float32(clip)
    refs = []
    for s in range(S):
        r = lsc.Ref(shape, seed=1000 + 7 * s + cells)
        g.set_weights(r.weights(), stream=s)
        refs.append((r, r.run(*streams[s])))
    assert g.memory_usage() == refs[0][0].memory_usage()
    P, A, Cx = run_gpu(gpu, g, streams, chunks_for(horizon, N))
    assert g.any_launches == 3
    for s in range(S):
        r, want = refs[s]
        assert r.backward_passes() == 3
        assert_stream_equals_ref(g, s, r, (P[s], A[s], Cx[s]), want, shape)
    g.close()


@pytest.mark.parametrize("case", lsc.golden(), ids=lambda c: c["name"])
def test_kernel_equals_the_reference_classes(gpu, oracle, case):
    """The fixture cases recorded from the reference's own Lstm: every byte's distribution through gmx_lstm_forward /
    gmx_lstm_perceive, then sha256 of the gate weights, the output layer and both export sections."""
    ppm, data = oracle.lstm_synth(case["n_bytes"], seed=case["synth_seed"], mask=case["mask"], family=case["family"])
    g = gpu.LstmGroup(1, shape=case["shape"])
    g.set_weights(lsc.Ref(case["shape"], seed=case["seed"]).weights())
    last = 0
    for n in range(case["n_bytes"]):
        probs, _ = g.forward(ppm[n], last)
        assert np.array_equal(u32(probs), case["probs"][n]), (case["name"], n)
        g.perceive(data[n])
        last = int(data[n])
    w, o = g.get_weights(0)
    assert lsc.sha(w.tobytes()) == case["sha_weights"]
    assert lsc.sha(o.tobytes()) == case["sha_output_layer"]
    lng, sh = g.export(0)
    assert lsc.sha(lng) == case["sha_long"]
    assert lsc.sha(sh) == case["sha_short"]
    g.close()


@pytest.fixture
def build_any():
    """GMX_LSTM_BUILD=any while a bank is created gives a stock-shape bank the general layout and kernel."""
    old = os.environ.get("GMX_LSTM_BUILD")
    os.environ["GMX_LSTM_BUILD"] = "any"
    yield
    if old is None:
        os.environ.pop("GMX_LSTM_BUILD", None)
    else:
        os.environ["GMX_LSTM_BUILD"] = old


def test_general_kernel_at_the_stock_shape_equals_oracle(gpu, oracle, build_any):
    """The body of test_gpu_lstm.py's test_lstm_kernel_equals_oracle_through_backward_passes on the general kernel."""
    S, N = 3, 450                       # four backward passes + Adam steps, launches that split them
    refs, streams = [], []
    for s in range(S):
        m = oracle.LstmModel()          # srand(0xDEADBEEF) + the reference's constructor chain
        ppm, data = oracle.lstm_synth(N, seed=11 + s, mask=15 if s == 1 else 255)
        refs.append((m, m.weights()) + m.run(ppm, data))
        streams.append((ppm, data))
    g = gpu.LstmGroup(S)
    assert tuple(g.shape) == (50, 100, np.float32(0.03), np.float32(10.0))
    for s in range(S):
        g.set_weights(refs[s][1], stream=s)
    P, A, Cx = run_gpu(gpu, g, streams, [170, 170, 110])
    assert g.any_launches == 3
    for s in range(S):
        m, _, pred, act, ctx = refs[s]
        bad = np.argwhere(u32(P[s]) != u32(pred))
        assert len(bad) == 0, (s, bad[:4], P[s][tuple(bad[0])], pred[tuple(bad[0])])
        assert np.array_equal(A[s], act) and np.array_equal(Cx[s], ctx)
        w, o = g.get_weights(s)
        assert np.array_equal(u32(w), u32(m.weights())), s
        assert np.array_equal(u32(o), u32(m.output_layer())), s
        assert g.export(s) == (m.export_long(), m.export_short()), s
    g.close()


def test_stock_bank_never_launches_the_general_kernel(gpu, oracle, monkeypatch):
    monkeypatch.delenv("GMX_LSTM_BUILD", raising=False)
    m = oracle.LstmModel()
    ppm, data = oracle.lstm_synth(12, seed=3)
    pred, act, ctx = m.run(ppm, data)
    for g in (gpu.LstmGroup(1), gpu.LstmGroup(1, shape=(50, 100, 0.03, 10.0))):   # gmx_lstm_create and _create_shaped
        g.set_weights(oracle.LstmModel().weights())
        P, A, Cx = run_gpu(gpu, g, [(ppm, data)], [12])
        assert np.array_equal(u32(P[0]), u32(pred)) and np.array_equal(A[0], act) and np.array_equal(Cx[0], ctx)
        assert g.any_launches == 0
        assert tuple(g.shape) == (50, 100, np.float32(0.03), np.float32(10.0))
        assert len(g.export_all()) == 1                                            # every surface: the group checkpoint too
        g.close()


def test_ragged_generation_per_byte_and_restart(gpu, oracle):
    shape = (65, 5, 0.01, 0.05)
    H, S = shape[1], 3
    lens = [0, H - 1, 2 * H + 1]
    N = max(lens) + 2 * H + 3
    streams = make_streams(oracle, S, N, seed=77)
    refs = [lsc.Ref(shape, seed=500 + s) for s in range(S)]
    g = gpu.LstmGroup(S, shape=shape)
    for s in range(S):
        g.set_weights(refs[s].weights(), stream=s)
    b = gpu.LstmBatch(g, N)
    for s, (ppm, data) in enumerate(streams):
        b.ppm[s], b.bytes[s] = ppm, data
    b.upload(N)
    # ---- one ragged launch: 0, horizon - 1 and 2 horizon + 1 bytes
    g.run_ragged(b, lens)
    b.download(max(lens))
    b.wait()
    pos = list(lens)
    for s in range(S):
        want = refs[s].run(streams[s][0][:lens[s]], streams[s][1][:lens[s]])
        assert_stream_equals_ref(g, s, refs[s], (b.predictions[s, :lens[s]], b.active[s, :lens[s]], b.contexts[s, :lens[s]]),
                                 want, "ragged")
    # ---- export -> reset -> import -> continue equals the uninterrupted run; a copy inside the group continues alike
    saved = [g.export(s) for s in range(S)]
    g.reset()
    assert g.export(2) != saved[2]
    for s in range(S):
        g.import_(*saved[s], stream=s)
        assert g.export(s) == saved[s], s
    g.copy_from(g, src_stream=2, stream=0)             # stream 0 now stands where stream 2 stands
    assert g.export(0) == saved[2]
    own = [2, 1, 2]                                    # whose input and whose restatement each stream follows from here

    def step(n, learn, where):
        for s in range(S):
            ppm, data = streams[own[s]]
            b.ppm[s, :n], b.bytes[s, :n] = ppm[pos[own[s]]:pos[own[s]] + n], data[pos[own[s]]:pos[own[s]] + n]
        b.upload(n)
        g.run(b, n, learn=learn)
        b.download(n)
        b.wait()
        for o in (1, 2):
            ppm, data = streams[o]
            want = refs[o].run(ppm[pos[o]:pos[o] + n], data[pos[o]:pos[o] + n], learn=learn)
            for s in range(S):
                if own[s] == o:
                    assert_stream_equals_ref(g, s, refs[o], (b.predictions[s, :n], b.active[s, :n], b.contexts[s, :n]),
                                             want, where)
            pos[o] += n

    step(2 * H, True, "after import / copy")           # two more backward passes
    # ---- generation: three bytes without Learn
    step(3, False, "learn off")
    # ---- the per-byte surface against the batched run: a second group, byte by byte
    g2 = gpu.LstmGroup(1, shape=shape)
    r2 = lsc.Ref(shape, seed=500 + 1)
    g2.set_weights(r2.weights())
    ppm1, data1 = streams[1]
    n1 = 3 * H + 1
    want = r2.run(ppm1[:n1], data1[:n1])
    last = 0
    for n in range(n1):
        probs, ctx = g2.forward(ppm1[n], last)
        assert np.array_equal(u32(probs), u32(want["probs"][n])) and ctx == want["ctx"][n], n
        g2.perceive(data1[n])
        last = int(data1[n])
    g3 = gpu.LstmGroup(1, shape=shape)
    g3.set_weights(lsc.Ref(shape, seed=500 + 1).weights())
    P, A, Cx = run_gpu(gpu, g3, [(ppm1[:n1], data1[:n1])], chunks_for(H, n1))
    assert np.array_equal(u32(P[0]), u32(want["pred"]))
    assert g2.export(0) == g3.export(0) == (r2.export_long(), r2.export_short())
    # ---- a copy between banks of different shapes is refused
    other = gpu.LstmGroup(1, shape=(65, 6, 0.01, 0.05))
    before = other.export(0)
    with pytest.raises(gpu.GmxError) as e:
        other.copy_from(g2)
    assert e.value.status == -1 and other.export(0) == before
    stock = gpu.LstmGroup(1)
    with pytest.raises(gpu.GmxError) as e:
        stock.copy_from(g2)
    assert e.value.status == -1
    for x in (b, g, g2, g3, other, stock):
        x.close()


def test_feed_into_mixer_and_indirect_batches(gpu, oracle):
    """gmx_lstm_feed of a (65, 5) bank: the mixers and the Indirect models that read the slot, its active bit and the
    two context columns from the device give what they give when the host writes the batch's own outputs there."""
    shape = (65, 5, 0.03, 10.0)
    _, z = goldenlib.load("ind_stock41")
    tabs = (z["ns_next"], z["rm_next"])
    models, topo = topology.stock_indirect(), topology.stock(90)
    K, N_IN, S, NB = len(models), 90, 3, 16
    T = 8 * NB
    LSTM_SLOT, IND_LSTM, MIX_LSTM = 1, 16, 22
    lg = gpu.LstmGroup(S, shape=shape)
    lb = gpu.LstmBatch(lg, NB)
    streams = make_streams(oracle, S, NB, seed=900)
    for s in range(S):
        lg.set_weights(lsc.Ref(shape, seed=40 + s).weights(), stream=s)
        lb.ppm[s], lb.bytes[s] = streams[s]
    lb.upload(NB)
    lg.run(lb, NB)
    lb.download(NB)
    lb.wait()
    lp, la, lc = lb.predictions.copy(), lb.active.copy(), lb.contexts.copy()
    rng = np.random.default_rng(5)
    recs = []
    for s in range(S):
        data = streams[s][1]
        bits = np.unpackbits(data.reshape(-1, 1), axis=1).reshape(-1)
        k = np.tile(np.arange(8), NB)
        prefix = np.repeat(data.astype(np.uint32), 8) >> (8 - k)
        bc = ((1 << k) | np.where(k > 0, prefix, 0)).astype(np.uint32) - 1
        ictx = np.repeat(rng.integers(0, 5000, (NB, K)).astype(np.uint32), 8, axis=0)
        mctx = np.repeat(rng.integers(0, 1 << 16, (NB, 33)).astype(np.uint32), 8, axis=0)
        pred, act, _, _ = oracle.synth(N_IN, 33, T, seed=70 + s, zero_mod=3)
        recs.append((bits, bc, ictx, mctx, pred, act))
    results = []
    for fed in (True, False):
        ig, mg = gpu.IndirectGroup(models, *tabs, S), gpu.MixerGroup(topo, S)
        ib, mb = gpu.IndirectBatch(ig, T), gpu.Batch(mg, T, outputs=True, mask=True)
        for s, (bits, bc, ictx, mctx, pred, act) in enumerate(recs):
            ictx, mctx, pred, act = ictx.copy(), mctx.copy(), pred.copy(), act.copy()
            if fed:      # the host leaves the LSTM's places empty
                ictx[:, IND_LSTM], mctx[:, MIX_LSTM], pred[:, LSTM_SLOT], act[:, LSTM_SLOT] = 0, 0, 0, 0
            else:        # ... or writes the batch's own outputs there
                ictx[:, IND_LSTM] = mctx[:, MIX_LSTM] = np.repeat(lc[s, :NB], 8)
                pred[:, LSTM_SLOT], act[:, LSTM_SLOT] = lp[s, :NB].reshape(-1), la[s, :NB].reshape(-1)
            ib.set_records(s, ictx, bc, bits)
            mb.set_records(s, pred, act, mctx, bits)
        ib.upload(T)
        mb.upload(T)
        if fed:
            lg.feed(lb, NB, mixer_batch=mb, slot=LSTM_SLOT, mixer_ctx_col=MIX_LSTM, ind_batch=ib, ind_ctx_col=IND_LSTM)
        ig.run(ib, T, learn=True)
        mg.run(mb, T, learn=True)
        ib.download(T)
        mb.download(T)
        ib.wait()
        mb.wait()
        results.append((ib.predictions.copy(), ib.active.copy(), mb.outputs.copy(), mb.p.copy(),
                        [ig.export(s) for s in range(S)], [mg.export(s) for s in range(S)]))
        for x in (ib, mb, ig, mg):
            x.close()
    a, b = results
    assert np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1])      # the Indirect models saw the column
    assert np.array_equal(u32(a[2]), u32(b[2])) and np.array_equal(u32(a[3]), u32(b[3]))  # the mixers: slot, bit, column
    assert a[4] == b[4] and a[5] == b[5]
    # and the column matters: the fed run differs from one that leaves the places empty
    assert len(np.unique(lc)) > 1 and la.any()
    lb.close()
    lg.close()


def test_refusals_leave_a_shaped_bank_untouched(gpu, oracle):
    shape = (65, 5, 0.03, 10.0)
    topo = topology.stock(90)
    S = 2
    g = gpu.LstmGroup(S, shape=shape)
    streams = make_streams(oracle, S, 7, seed=15)
    for s in range(S):
        g.set_weights(lsc.Ref(shape, seed=60 + s).weights(), stream=s)
    run_gpu(gpu, g, streams, [7])
    before = [g.export(s) for s in range(S)]
    mg = gpu.MixerGroup(topo, S)
    with pytest.raises(gpu.GmxError) as e:
        gpu.ChainStep(mg, None, g, lstm_slot=1, mixer_ctx_col=22)
    assert e.value.status == -1
    with pytest.raises(gpu.GmxError) as e:
        g.export_all()
    assert e.value.status == -1
    with pytest.raises(gpu.GmxError) as e:
        g.import_all(before)
    assert e.value.status == -1
    with pytest.raises(gpu.GmxError) as e:           # sections of the stock size are no more welcome
        g.import_all([(b"\0" * 5560200, b"\0" * 1458256)] * S)
    assert e.value.status == -1
    launches = g.any_launches
    assert [g.export(s) for s in range(S)] == before and g.any_launches == launches
    # forward / perceive on it never start a session: every call is a launch of the general kernel
    g.forward(streams[0][0][0], int(streams[0][1][6]))
    g.perceive(3)
    assert g.any_launches == launches + 2
    for x in (mg, g):
        x.close()
