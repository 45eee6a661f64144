"""The PPMd bank (gmx_ppmd, gmx_ppmd.hip) against the host build of the same header (tests/cpp/test_ppmd.cpp), which
tests/test_ppmd_cpu.py pins to the reference's own ModPPMD (tests/golden/ppmd_trace.npz).  Tolerance 0 everywhere:
floats are compared as uint32."""
import ctypes as C

import numpy as np
import pytest

import ppmd_common as pc
from gmix_amd import GmxError, topology
from gmix_amd.bank import PPMD_PPM, PPMD_PREDICTIONS, PPMD_USED

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5
CHUNK = 4096


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def host_records(data, order=pc.ORDER, arena_mb=pc.ARENA_MB):
    """The restatement over one stream's bytes as batch records -> (results, restores, memory_usage)."""
    m = pc.HostModel(order, arena_mb)
    r = m.records(data)
    out = (r, m.restores, m.memory_usage)
    m.close()
    return out


def assert_chunk(b, s, n, want, at, what):
    """Records [0, n) of stream s of batch b against records [at, at + n) of the restatement."""
    sl = slice(at, at + n)
    assert np.array_equal(u32(b.ppm[s, :n]), want["ppm"][sl]), (what, s, at, "ppm")
    assert np.array_equal(u32(b.predictions[s, :n]), want["pred"][sl]), (what, s, at, "predictions")
    assert np.array_equal(b.active[s, :n], want["active"][sl]), (what, s, at, "active")
    assert np.array_equal(b.used[s, :n], want["used"][sl]), (what, s, at, "used")


def run_counts(g, b, streams, counts, done):
    """One launch: counts[s] further bytes of streams[s] from done[s] on (a list: ragged; an int: uniform)."""
    ragged = not np.isscalar(counts)
    c = list(counts) if ragged else [counts] * g.S
    for s, d in enumerate(streams):
        b.bytes[s, :c[s]] = d[done[s]:done[s] + c[s]]
    b.upload(max(c))
    g.run(b, np.array(c, np.uint64) if ragged else counts)
    b.download(max(c))
    b.wait()
    return c


def test_flushes(gpu):
    """Three streams of different lengths through ragged launches of at most 4 096 bytes, two of them across a model
    flush: sym3 runs its arena full, rand256 makes the allocator give up with the arena half used."""
    names = ("sym3", "rand256", "noisy500")
    streams = [pc.case_bytes(n) for n in names]
    want = [host_records(d) for d in streams]
    # the restatement flushes inside the run (before the kernel is looked at)
    assert [w[1] for w in want] == [1, 1, 0]
    for (r, _, _), n in zip(want[:2], names):
        fl = pc.flushes(r["used"])
        assert len(fl) == 1 and 256 < fl[0] < len(r["used"]) - 256, (n, fl)
    S = len(streams)
    g = gpu.PpmdGroup(S, pc.ORDER, pc.ARENA_MB)
    b = gpu.PpmdBatch(g, CHUNK)
    done = [0] * S
    launches = 0
    while any(done[s] < len(streams[s]) for s in range(S)):
        c = run_counts(g, b, streams, [min(CHUNK, len(streams[s]) - done[s]) for s in range(S)], done)
        launches += 1
        for s in range(S):
            assert_chunk(b, s, c[s], want[s][0], done[s], "flushes")
            done[s] += c[s]
    assert launches == 15 and g.launches() == launches
    for s in range(S):
        assert g.restores(s) == want[s][1] and g.memory_usage(s) == want[s][2], s
    assert g.restores(S) == -1 and g.memory_usage(-1) == 0
    b.close()
    g.close()


@pytest.mark.parametrize("order", [4, 64, 20])
def test_order_range_tiny_launches_and_reset(gpu, order):
    """The ends of the order range (the depth of the explicit stacks) and the stock order; launches of 1, 2, 255 and 257
    bytes, a ragged one of 0 / 1 / 7 / 300 / 300, and a stream that is reset in the middle."""
    names = ("rand256_o4", "sym3_o64", "e-run", "abcd", "abcd")
    streams = [pc.case_bytes(n, 3000) for n in names]
    S = len(streams)
    g = gpu.PpmdGroup(S, order, pc.ARENA_MB)
    b = gpu.PpmdBatch(g, 300)
    plan = [1, 2, 255, 257, [0, 1, 7, 300, 300], "reset", 300, [300, 0, 3, 1, 64]]
    total = [0] * S
    for step in plan:
        if step != "reset":
            c = step if not np.isscalar(step) else [step] * S
            total = [t + k for t, k in zip(total, c)]
    want = [host_records(d[:total[s]], order)[0] for s, d in enumerate(streams)]
    done = [0] * S
    fresh_from = None
    for step in plan:
        if step == "reset":
            g.reset(4)
            fresh_from = done[4]
            want[4] = host_records(streams[4][fresh_from:total[4]], order)[0]    # a fresh stream from there
            continue
        c = run_counts(g, b, streams, step, done)
        for s in range(S):
            at = done[s] - (fresh_from if s == 4 and fresh_from is not None else 0)
            assert_chunk(b, s, c[s], want[s], at, ("order", order, step))
            done[s] += c[s]
    assert done == total and fresh_from == 815
    for s in range(S):
        assert g.restores(s) == 0
        assert g.memory_usage(s) == int(want[s]["used"][-1]), s
    b.close()
    g.close()


def test_surfaces_agree(gpu):
    """The per-byte surface (the caller hands in the byte coded last) against records of the same bytes on a second
    bank, one stream sitting out every third step; then the banks swap surfaces."""
    names = ("noisy500", "abcd", "e-run")
    N, M = 400, 100
    x = [pc.case_bytes(n, N + M) for n in names]
    S = len(x)
    a, r = gpu.PpmdGroup(S, pc.ORDER, pc.ARENA_MB), gpu.PpmdGroup(S, pc.ORDER, pc.ARENA_MB)
    rb, ab = gpu.PpmdBatch(r, N), gpu.PpmdBatch(a, M + 1)
    for s in range(S):
        rb.bytes[s, :N] = x[s][:N]
    rb.upload(N)
    r.run(rb, N)
    rb.download(N)
    rb.wait()
    rec_ppm = u32(rb.ppm[:, :N]).copy()
    # record n follows UpdateByte(x[n - 1]) (0 for n = 0): the steps hand in exactly those
    k = [0] * S
    step = launched = 0
    while min(k) < N:
        take = np.array([1 if k[s] < N and not (s == 1 and step % 3 == 2) else 0 for s in range(S)], np.uint8)
        last = np.array([(x[s][k[s] - 1] if k[s] else 0) if take[s] else 0xAA for s in range(S)], np.uint8)
        before = u32(a.step_ppm).copy()
        launched += int(take.any())
        ppm = u32(a.step(last, take))
        for s in range(S):
            if take[s]:
                assert np.array_equal(ppm[s], rec_ppm[s, k[s]]), (s, k[s])
                k[s] += 1
            else:
                assert np.array_equal(ppm[s], before[s]), (s, "a stream that sits out keeps its row")
        step += 1
    assert step > N and a.launches() == launched >= N
    for s in range(S):
        assert a.memory_usage(s) == r.memory_usage(s) == int(rb.used[s, N - 1])
    # swap.  `a` has prepared byte N - 1 and owes nothing: its first record is that byte, prepared again without an
    # update; `r` owes byte N - 1, which its first step hands in.
    for s in range(S):
        ab.bytes[s, :M + 1] = x[s][N - 1:N + M]
    ab.upload(M + 1)
    a.run(ab, M + 1)
    ab.download(M + 1)
    ab.wait()
    assert np.array_equal(u32(ab.ppm[:, 0]), rec_ppm[:, N - 1])
    assert np.array_equal(ab.used[:, 0], rb.used[:, N - 1])
    assert np.array_equal(u32(ab.predictions[:, 0]), u32(rb.predictions[:, N - 1]))
    for n in range(M):
        ppm = u32(r.step(np.array([x[s][N - 1 + n] for s in range(S)], np.uint8)))
        assert np.array_equal(ppm, u32(ab.ppm[:, n + 1])), n
    want = [host_records(x[s])[0] for s in range(S)]
    for s in range(S):
        assert np.array_equal(u32(ab.ppm[s, 1:]), want[s]["ppm"][N:]), s
        assert np.array_equal(u32(ab.predictions[s, 1:]), want[s]["pred"][N:]), s
        assert np.array_equal(ab.used[s, 1:], want[s]["used"][N:]), s
        assert a.memory_usage(s) == r.memory_usage(s)
    for h in (rb, ab, a, r):
        h.close()


def test_arena_size_matters_only_after_a_flush(gpu):
    """On the device: 1 MB against 8 MB arenas give the same floats and the same `used`."""
    d = pc.case_bytes("noisy500", 20000)
    got = []
    for mb in (1, 8):
        g = gpu.PpmdGroup(1, pc.ORDER, mb)
        assert g.bank_bytes >= mb << 20
        b = gpu.PpmdBatch(g, CHUNK)
        ppm, used = [], []
        for at in range(0, len(d), CHUNK):
            n = min(CHUNK, len(d) - at)
            b.bytes[0, :n] = d[at:at + n]
            b.upload(n)
            g.run(b, n)
            b.download(n, PPMD_PPM | PPMD_USED)
            b.wait()
            ppm.append(u32(b.ppm[0, :n]).copy())
            used.append(b.used[0, :n].copy())
        assert g.restores(0) == 0
        got.append((np.concatenate(ppm), np.concatenate(used)))
        b.close()
        g.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    want = host_records(d)[0]
    assert np.array_equal(got[0][0], want["ppm"]) and np.array_equal(got[0][1], want["used"])


def test_feed_into_lstm_and_mixer_batches(gpu, oracle):
    """gmx_ppmd_feed: the LSTM that reads ppm from the device and the mixers that read slot 0 and its active bit from
    the device give what they give when the host writes the bank's downloaded outputs there."""
    S, NB, SLOT, N_IN = 2, 64, 0, 90
    T = 8 * NB
    topo = topology.stock(N_IN)
    data = [pc.case_bytes("noisy500", NB), pc.case_bytes("abcd", NB)]
    pg = gpu.PpmdGroup(S, pc.ORDER, pc.ARENA_MB)
    pb = gpu.PpmdBatch(pg, NB)
    for s in range(S):
        pb.bytes[s] = data[s]
    pb.upload(NB)
    pg.run(pb, NB)
    pb.download(NB)
    pb.wait()
    ppm, pp, pa = pb.ppm.copy(), pb.predictions.copy(), pb.active.copy()
    for s in range(S):
        want = host_records(data[s])[0]
        assert np.array_equal(u32(ppm[s]), want["ppm"]) and np.array_equal(u32(pp[s]), want["pred"])
    assert pa.any() and len(np.unique(u32(pp))) > 8
    rng = np.random.default_rng(11)
    w0 = ((rng.random((3, 50, 563), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
    recs = []
    for s in range(S):
        bits = np.unpackbits(data[s].reshape(-1, 1), axis=1).reshape(-1)
        mctx = np.repeat(rng.integers(0, 1 << 16, (NB, 33)).astype(np.uint32), 8, axis=0)
        pred, act, _, _ = oracle.synth(N_IN, 33, T, seed=70 + s, zero_mod=3)
        recs.append((bits, mctx, pred, act))
    results = []
    for mode in ("fed", "host", "empty"):
        lg, mg = gpu.LstmGroup(S), gpu.MixerGroup(topo, S)
        lb, mb = gpu.LstmBatch(lg, NB), gpu.Batch(mg, T, outputs=True, mask=True)
        for s, (bits, mctx, pred, act) in enumerate(recs):
            lg.set_weights(w0, stream=s)
            pred, act = pred.copy(), act.copy()
            lb.bytes[s] = data[s]
            if mode == "host":      # the host writes the bank's own outputs there
                lb.ppm[s] = ppm[s]
                pred[:, SLOT], act[:, SLOT] = pp[s].reshape(-1), pa[s].reshape(-1)
            else:                   # ... or leaves the places empty
                lb.ppm[s] = 0
                pred[:, SLOT], act[:, SLOT] = 0, 0
            mb.set_records(s, pred, act, mctx, bits)
        lb.upload(NB)
        mb.upload(T)
        if mode == "fed":
            pg.feed(pb, NB, lstm_batch=lb, mixer_batch=mb, slot=SLOT)
        lg.run(lb, NB)
        mg.run(mb, T, learn=True)
        lb.download(NB)
        mb.download(T)
        lb.wait()
        mb.wait()
        results.append((u32(lb.predictions).copy(), lb.contexts.copy(), u32(mb.outputs).copy(), u32(mb.p).copy(),
                        [lg.export(s) for s in range(S)], [mg.export(s) for s in range(S)]))
        for h in (lb, mb, lg, mg):
            h.close()
    fed, host, empty = results
    for i in range(4):
        assert np.array_equal(fed[i], host[i]), i
    assert fed[4] == host[4] and fed[5] == host[5]
    # the fed places matter
    assert not np.array_equal(fed[0], empty[0]) and not np.array_equal(fed[3], empty[3])
    assert fed[4] != empty[4] and fed[5] != empty[5]
    # either target alone
    lg, mg = gpu.LstmGroup(S), gpu.MixerGroup(topo, S)
    lb, mb = gpu.LstmBatch(lg, NB), gpu.Batch(mg, T, outputs=True, mask=True)
    pg.feed(pb, NB, lstm_batch=lb)
    pg.feed(pb, NB // 2, mixer_batch=mb, slot=89)
    pg.sync()
    for h in (lb, mb, lg, mg, pb, pg):
        h.close()


def test_refusals_leave_the_bank_untouched(gpu):
    S, NB = 2, 16
    data = [pc.case_bytes("noisy500", 3 * NB), pc.case_bytes("abcd", 3 * NB)]
    g, twin, other = gpu.PpmdGroup(S, pc.ORDER, 1), gpu.PpmdGroup(S, pc.ORDER, 1), gpu.PpmdGroup(3, pc.ORDER, 1)
    b, tb, ob = gpu.PpmdBatch(g, NB), gpu.PpmdBatch(twin, NB), gpu.PpmdBatch(other, NB)
    topo = topology.stock(90)
    mg, mg3 = gpu.MixerGroup(topo, S), gpu.MixerGroup(topo, 3)
    mb, mb_short = gpu.Batch(mg, 8 * NB, mask=True), gpu.Batch(mg, 8 * NB - 1, mask=True)
    mb_plain, mb3 = gpu.Batch(mg, 8 * NB, mask=False), gpu.Batch(mg3, 8 * NB, mask=True)
    lg3 = gpu.LstmGroup(3)
    lb3 = gpu.LstmBatch(lg3, NB)

    def both(n0):
        for grp, bat in ((g, b), (twin, tb)):
            for s in range(S):
                bat.bytes[s] = data[s][n0:n0 + NB]
            bat.upload(NB)
            grp.run(bat, NB)
            bat.download(NB)
            bat.wait()
        assert np.array_equal(u32(b.ppm), u32(tb.ppm)) and np.array_equal(b.used, tb.used)
        assert np.array_equal(u32(b.predictions), u32(tb.predictions)) and np.array_equal(b.active, tb.active)

    both(0)
    before = g.launches()
    L = g.L
    h = C.c_void_p()
    for order, arena_mb in ((1, 1), (65, 1), (20, 0), (20, 4096)):
        assert L.gmx_ppmd_create(C.byref(h), 1, order, arena_mb, 0) == INVALID and not h.value
    assert L.gmx_ppmd_create(C.byref(h), 1, 20, 1, 99) == INVALID and not h.value
    refused = [
        lambda: g.run(b, NB + 1),
        lambda: g.run(b, np.array([1, NB + 1], np.uint64)),
        lambda: g.run(ob, 1),                                             # another bank's batch
        lambda: g.feed(b, NB + 1, mixer_batch=mb, slot=0),
        lambda: g.feed(b, NB),                                            # no target
        lambda: g.feed(b, NB, mixer_batch=mb3, slot=0),                   # stream counts differ
        lambda: g.feed(b, NB, lstm_batch=lb3),
        lambda: g.feed(b, NB, mixer_batch=mb, slot=90),                   # a slot outside the record
        lambda: g.feed(b, NB, mixer_batch=mb, slot=-1),
        lambda: g.feed(b, NB, mixer_batch=mb_plain, slot=0),              # no mask column
        lambda: g.feed(b, NB, mixer_batch=mb_short, slot=0),              # max_bits < 8 * n_bytes
        lambda: g.feed(ob, NB, mixer_batch=mb, slot=0),
        lambda: b.download(NB, 0),
        lambda: b.download(NB, 8),
        lambda: b.download(NB + 1, PPMD_PREDICTIONS),
        lambda: b.upload(NB + 1),
        lambda: g.reset(S),
        lambda: g.reset(-2),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(GmxError) as e:
            call()
        assert e.value.status == INVALID, i
    with pytest.raises(GmxError) as e:
        g.step_wait()
    assert e.value.status == STATE
    g.step_launch(np.zeros(S, np.uint8), np.zeros(S, np.uint8))           # nobody takes: no launch
    with pytest.raises(GmxError) as e:
        g.step_launch(np.zeros(S, np.uint8))
    assert e.value.status == STATE
    g.step_wait()
    assert g.launches() == before
    both(NB)
    both(2 * NB)
    assert g.launches() == before + 2 == twin.launches()
    for x in (lb3, lg3, mb, mb_short, mb_plain, mb3, mg, mg3, b, tb, ob, g, twin, other):
        x.close()
