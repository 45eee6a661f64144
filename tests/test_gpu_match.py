"""The Match-model banks (gmx_match.hip behind gmx_match_* of include/gmxmix.h) against what the reference recorded
(tests/golden/match_*.npz) and against tests/helpers/match_ref.c, which tests/test_match_ref.py pins to the same
fixtures.  Tolerance 0 everywhere: floats are compared as bit patterns."""
import numpy as np
import pytest

import match_common as mc
from gmix_amd import GmxError, Topology
from gmix_amd.match import stream_bits

pytestmark = pytest.mark.gpu
GMX_ERR_INVALID, GMX_ERR_FORMAT = -1, -6


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cap_for(f):
    return len(f.data) + 64


def run_chunks(g, b, streams, sizes):
    """streams: [(ctx, bc, bits)] of equal length; sizes: the chunk lengths in order.  -> slots, act, lm [S][T]..."""
    S, T, K = len(streams), len(streams[0][2]), g.K
    P = np.zeros((S, T, K), np.uint32)
    A = np.zeros((S, T, K), np.uint8)
    Lm = np.zeros((S, T), np.uint32)
    t0 = 0
    for n in sizes:
        for s, (ctx, bc, bits) in enumerate(streams):
            b.set_records(s, ctx[t0:t0 + n], bc[t0:t0 + n], bits[t0:t0 + n])
        b.upload(n)
        g.run(b, n)
        b.download(n)
        b.wait()
        P[:, t0:t0 + n] = u32(b.predictions[:, :n])
        A[:, t0:t0 + n] = b.active[:, :n]
        Lm[:, t0:t0 + n] = b.longest[:, :n]
        t0 += n
    assert t0 == T
    return P, A, Lm


def schedule(f, c):
    """Chunk lengths for a whole fixture.  c = 7, 64, 1000: chunks of c bits from the first bit to the last, so batches
    begin inside bytes at every phase.  c = 1: a launch per bit over the whole stream would take minutes, so the
    launch-per-bit windows lie over what the fixture's coverage counters point at -- the stream's first 2 100 bits, the
    beginning of its longest run of one byte value (same-entry write-then-read, end-of-history resets), the first match
    that stays at longest_match 7 for 48 bits (match_length_ 255; not in match_tiny), the first byte kept out of the
    history, the last 1 900 bits -- with chunks of 1 000 between them."""
    T = f.T
    if c > 1:
        return [c] * (T // c) + ([T % c] if T % c else [])
    d = f.data
    edges = np.flatnonzero(np.concatenate(([1], np.diff(d) != 0, [1])))
    run = edges[np.argmax(np.diff(edges))]
    marks = [8 * int(run)]
    skipped = np.flatnonzero((f.bc >= 127) & (f.lm >= 2))
    marks.append(int(skipped[0]))
    seven = np.flatnonzero(np.convolve(f.lm == 7, np.ones(48, int), "valid") == 48)
    if seven.size:
        marks.append(int(seven[0]))
    per_bit = np.zeros(T, bool)
    per_bit[:2100] = True
    per_bit[T - 1900:] = True
    for m in marks:
        per_bit[max(0, m - 300):m + 900] = True
    sizes, t = [], 0
    while t < T:
        if per_bit[t]:
            sizes.append(1)
        else:
            stop = t + np.argmax(per_bit[t:])  # (the last window reaches T, so there is always a next one)
            sizes.append(min(1000, int(stop) - t))
        t += sizes[-1]
    return sizes


def even_chunks(T, c):
    return [c] * (T // c) + ([T % c] if T % c else [])


@pytest.mark.parametrize("chunk", [1, 7, 64, 1000])
@pytest.mark.parametrize("name", mc.FIXTURES)
def test_fixture_through_the_batched_path(gpu, name, chunk):
    f = mc.fixture(name)
    S = 3 if name == "match_stock" else 2
    g = gpu.MatchGroup(f.models(), cap_for(f), S)
    b = gpu.MatchBatch(g, max(chunk, 1000))
    P, A, Lm = run_chunks(g, b, [(f.ctx, f.bc, f.bits)] * S, schedule(f, chunk))
    for s in range(S):
        bad = np.flatnonzero(mc.slot_hash(P[s]) != f.slot_hash)
        assert bad.size == 0, (s, "slot values differ first at bit", bad[:1])
        assert np.array_equal(A[s], f.act), s
        assert np.array_equal(Lm[s], f.lm), s
    for s in (0, S - 1):
        assert g.export(s) == (f.long, f.short)
    assert [g.memory_usage(k) for k in range(f.K)] == f.usage
    assert g.history_size(0) == len(f.data) - f.meta["not_pushed"]
    b.close()
    g.close()


@pytest.mark.parametrize("name", ["match_k8", "match_tiny"])
def test_nine_streams_ragged_from_other_offsets(gpu, name):
    """One full lane group plus one stream; stream s replays the fixture from byte 61 s; every launch gives each
    stream another length, 0 among them.  Checked against match_ref.c."""
    f = mc.fixture(name)
    S, NB, chunk = 9, 8 * 900, 700
    g = gpu.MatchGroup(f.models(), 1024, S)
    b = gpu.MatchBatch(g, chunk)
    rng = np.random.RandomState(3)
    recs, want = [], []
    for s in range(S):
        o = 8 * 61 * s
        recs.append((f.ctx[o:o + NB], f.bc[o:o + NB], f.bits[o:o + NB]))
        want.append(mc.Ref(f.models()))
    pos = np.zeros(S, np.int64)
    rounds = 0
    while (pos < NB).any():
        n = np.minimum(rng.choice([0, 1, 13, 64, 257, chunk], S), NB - pos).astype(np.uint64)
        if rounds == 0:
            n[1] = 0
        for s in range(S):
            k = int(n[s])
            b.set_records(s, recs[s][0][pos[s]:pos[s] + k], recs[s][1][pos[s]:pos[s] + k], recs[s][2][pos[s]:pos[s] + k])
        b.upload(int(n.max()))
        g.run_ragged(b, n)
        b.download(int(n.max()))
        b.wait()
        for s in range(S):
            k = int(n[s])
            wp, wa, wl = want[s].run(recs[s][0][pos[s]:pos[s] + k], recs[s][1][pos[s]:pos[s] + k],
                                     recs[s][2][pos[s]:pos[s] + k])
            assert np.array_equal(u32(b.predictions[s, :k]), wp), (s, rounds)
            assert np.array_equal(b.active[s, :k], wa), (s, rounds)
            assert np.array_equal(b.longest[s, :k], wl), (s, rounds)
        pos += n.astype(np.int64)
        rounds += 1
    for s in range(S):
        assert g.export(s) == want[s].export(), s
    b.close()
    g.close()


@pytest.mark.parametrize("name", ["match_k8", "match_tiny"])
def test_per_bit_surface_equals_the_batched_one(gpu, name):
    """2 000 bits from inside the fixture (matches, pushes and skipped pushes among them), the stream moving between
    gmx_match_forward / _learn and batches in the middle of bytes."""
    f = mc.fixture(name)
    T = 2000
    g = gpu.MatchGroup(f.models(), 1024, 2)
    b = gpu.MatchBatch(g, 512)
    ref = mc.Ref(f.models())
    wp, wa, wl = ref.run(f.ctx[:T], f.bc[:T], f.bits[:T])
    t = 0
    for kind, n in [("bit", 333), ("batch", 402), ("bit", 511), ("batch", 300), ("bit", 454)]:
        if kind == "batch":
            for s in range(2):
                b.set_records(s, f.ctx[t:t + n], f.bc[t:t + n], f.bits[t:t + n])
            b.upload(n)
            g.run(b, n)
            b.download(n)
            b.wait()
            for s in range(2):
                assert np.array_equal(u32(b.predictions[s, :n]), wp[t:t + n])
                assert np.array_equal(b.active[s, :n], wa[t:t + n])
                assert np.array_equal(b.longest[s, :n], wl[t:t + n])
        else:
            for i in range(t, t + n):
                for s in range(2):
                    p, a, lm = g.forward(f.ctx[i], f.bc[i], stream=s)
                    assert np.array_equal(u32(p), wp[i]) and np.array_equal(a, wa[i]) and lm == wl[i], (i, s)
                    g.learn(f.bits[i], stream=s)
        t += n
    assert t == T
    for s in range(2):
        assert g.export(s) == ref.export()
        assert np.array_equal(u32(g.slot_values(s)[0]), u32(ref.slots()[0])) and g.slot_values(s)[1] == ref.slots()[1]
    with pytest.raises(GmxError):
        g.learn(0, stream=0)  # no forward before it
    b.close()
    g.close()


def test_into_a_mixer_batch(gpu, oracle):
    """gmx_match_run writes predictions, mask bits and longest_match into a mixer batch's device records; everything
    else in them keeps the host's pattern, and the mixers then compute what the oracle computes from the merged
    records."""
    f = mc.fixture("match_k8")
    N, T, S = 40, 1600, 2
    mixers = [(0, 8, 0.005), (0, 256, 0.004), (0, 8, 0.0005), (1, 8, 0.0008), (1, 256, 0.003), (2, 1, 0.0005)]
    cols = [0, 2, 3]  # the gate contexts that are longest_match
    topo = Topology(N, mixers, (1,))
    slots = [3, 31, 32, 33, 39, 0, 17, 8]  # both mask words, their first and last bits
    models = [(t, f.limit, sl) for t, sl in zip(f.tables, slots)]
    g = gpu.MatchGroup(models, 1024, S)
    mg = gpu.MixerGroup(topo, S)
    b = gpu.MatchBatch(g, T)
    mb = gpu.Batch(mg, T, outputs=True, mask=True)
    want = []
    for s in range(S):
        o = 8 * 500 * s
        ctx, bc, bits = f.ctx[o:o + T], f.bc[o:o + T], f.bits[o:o + T]
        other, act_o, mctx, _ = oracle.synth(N, len(mixers), T, seed=40 + s, ctx_mode=2, zero_mod=4)
        act_o[:, slots] = 1 - (np.arange(T)[:, None] + np.arange(8)[None, :]) % 2  # a pattern the run must replace
        b.set_records(s, ctx, bc, bits)
        mb.set_records(s, other, act_o, mctx, bits)
        wp, wa, wl = mc.Ref(f.models()).run(ctx, bc, bits)
        pred, act, mc2 = other.copy(), act_o.copy(), mctx.copy()
        pred[:, slots] = wp.view(np.float32)
        act[:, slots] = wa
        mc2[:, cols] = wl[:, None]
        om = oracle.Bank(N, topo.skip, topo.mixers)
        want.append((wp, wa, wl) + om.run(pred, act, mc2, bits))
    b.upload(T)
    mb.upload(T)
    g.run(b, T, into=mb, ctx_columns=cols)
    mg.run(mb, T, learn=True)
    b.download(T)
    mb.download(T)
    b.wait()
    mb.wait()
    for s in range(S):
        wp, wa, wl, p_ref, o_ref = want[s]
        assert np.array_equal(u32(b.predictions[s]), wp) and np.array_equal(b.active[s], wa)
        assert np.array_equal(b.longest[s], wl)
        assert np.array_equal(u32(mb.outputs[s, :T]), u32(o_ref)), s
        assert np.array_equal(u32(mb.p[s, :T]), u32(p_ref)), s
    for x in (b, mb, g, mg):
        x.close()


@pytest.mark.parametrize("name", mc.FIXTURES)
def test_checkpoint_round_trips(gpu, name):
    """export -> reset -> import -> continue, copy -> continue, and sections exchanged with match_ref.c, all inside a
    byte; the end state is the fixture's."""
    f = mc.fixture(name)
    cut = 8 * (len(f.data) // 2) + 3
    g = gpu.MatchGroup(f.models(), cap_for(f), 3)
    b = gpu.MatchBatch(g, 4096)
    first = even_chunks(cut, 4096)
    rest = even_chunks(f.T - cut, 4096)
    P0, A0, L0 = run_chunks(g, b, [(f.ctx[:cut], f.bc[:cut], f.bits[:cut])] * 3, first)
    ref = mc.Ref(f.models())
    ref.run(f.ctx[:cut], f.bc[:cut], f.bits[:cut])
    sec = g.export(0)
    assert sec == ref.export()          # a section of the device is what match_ref.c writes ...
    slots, new_bit = g.slot_values(0)
    g.reset()
    assert g.history_size(0) == 0
    g.import_(*sec, stream=0)           # ... stream 0: its own section back after a reset
    g.set_slot_values(slots, new_bit, stream=0)
    g.copy_from(g, src_stream=0, dst_stream=1)  # stream 1: a copy of stream 0
    g.import_(*ref.export(), stream=2)  # stream 2: the section match_ref.c wrote
    g.set_slot_values(*ref.slots(), stream=2)
    back = mc.Ref(f.models())
    back.import_(*sec)                  # and match_ref.c reads the device's
    assert back.export() == sec
    tail = (f.ctx[cut:], f.bc[cut:], f.bits[cut:])
    P1, A1, L1 = run_chunks(g, b, [tail] * 3, rest)
    for s in range(3):
        assert (mc.slot_hash(np.concatenate([P0[s], P1[s]])) == f.slot_hash).all(), s
        assert np.array_equal(np.concatenate([A0[s], A1[s]]), f.act), s
        assert np.array_equal(np.concatenate([L0[s], L1[s]]), f.lm), s
        assert g.export(s) == (f.long, f.short), s
    b.close()
    g.close()


def _sections(gpu):
    """A bank of two sparse models and a dense one after 3 000 bits, and its sections."""
    f = mc.fixture("match_k8")
    models = [(f.tables[4], f.limit), (f.tables[7], f.limit), (f.tables[0], f.limit)]
    g = gpu.MatchGroup(models, 1024, 1)
    b = gpu.MatchBatch(g, 3000)
    b.set_records(0, f.ctx[:3000, [4, 7, 0]], f.bc[:3000], f.bits[:3000])
    b.upload(3000)
    g.run(b, 3000)
    b.close()
    return g, models, g.export(0)


def test_import_rejects_bad_sections_and_leaves_the_bank_alone(gpu):
    import struct
    g, models, (lb, sb) = _sections(gpu)
    hs = struct.unpack_from("<Q", lb, 0)[0]
    p0 = 8 + hs
    cnt0 = struct.unpack_from("<I", lb, p0)[0]
    assert 2 <= cnt0 < (5.0 / 9.0) * models[0][0]  # model 0 is sparse, with records to damage
    rec = p0 + 4
    bad = {}
    x = bytearray(lb)
    struct.pack_into("<I", x, rec + 4, hs)  # a pointer at the history's size
    bad["pointer"] = (bytes(x), sb)
    x = bytearray(lb)
    x[rec:rec + 9], x[rec + 9:rec + 18] = lb[rec + 9:rec + 18], lb[rec:rec + 9]  # keys descend
    bad["descending"] = (bytes(x), sb)
    x = bytearray(lb)
    x[rec + 8] = 1  # a fifth pointer byte
    bad["fifth byte"] = (bytes(x), sb)
    # the count says sparse, the body is the dense one
    dense_body = bytearray(5 * models[0][0])
    body_end = rec + 9 * cnt0
    bad["wrong branch"] = (lb[:rec] + bytes(dense_body) + lb[body_end:], sb)
    # the count says dense (every entry valid), the body is the sparse one
    x = bytearray(lb)
    struct.pack_into("<I", x, p0, models[0][0])
    bad["count"] = (bytes(x), sb)
    bad["truncated"] = (lb[:-5], sb)
    bad["truncated short"] = (lb, sb[:-1])
    x = bytearray(sb)
    x[9] = 3  # bit_pos_ neither 0 nor a power of two
    bad["bit_pos"] = (lb, bytes(x))
    x = bytearray(lb)
    struct.pack_into("<Q", x, 0, 5000)  # a history beyond the capacity
    bad["capacity"] = (bytes(x), sb)
    for what, (l, s) in bad.items():
        with pytest.raises(GmxError) as e:
            g.import_(l, s)
        assert e.value.status == GMX_ERR_FORMAT, what
        assert g.export(0) == (lb, sb), what
    g.import_(lb, sb)
    assert g.export(0) == (lb, sb)
    g.close()


def test_history_capacity_is_checked_before_anything_is_queued(gpu):
    """history_capacity 64 and 80 bytes that match nothing: GMX_ERR_INVALID, state unchanged; 64 bytes fit."""
    data = ((np.arange(80) * 37 + 11) % 251).astype(np.uint8)  # 80 different bytes
    bits, bc = stream_bits(data)
    ctx = np.repeat(np.concatenate(([0], data[:-1])).astype(np.uint32), 8)[:, None]
    g = gpu.MatchGroup([(256, 400)], 64, 1)
    b = gpu.MatchBatch(g, 640)
    b.set_records(0, ctx, bc, bits)
    b.upload(640)
    before = g.export(0)
    with pytest.raises(GmxError) as e:
        g.run(b, 640)
    assert e.value.status == GMX_ERR_INVALID
    assert g.export(0) == before and g.history_size(0) == 0
    g.run(b, 512)  # 64 bytes fit ...
    assert g.history_size(0) == 64
    full = g.export(0)
    b.set_records(0, ctx[512:520], bc[512:520], bits[512:520])
    b.upload(8)
    with pytest.raises(GmxError) as e:
        g.run(b, 8)  # ... the 65th does not, even after the true sizes have been fetched
    assert e.value.status == GMX_ERR_INVALID
    assert g.export(0) == full
    b.close()
    g.close()
