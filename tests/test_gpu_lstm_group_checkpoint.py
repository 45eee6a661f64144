"""The checkpoint of a whole LSTM group on the device (gmx_lstm_group_export / gmx_lstm_group_import, gmx_lstm_ckpt.hip)
against the per-stream calls gmx_lstm_export / gmx_lstm_import -- which tests/test_gpu_lstm.py pins to the oracle and
the reference's files -- and against those files directly: every comparison on bytes or uint32 patterns, tolerance 0."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LB, SB = 5560200, 1458256
INVALID, FORMAT = -1, -6


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def learn(gpu, g, streams, lengths):
    """Stream s of g takes the first lengths[s] bytes of streams[s] = (ppm, data) in one run_ragged."""
    n = max(max(lengths), 1)
    b = gpu.LstmBatch(g, n)
    b.ppm[:] = 1.0 / 256
    b.bytes[:] = 0
    for s, (ppm, data) in enumerate(streams):
        k = lengths[s]
        b.ppm[s, :k] = ppm[:k]
        b.bytes[s, :k] = data[:k]
    b.upload(n)
    g.run_ragged(b, lengths, learn=True)
    b.download(n)
    b.wait()
    out = (b.predictions.copy(), b.active.copy(), b.contexts.copy())
    b.close()
    return out


def seeded_group(gpu, oracle, n, seed0):
    """n streams, each with the reference's initial weights after another srand()."""
    g = gpu.LstmGroup(n)
    for s in range(n):
        g.set_weights(oracle.LstmModel(srand_seed=seed0 + s).weights(), stream=s)
    return g


def vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raw_export(g, first, count, lbuf, lcap, sbuf, scap, strides=True):
    nl, ns = C.c_size_t(0), C.c_size_t(0)
    rc = g.L.gmx_lstm_group_export(g.h, first, count, vp(lbuf), lcap, vp(sbuf), scap,
                                   C.byref(nl) if strides else None, C.byref(ns) if strides else None)
    return rc, nl.value, ns.value


def raw_import(g, first, count, lbytes, sbytes):
    a = np.frombuffer(lbytes or b"\0", np.uint8)
    b = np.frombuffer(sbytes or b"\0", np.uint8)
    return g.L.gmx_lstm_group_import(g.h, first, count, vp(a), len(lbytes), vp(b), len(sbytes))


class stage_bytes:
    """GMX_CKPT_STAGE_BYTES, read by the library at every call."""

    def __init__(self, v):
        self.v = str(int(v))

    def __enter__(self):
        self.old = os.environ.get("GMX_CKPT_STAGE_BYTES")
        os.environ["GMX_CKPT_STAGE_BYTES"] = self.v

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("GMX_CKPT_STAGE_BYTES", None)
        else:
            os.environ["GMX_CKPT_STAGE_BYTES"] = self.old


LENGTHS = [230, 0, 37, 1, 130]   # two backward passes and 30 bytes; untouched; inside the first epoch; one byte; one pass


@pytest.fixture(scope="module")
def five(gpu, oracle):
    """Five streams of different initial weights and lengths, and their per-stream exports (computed once, read only)."""
    g = seeded_group(gpu, oracle, 5, 100)
    streams = [oracle.lstm_synth(max(LENGTHS), seed=31 + s, mask=(255, 255, 15, 127, 63)[s]) for s in range(5)]
    learn(gpu, g, streams, LENGTHS)
    ref = [g.export(i) for i in range(5)]
    yield g, ref
    g.close()


def test_export_all_equals_per_stream_exports(five):
    g, ref = five
    got = g.export_all()
    assert len(got) == 5
    for i in range(5):
        assert len(got[i][0]) == LB and len(got[i][1]) == SB
        assert got[i][0] == ref[i][0], ("long", i)
        assert got[i][1] == ref[i][1], ("short", i)
    # no two streams share weights or a length: every section is its own
    for i in range(5):
        for j in range(i + 1, 5):
            assert ref[i][0] != ref[j][0] and ref[i][1] != ref[j][1], (i, j)


def test_export_all_gives_the_references_bytes(gpu, oracle):
    import goldenlib
    meta, z = goldenlib.load("lstm_short")
    kw = meta["synth"]
    N = meta["bytes"]
    streams = [oracle.lstm_synth(N, seed=17, mask=63),
               oracle.lstm_synth(N, seed=kw.get("seed", 0), mask=kw.get("mask", 255)),
               oracle.lstm_synth(N, seed=18, mask=255)]
    m = oracle.LstmModel()
    assert m.weights_hash() == meta["init_weights_hash"]
    g = gpu.LstmGroup(3)
    for s in range(3):
        g.set_weights(m.weights(), stream=s)
    P, A, Cx = learn(gpu, g, streams, [N, N, N])
    D = meta["dump"]
    assert np.array_equal(u32(P[1, :D]), z["pred"]) and np.array_equal(A[1, :D], z["active"])
    got = g.export_all()
    lng, sh = got[1]
    assert len(sh) == meta["short_size"] and oracle.fnv64_bytes(sh) == meta["short_hash"]
    assert oracle.fnv64_bytes(lng) == meta["long_hash"]
    for other in (0, 2):
        assert got[other][0] != lng and got[other][1] != sh
    assert got[0] != got[2]
    g.close()


def test_every_range_header_mode_in_one_group(gpu, oracle):
    N = 131
    ppm, data = oracle.lstm_synth(N, seed=9, mask=127)
    m0 = oracle.LstmModel()
    w = m0.weights()
    g = gpu.LstmGroup(5)
    for s in range(3):
        g.set_weights(w, stream=s)
    # 0: untouched.  1: at a byte boundary
    learn(gpu, g, [(ppm, data)] * 5, [0, 37, 0, 0, 0])
    # 2: between forward and perceive
    g.forward(ppm[0], 0, stream=2)
    # 3: just imported from an oracle file taken inside a byte, its range wherever the caller's coder stood
    m = oracle.LstmModel()
    m.run(ppm[:130], data[:130])
    m.predict_byte(ppm[130], int(data[129]))
    sh = bytearray(m.export_short())
    for i, v in enumerate((231, 200, 176)):
        sh[4 * i:4 * i + 4] = v.to_bytes(4, "little")
    inside = (m.export_long(), bytes(sh))
    g.import_(*inside, stream=3)
    # 4: a copy of that one
    g.copy_from(g, src_stream=3, stream=4)
    got = g.export_all()
    ref = [g.export(i) for i in range(5)]
    assert got == ref
    assert got[0] == (m0.export_long(), m0.export_short())
    assert got[3] == inside and got[4] == inside
    tmb = [[int.from_bytes(s[1][4 * i:4 * i + 4], "little") for i in range(3)] for s in got]
    b = int(data[36])
    assert tmb == [[255, 127, 0], [b | 1, b & ~1, b & ~1], [255, 127, 0], [231, 200, 176], [231, 200, 176]]
    assert got[2][1] != got[0][1]            # (the forward moved the state, the header alone did not say so)
    g.close()


def test_halves(five):
    g, ref = five
    only_short = g.export_all(long=False)
    only_long = g.export_all(short=False)
    assert only_short == [(None, r[1]) for r in ref]
    assert only_long == [(r[0], None) for r in ref]
    # the raw call: a half passed as NULL, with a cap, is not touched -- there is nothing it could touch -- and the other
    # half arrives in full
    lbuf = np.full(2 * LB, 0xA5, np.uint8)
    sbuf = np.full(2 * SB, 0xA5, np.uint8)
    assert raw_export(g, 1, 2, None, 2 * LB, sbuf, 2 * SB)[0] == 0
    assert sbuf.tobytes() == ref[1][1] + ref[2][1] and np.all(lbuf == 0xA5)
    sbuf[:] = 0xA5
    assert raw_export(g, 1, 2, lbuf, 2 * LB, None, 2 * SB, strides=False)[0] == 0
    assert lbuf.tobytes() == ref[1][0] + ref[2][0] and np.all(sbuf == 0xA5)


def test_ranges_sizing_and_capacity(gpu, five):
    g, ref = five
    S = g.S
    for first, count in ((0, 1), (4, 1), (1, 3), (2, 2), (0, 5)):
        assert g.export_all(first, count) == ref[first:first + count], (first, count)
    assert g.export_all(0, 0) == [] and g.export_all(S, 0) == []
    lbuf = np.full(LB + 64, 0x5A, np.uint8)
    sbuf = np.full(SB + 64, 0x5A, np.uint8)
    for first, count in ((-1, 1), (0, -1), (0, S + 1), (S, 1), (S + 1, 0)):
        rc, nl, ns = raw_export(g, first, count, lbuf, lbuf.size, sbuf, sbuf.size)
        assert rc == INVALID and (nl, ns) == (LB, SB), (first, count)
        assert raw_import(g, first, count, ref[0][0], ref[0][1]) == INVALID, (first, count)
    assert np.all(lbuf == 0x5A) and np.all(sbuf == 0x5A)
    # sizing: both strides, nothing else
    assert raw_export(g, 0, S, None, 0, None, 0) == (0, LB, SB)
    assert raw_export(g, 0, 0, None, 0, None, 0) == (0, LB, SB)
    assert raw_export(g, 0, S, None, 0, None, 0, strides=False)[0] == 0
    # a cap one byte short of either half: refused, nothing written to either buffer
    for lcap, scap in ((LB - 1, SB), (LB, SB - 1)):
        assert raw_export(g, 3, 1, lbuf, lcap, sbuf, scap)[0] == INVALID
        assert np.all(lbuf == 0x5A) and np.all(sbuf == 0x5A)
    # room to spare stays as it was
    assert raw_export(g, 3, 1, lbuf, lbuf.size, sbuf, sbuf.size)[0] == 0
    assert lbuf[:LB].tobytes() == ref[3][0] and np.all(lbuf[LB:] == 0x5A)
    assert sbuf[:SB].tobytes() == ref[3][1] and np.all(sbuf[SB:] == 0x5A)
    # import: count 0 is fine wherever a range may start, a missing half is not
    assert raw_import(g, 0, 0, b"", b"") == 0 and raw_import(g, S, 0, b"", b"") == 0
    assert g.L.gmx_lstm_group_import(g.h, 0, 1, None, LB, None, SB) == INVALID
    assert g.export_all() == ref               # (none of the refused calls moved anything)


def test_slices(gpu, five):
    g, ref = five
    h = gpu.LstmGroup(5)
    with stage_bytes(1):                        # every stream a slice of its own
        assert g.export_all() == ref
        h.import_all(ref)
    assert h.export_all() == ref
    # between one and two sections of a half: still one stream a slice, through buffers of another size; between two
    # and three: slices of two, so an odd stream lies 5 560 200 bytes (8 mod 16) or 1 458 256 into the staging buffer,
    # and a sub-range from stream 1 puts the even streams there
    for cap_l, cap_s in ((LB * 3 // 2, SB * 3 // 2), (LB * 5 // 2, SB * 5 // 2)):
        with stage_bytes(cap_l):
            assert g.export_all(short=False) == [(r[0], None) for r in ref]
            assert g.export_all(1, 4, short=False) == [(r[0], None) for r in ref[1:]]
        with stage_bytes(cap_s):
            assert g.export_all(long=False) == [(None, r[1]) for r in ref]
            assert g.export_all(1, 4, long=False) == [(None, r[1]) for r in ref[1:]]
            assert g.export_all() == ref        # (the long half one stream a slice, the short half two)
    for cap in (LB * 5 // 2, SB * 5 // 2):
        h.reset()
        with stage_bytes(cap):
            h.import_all(ref[1:], first=1)
            assert h.export_all(1, 4) == ref[1:]
        assert h.export_all(1, 4) == ref[1:]
        assert h.export(0)[1] != ref[0][1]
    h.close()


def test_import_replaces_isolates_and_continues(gpu, oracle):
    N = 230
    a = seeded_group(gpu, oracle, 2, 300)
    sa = [oracle.lstm_synth(2 * N, seed=51 + s, mask=(255, 31)[s]) for s in range(2)]
    learn(gpu, a, sa, [230, 130])
    g = seeded_group(gpu, oracle, 4, 400)
    sg = [oracle.lstm_synth(150, seed=61 + s, mask=127) for s in range(4)]
    learn(gpu, g, sg, [60, 110, 20, 150])
    before = g.export_all()
    secs = a.export_all()
    assert secs == [a.export(0), a.export(1)]
    g.import_all(secs, first=1)
    after = g.export_all()
    assert after[0] == before[0] and after[3] == before[3]
    assert after[1:3] == secs
    t = gpu.LstmGroup(4)                        # the twin: the same history through the per-stream calls
    for s in range(4):
        t.import_(*before[s], stream=s)
    t.import_(*secs[0], stream=1)
    t.import_(*secs[1], stream=2)
    assert [t.export(s) for s in range(4)] == after
    # 230 more bytes: across a backward pass, which reads lin_t, the padding and the scalars the host computed
    more = [(p[N:], d[N:]) for p, d in sa]
    ra = learn(gpu, a, more, [N, N])
    idle = (more[0][0][:1], more[0][1][:1])
    rg = learn(gpu, g, [idle, more[0], more[1], idle], [0, N, N, 0])
    rt = learn(gpu, t, [idle, more[0], more[1], idle], [0, N, N, 0])
    for s in range(2):
        for r in (rg, rt):
            assert np.array_equal(u32(r[0][1 + s]), u32(ra[0][s])), s
            assert np.array_equal(r[1][1 + s], ra[1][s]) and np.array_equal(r[2][1 + s], ra[2][s]), s
    end_a, end_g = a.export_all(), g.export_all()
    assert end_g[1:3] == end_a and end_g[0] == before[0] and end_g[3] == before[3]
    assert [t.export(s) for s in range(4)] == end_g
    assert end_a[0] != secs[0]
    for x in (a, g, t):
        x.close()


def test_import_accepts_a_mid_byte_file(gpu, oracle):
    N = 134
    ppm, data = oracle.lstm_synth(N, seed=71, mask=63)
    a = seeded_group(gpu, oracle, 1, 500)
    learn(gpu, a, [(ppm, data)], [130])
    a.forward(ppm[130], int(data[129]), stream=0)
    mid = a.export(0)                           # between that forward and its perceive
    g, t = gpu.LstmGroup(3), gpu.LstmGroup(3)
    g.import_all([mid, mid], first=1)
    for s in (1, 2):
        t.import_(*mid, stream=s)
    assert g.export_all() == [t.export(s) for s in range(3)]
    assert g.export_all(1, 2) == [mid, mid]
    for x in (g, t):
        x.perceive(int(data[130]), stream=1)    # stream 1: the perceive that was still to come ...
    rg = [g.forward(ppm[131], int(data[130]), stream=1), g.forward(ppm[131], int(data[130]), stream=2)]
    rt = [t.forward(ppm[131], int(data[130]), stream=1), t.forward(ppm[131], int(data[130]), stream=2)]
    for (pg, cg), (pt, ct) in zip(rg, rt):      # ... stream 2: a forward at once (the byte was never learned)
        assert np.array_equal(u32(pg), u32(pt)) and cg == ct
    for x in (g, t):
        for s in (1, 2):
            x.perceive(int(data[131]), stream=s)
    assert g.export_all() == [t.export(s) for s in range(3)]
    for x in (a, g, t):
        x.close()


@pytest.fixture(scope="module")
def learned3(gpu, oracle):
    g = seeded_group(gpu, oracle, 3, 600)
    learn(gpu, g, [oracle.lstm_synth(40, seed=81 + s, mask=255) for s in range(3)], [40, 7, 0])
    yield g
    g.close()


def put(b, at, v, width=4):
    b = bytearray(b)
    b[at:at + width] = int(v).to_bytes(width, "little")
    return bytes(b)


MALFORMED = {
    "long_4_bytes_short": lambda l, s: (l[:-4], s),
    "short_trailing_byte": lambda l, s: (l, s + b"\0"),
    "top_300": lambda l, s: (l, put(s, 0, 300)),
    "bot_above_mid": lambda l, s: (l, put(put(put(s, 0, 255), 4, 200), 8, 201)),
    "epoch_100": lambda l, s: (l, put(s, 227040, 100)),
    "update_steps_3001": lambda l, s: (l, put(s, 287648, 3001, 8)),
}


@pytest.mark.parametrize("case", list(MALFORMED))
def test_malformed_input_changes_nothing(gpu, five, learned3, case):
    _, ref = five
    g = learned3
    before = g.export_all()
    good = [ref[0], ref[4], ref[2]]
    bad_l, bad_s = MALFORMED[case](*good[2])
    rc = raw_import(g, 0, 3, good[0][0] + good[1][0] + bad_l, good[0][1] + good[1][1] + bad_s)
    assert rc == FORMAT
    with pytest.raises(gpu.GmxError) as e:
        g.import_all([good[0], good[1], (bad_l, bad_s)])
    assert e.value.status == FORMAT
    assert g.export_all() == before
    assert [g.export(s) for s in range(3)] == before
    g.import_all(good[:2])                      # the intact sections still go in
    assert g.export_all() == good[:2] + [before[2]]
    g.import_all(before)
    assert g.export_all() == before


@pytest.mark.parametrize("sessions", [1, 0])
def test_export_all_with_open_sessions(gpu, oracle, sessions):
    N = 14
    ppm, data = oracle.lstm_synth(N, seed=21, mask=31)
    w = oracle.LstmModel().weights()
    g, t = gpu.LstmGroup(2), gpu.LstmGroup(2)
    for x in (g, t):
        x.L.gmx_debug_lstm_use_sessions.argtypes = [C.c_void_p, C.c_int]
        assert x.L.gmx_debug_lstm_use_sessions(x.h, sessions) == 0
        x.set_weights(w, stream=1)
    last = 0
    for n in range(N):
        pg, cg = g.forward(ppm[n], last, stream=1)
        pt, ct = t.forward(ppm[n], last, stream=1)
        assert np.array_equal(u32(pg), u32(pt)) and cg == ct, n
        if n == 5:                              # between a forward and its perceive, the session open
            got = g.export_all()
            assert got == [g.export(0), g.export(1)]
            assert [int.from_bytes(got[1][1][4 * i:4 * i + 4], "little") for i in range(3)] == [255, 127, 0]
        for x in (g, t):
            x.perceive(int(data[n]), stream=1)
        if n == 9:                              # after a perceive that the session has only noted
            got = g.export_all()
            assert got == [g.export(0), g.export(1)]
            b = int(data[n])
            assert [int.from_bytes(got[1][1][4 * i:4 * i + 4], "little") for i in range(3)] == [b | 1, b & ~1, b & ~1]
        last = int(data[n])
    assert g.export_all() == [t.export(0), t.export(1)]
    g.close()
    t.close()
