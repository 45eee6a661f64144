"""The group checkpoint on the device (gmx_group_export / gmx_group_import, gmx_ckpt.hip): streams
[first, first + count) of a group in one call, the learned rows found, packed and scattered back by kernels.  Every
comparison is on bytes or uint32 patterns, tolerance 0: the sections are the per-stream export's bytes (and so the
reference's), and a group restored from them continues with the floats of the one they were taken from.

The staging cap of the library is replaced through the environment variable GMX_CKPT_STAGE_BYTES, which
gmx_group_export / gmx_group_import read at every call (test_slices)."""
import ctypes as C
import struct

import numpy as np
import pytest

import goldenlib
import kernel_shapes as ks
from gmix_amd import topology
from golden.cases import CASES

pytestmark = pytest.mark.gpu

INVALID, FORMAT = -1, -6


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


LAYOUTS = {
    # the reference's topology: the counter folded into the row's last 8 bytes
    "stock90": (lambda: topology.stock(90), dict(ctx_mode=4, zero_mod=11, bit_mode=1)),
    # the 256-input 24/8/1 bank: the counter right behind the weights
    "synth3_256": (lambda: topology.synth3(256), dict(ctx_mode=0)),
    "single256": (lambda: topology.single(256, 1 << 16), dict(ctx_mode=0)),
    # general shapes: a counter table of their own
    "bank24_n42_odd": (lambda: ks.topo_24_8_1(42, 0, max_large=2), ks.pattern(1)),
    "bank24_n100_pow2": (lambda: ks.topo_24_8_1(100, 1, pow2=True, max_large=2), ks.pattern(0)),
    "bank24_n300_odd": (lambda: ks.topo_24_8_1(300, 2, max_large=2), ks.pattern(3)),
    "random5": (lambda: ks.random_case(5)[0], ks.pattern(2)),
    "single_n255_t1": (lambda: ks.single_like(255, 1, 1), ks.pattern(0)),
}
GENERAL = "bank24_n42_odd"
# (the 256-input shape of the continuation tests: the same layout as synth3_256 at tables a test can afford twice)
WIDE = (lambda: ks.wide_like(0), ks.pattern(4))


def learned_group(gpu, topo, kw, lengths, seed=17):
    """A group whose stream s has learned lengths[s] bits of the synthetic stream (one ragged launch)."""
    g = gpu.MixerGroup(topo, len(lengths))
    b = gpu.Batch(g, max(max(lengths), 1), outputs=False, mask=True)
    b.fill_synthetic(seed=seed, **kw)
    g.run_ragged(b, lengths)
    g.sync()
    b.close()
    return g


def per_stream(g, first=0, count=None):
    count = g.S - first if count is None else count
    return [g.export(first + i) for i in range(count)]


def raw_export(g, first, count, cap=None, with_buffers=True):
    """gmx_group_export as the C caller sees it: (status, long_off list)."""
    off = (C.c_size_t * (max(count, 0) + 1))(*([123456789] * (max(count, 0) + 1)))
    if not with_buffers:
        return g.L.gmx_group_export(g.h, first, count, None, 0, off, None), list(off)
    lb = np.full(max(cap or 1, 1), 0xAB, np.uint8)
    sb = np.zeros(max(count, 1) * 24 * g.topo.n_mixers, np.uint8)
    rc = g.L.gmx_group_export(g.h, first, count, lb.ctypes.data_as(C.c_void_p), cap or 0, off,
                              sb.ctypes.data_as(C.c_void_p))
    return rc, list(off), lb


# ---- 1: the per-stream export's bytes, every layout ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_same_bytes_as_per_stream_export(gpu, name):
    make, kw = LAYOUTS[name]
    g = learned_group(gpu, make(), kw, [300, 0, 157, 1, 640])
    ref = per_stream(g)
    got = g.export_all()
    assert len(got) == 5
    for i in range(5):
        assert got[i][1] == ref[i][1], (name, i, "short")
        assert len(got[i][0]) == len(ref[i][0]) and got[i][0] == ref[i][0], (name, i, "long")
    assert len(ref[1][0]) == 8 * g.topo.n_mixers and len(ref[4][0]) > len(ref[1][0])
    g.close()


# ---- 2: the reference's bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stock90_learnable", "stock90_smallctx", "single256", "synth3_n256",
                                  "bank24_n100_skip99", "tiny_two_skips"])
def test_same_bytes_as_reference(gpu, oracle, name):
    meta, _z = goldenlib.load(name)
    topo = goldenlib.topo_of(meta)
    kw, nolearn = goldenlib.synth_kwargs(meta)
    assert nolearn is None
    T = meta["T"]
    g = gpu.MixerGroup(topo, 4)
    b = gpu.Batch(g, T, outputs=False, mask=True)
    for s in range(4):
        k = dict(kw) if s == 2 else dict(kw, seed=kw.get("seed", 0) + 1000 + s)   # the others run something else
        b.set_records(s, *oracle.Stream(topo.n_inputs, topo.n_mixers, **k).next(T))
    b.upload(T)
    g.run_ragged(b, [T // 2, 0, T, T - 1])
    secs = g.export_all()
    lb, sb = secs[2]
    assert sb.hex() == meta["short_hex"]
    assert len(lb) == meta["long_len"] and goldenlib.sha256(lb) == meta["long_sha256"]
    assert secs[0][0] != lb and secs[3][0] != lb
    b.close()
    g.close()


# ---- 3: streams that never learned ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stock90", "single256", GENERAL])
def test_never_learned_streams(gpu, name):
    g = gpu.MixerGroup(LAYOUTS[name][0](), 3)
    m = g.topo.n_mixers
    secs = g.export_all()
    for i, (lb, sb) in enumerate(secs):
        assert lb == bytes(8 * m)
        assert sb == struct.pack("<3Q", 0, 1, 0) * m   # steps_, max_steps_, contexts_seen_ as constructed
        assert (lb, sb) == g.export(i)
    g.close()


# ---- 4: sub-ranges and arguments ------------------------------------------------------------------------------------
def test_sub_ranges_and_arguments(gpu):
    make, kw = LAYOUTS[GENERAL]
    g = learned_group(gpu, make(), kw, [100, 200, 0, 300, 50])
    ref = per_stream(g)
    assert g.export_all(first=1, count=2) == ref[1:3]
    assert g.export_all(first=4) == ref[4:]
    assert g.export_all(first=0, count=0) == [] and g.export_all(first=5, count=0) == []
    rc, off = raw_export(g, 2, 0, with_buffers=False)
    assert rc == 0 and off[0] == 0
    for first, count in ((-1, 1), (0, -1), (0, 6), (5, 1), (6, 0), (3, 3)):
        assert raw_export(g, first, count, with_buffers=False)[0] == INVALID, (first, count)
    rc, off = raw_export(g, 1, 3, with_buffers=False)     # sizing
    sizes = [len(l) for l, _ in ref[1:4]]
    assert rc == 0 and off == [0, sizes[0], sizes[0] + sizes[1], sum(sizes)]
    rc, off, lb = raw_export(g, 1, 3, cap=sum(sizes) - 1)  # too small: long_off filled, nothing written
    assert rc == INVALID and off == [0, sizes[0], sizes[0] + sizes[1], sum(sizes)]
    assert (lb == 0xAB).all()
    rc, off, lb = raw_export(g, 1, 3, cap=sum(sizes))
    assert rc == 0 and lb.tobytes() == b"".join(l for l, _ in ref[1:4])
    # a long buffer without a short one (or the other way round) is no sizing call
    one = np.zeros(sum(sizes), np.uint8)
    off = (C.c_size_t * 4)()
    assert g.L.gmx_group_export(g.h, 1, 3, one.ctypes.data_as(C.c_void_p), one.size, off, None) == INVALID
    # import: the same range checks
    for first, count in ((-1, 1), (0, 6), (5, 1)):
        with pytest.raises(gpu.GmxError) as e:
            g.import_all(ref[:1] * count if count > 0 else [], first=first)
        assert e.value.status == INVALID
    g.import_all([], first=2)
    assert per_stream(g) == ref
    g.close()


# ---- 5: import continues bit-exactly --------------------------------------------------------------------------------
CONTINUE = {
    "stock90": LAYOUTS["stock90"], "wide256": WIDE, "single256": LAYOUTS["single256"], "general": LAYOUTS[GENERAL],
    "stock90_not_fresh": LAYOUTS["stock90"], "general_not_fresh": LAYOUTS[GENERAL],
}


@pytest.mark.parametrize("name", list(CONTINUE))
def test_import_continues_bit_exactly(gpu, name):
    make, kw = CONTINUE[name]
    topo = make()
    S, T1, T2 = 3, 500, 400
    A, B = gpu.MixerGroup(topo, S), gpu.MixerGroup(topo, S)
    bA = gpu.Batch(A, T1, outputs=True, mask=True)
    bB = gpu.Batch(B, T1, outputs=True, mask=True)
    bA.fill_synthetic(T1, seed=11, **kw)
    A.run_ragged(bA, [T1, T1 - 123, 0])
    if name.endswith("not_fresh"):          # B has learned something else: the import has to zero it
        bB.fill_synthetic(T1, seed=99, ctx_mode=0)
        B.run(bB, T1)
    secs = A.export_all()
    B.import_all(secs)
    assert B.export_all() == secs and per_stream(B) == secs
    bB.fill_synthetic(T1, seed=11, **kw)    # B's generator to where A's stands
    for g, b in ((A, bA), (B, bB)):
        b.fill_synthetic(T2, seed=11, restart=False, **kw)
        g.run(b, T2)
        b.download(T2)
        b.wait()
    assert np.array_equal(u32(bA.p[:, :T2]), u32(bB.p[:, :T2]))
    assert np.array_equal(u32(bA.outputs[:, :T2]), u32(bB.outputs[:, :T2]))
    assert per_stream(A) == per_stream(B)
    assert A.export_all() == B.export_all()
    for x in (bA, bB, A, B):
        x.close()


# ---- 6: across the two paths ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stock90", GENERAL])
def test_import_across_the_two_paths(gpu, name):
    make, kw = LAYOUTS[name]
    A = learned_group(gpu, make(), kw, [400, 90, 0, 250])
    one, many = per_stream(A), A.export_all()
    B = learned_group(gpu, make(), ks.pattern(0), [50, 50, 50, 50], seed=3)
    B.import_all(one)                       # sections of export(i) through import_all
    assert per_stream(B) == one and B.export_all() == one
    Cg = learned_group(gpu, make(), ks.pattern(0), [50, 50, 50, 50], seed=4)
    for i, (lb, sb) in enumerate(many):     # sections of export_all through import_(..., stream=i)
        Cg.import_(lb, sb, stream=i)
    assert per_stream(Cg) == one and Cg.export_all() == one
    # a sub-range leaves the other streams alone
    D = learned_group(gpu, make(), ks.pattern(0), [50, 60, 70, 80], seed=5)
    before = per_stream(D)
    D.import_all(many[1:3], first=2)
    assert per_stream(D) == before[:2] + many[1:3]
    for g in (A, B, Cg, D):
        g.close()


# ---- 7: malformed input changes nothing -----------------------------------------------------------------------------
def records_of(topo, lb):
    """[(mixer, offset of its header, cnt, record bytes)] of a long section."""
    out, p = [], 0
    for j, ws in enumerate(topo.weight_sizes()):
        cnt = struct.unpack_from("<I", lb, p)[0]
        out.append((j, p, cnt, 12 + 4 * ws))
        p += 8 + cnt * (12 + 4 * ws)
    assert p == len(lb)
    return out


@pytest.mark.parametrize("what", ["row_out_of_range", "steps_zero", "repeated_row", "descending_rows", "truncated",
                                  "trailing_bytes", "cnt_above_table", "input_size", "steps_disagree"])
def test_malformed_input_changes_nothing(gpu, what):
    make, kw = LAYOUTS[GENERAL]
    topo = make()
    A = learned_group(gpu, topo, kw, [300, 200, 400])
    secs = A.export_all()
    B = learned_group(gpu, topo, ks.pattern(0), [80, 0, 120], seed=9)
    before = B.export_all()
    lb, sb = bytearray(secs[2][0]), bytearray(secs[2][1])
    j, hdr, cnt, rec = next(r for r in records_of(topo, lb) if r[2] >= 2)
    r0, r1 = hdr + 8, hdr + 8 + rec
    if what == "row_out_of_range":
        struct.pack_into("<I", lb, r0, topo.mixers[j][1])
    elif what == "steps_zero":
        struct.pack_into("<Q", lb, r1 + 4, 0)
    elif what == "repeated_row":
        lb[r1:r1 + 4] = lb[r0:r0 + 4]
    elif what == "descending_rows":
        lb[r0:r0 + 4], lb[r1:r1 + 4] = lb[r1:r1 + 4], lb[r0:r0 + 4]
    elif what == "truncated":
        del lb[-4:]
    elif what == "trailing_bytes":
        lb += bytes(4)
    elif what == "cnt_above_table":
        struct.pack_into("<I", lb, hdr, topo.mixers[j][1] + 1)
    elif what == "input_size":
        struct.pack_into("<I", lb, hdr + 4, topo.weight_sizes()[j] + 1)
    elif what == "steps_disagree":
        struct.pack_into("<Q", sb, 24 * (topo.n_mixers - 1), 7)
    bad = secs[:2] + [(bytes(lb), bytes(sb))]
    with pytest.raises(gpu.GmxError) as e:
        B.import_all(bad)
    assert e.value.status == FORMAT
    assert B.export_all() == before and per_stream(B) == before
    B.import_all(secs)                      # and the intact sections still go in
    assert B.export_all() == secs
    A.close()
    B.close()


# ---- 8: sessions and lock step --------------------------------------------------------------------------------------
@pytest.mark.parametrize("persistent", [False, True])
def test_sessions_and_lockstep(gpu, oracle, persistent):
    topo = topology.stock(90)
    n, m = topo.n_inputs, topo.n_mixers
    S, T = 3, 60
    recs = [oracle.synth(n, m, T, seed=71 + s, ctx_mode=3, ctx_mod=5, zero_mod=6, bit_mode=1) for s in range(S)]
    G, W = gpu.MixerGroup(topo, S), gpu.MixerGroup(topo, S)      # W: the twin nobody checkpoints
    lsG = gpu.Lockstep(G, outputs=True, persistent=persistent)
    lsW = gpu.Lockstep(W, outputs=True, persistent=persistent)
    assert lsG.persistent == persistent

    def same_bytes_as_per_stream():
        got = G.export_all()
        assert got == per_stream(G)
        return got

    # a live per-bit session on stream 1: a checkpoint between a forward and its learn
    pred, act, ctx, bits = recs[1]
    for t in range(20):
        idx = np.nonzero(act[t])[0].astype(np.int32)
        pG, oG = G.forward(pred[t], idx, ctx[t], stream=1)
        pW, oW = W.forward(pred[t], idx, ctx[t], stream=1)
        assert np.array_equal(u32(oG), u32(oW)) and u32(pG) == u32(pW), t
        if t in (7, 13):
            same_bytes_as_per_stream()
        G.learn(bits[t], stream=1)
        W.learn(bits[t], stream=1)
        if t == 10:
            same_bytes_as_per_stream()
    # lock step over all streams: between a Predict and its Learn, and after a Learn
    for t in range(20, T):
        for ls in (lsG, lsW):
            for s in range(S):
                p_, a_, c_, _b = recs[s]
                ls.batch.set_records(s, p_[t:t + 1], a_[t:t + 1], c_[t:t + 1], np.zeros(1, np.uint8))
        pG, pW = lsG.predict().copy(), lsW.predict().copy()
        assert np.array_equal(u32(pG), u32(pW)), t
        assert np.array_equal(u32(lsG.batch.outputs[:, 0]), u32(lsW.batch.outputs[:, 0])), t
        if t in (30, 41):
            same_bytes_as_per_stream()
        for ls in (lsG, lsW):
            for s in range(S):
                ls.batch.bits[s, 0] = recs[s][3][t]
            ls.learn()
        if t == 35:
            same_bytes_as_per_stream()
    assert same_bytes_as_per_stream() == per_stream(W)
    for x in (lsG, lsW, G, W):
        x.close()


# ---- 9: slicing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stock90", GENERAL])
def test_slices(gpu, name, monkeypatch):
    make, kw = LAYOUTS[name]
    A = learned_group(gpu, make(), kw, [300, 0, 157, 1, 640])
    whole = A.export_all()
    sizes = [len(l) for l, _ in whole]
    # 1 byte: every stream a slice of its own (5 slices); the two largest sections' sum: slices of several streams
    for cap in (1, sorted(sizes)[-1] + sorted(sizes)[-2]):
        monkeypatch.setenv("GMX_CKPT_STAGE_BYTES", str(cap))
        assert A.export_all() == whole
        assert A.export_all(first=1, count=3) == whole[1:4]
        B = learned_group(gpu, make(), ks.pattern(0), [40] * 5, seed=2)
        B.import_all(whole)
        monkeypatch.delenv("GMX_CKPT_STAGE_BYTES")
        assert per_stream(B) == whole
        B.close()
    A.close()
