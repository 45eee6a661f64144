"""The Indirect group checkpoint on the device (gmx_indirect_group_export / gmx_indirect_group_import,
gmx_ind_ckpt.hip): streams [first, first + count) of a group in one call, the live entries found, packed and scattered
back by kernels.  Every comparison is on bytes or uint32 patterns, tolerance 0: the sections are the per-stream
export's bytes (and so the reference's), and a group restored from them continues with the floats of the one they
were taken from.

The section of one stream, per model: u32 cnt; cnt records {u32 key, u8 ns, u8 rm} in ascending key order if
cnt < size // 3 (size = 256 * table_size + 1), else the size ns bytes and the size rm bytes; 2048 bytes of logits.
craft() below writes such sections by hand; the per-stream gmx_indirect_import puts them into banks.

The staging cap of the library is replaced through the environment variable GMX_CKPT_STAGE_BYTES, which both calls
read at every call (test_slices)."""
import ctypes as C
import struct

import numpy as np
import pytest

import goldenlib
from gmix_amd.indirect import CKPT_CHUNK

pytestmark = pytest.mark.gpu

INVALID, FORMAT = -1, -6
MODELS5 = [(256, .02), (3, .1), (4096, .005), (1, .5), (65536, .02)]
SIZES5 = [256 * t + 1 for t, _ in MODELS5]
CTX_MOD = (40, 3, 900, 0)


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tabs():
    _, z = goldenlib.load("ind_tiny_dense")
    return z["ns_next"], z["rm_next"]


def learned_group(gpu, tabs, lengths, seed=17, models=MODELS5, ctx_mod=CTX_MOD):
    """A group whose stream s has learned lengths[s] bits of the device's synthetic stream (one ragged launch)."""
    g = gpu.IndirectGroup(models, tabs[0], tabs[1], len(lengths))
    b = gpu.IndirectBatch(g, max(max(lengths), 1))
    b.fill_synthetic(seed=seed, restart=True, ctx_mod=ctx_mod)
    g.run_ragged(b, lengths)
    g.sync()
    b.close()
    return g


def per_stream(g, first=0, count=None):
    count = g.S - first if count is None else count
    return [g.export(first + i) for i in range(count)]


def parse(sec, sizes=SIZES5):
    """[(offset of the model's header, cnt, dense)] of a section."""
    out, p = [], 0
    for size in sizes:
        cnt = struct.unpack_from("<I", sec, p)[0]
        dense = cnt >= size // 3
        out.append((p, cnt, dense))
        p += 4 + (2 * size if dense else 6 * cnt) + 2048
    assert p == len(sec)
    return out


def craft(states, rng, sizes=SIZES5):
    """A section with the given live entries: states[j] = sorted keys of model j; states and logits are random bytes
    (a live entry's ns is not 255)."""
    sec = bytearray()
    for size, keys in zip(sizes, states):
        keys = np.asarray(keys, np.uint32)
        assert (np.diff(keys.astype(np.int64)) > 0).all() and (len(keys) == 0 or keys[-1] < size)
        ns = rng.integers(0, 255, len(keys)).astype(np.uint8)
        rm = rng.integers(0, 256, len(keys)).astype(np.uint8)
        sec += struct.pack("<I", len(keys))
        if len(keys) < size // 3:
            rec = np.zeros(len(keys), np.dtype([("k", "<u4"), ("ns", "u1"), ("rm", "u1")]))
            rec["k"], rec["ns"], rec["rm"] = keys, ns, rm
            sec += rec.tobytes()
        else:
            lo, hi = np.full(size, 255, np.uint8), np.zeros(size, np.uint8)
            lo[keys], hi[keys] = ns, rm
            sec += lo.tobytes() + hi.tobytes()
        sec += rng.integers(0, 256, 2048).astype(np.uint8).tobytes()
    return bytes(sec)


def some_keys(rng, size, n):
    return np.sort(rng.choice(size, n, replace=False))


def round_trip(gpu, tabs, secs):
    """Sections through the per-stream import, the group export, the group import and the per-stream export."""
    A = gpu.IndirectGroup(MODELS5, tabs[0], tabs[1], len(secs))
    for i, sec in enumerate(secs):
        A.import_(sec, stream=i)
    ref = per_stream(A)
    assert ref == secs                      # (the crafted sections are what an export writes)
    got = A.export_all()
    for i in range(len(secs)):
        assert len(got[i]) == len(ref[i]) and got[i] == ref[i], i
    B = gpu.IndirectGroup(MODELS5, tabs[0], tabs[1], len(secs))
    B.import_all(got)
    back = per_stream(B)
    for i in range(len(secs)):
        assert back[i] == secs[i], i
    assert B.export_all() == secs
    A.close()
    B.close()


def raw_export(g, first, count, cap=None, with_buffer=True):
    """gmx_indirect_group_export as the C caller sees it: (status, off list[, buffer])."""
    off = (C.c_size_t * (max(count, 0) + 1))(*([123456789] * (max(count, 0) + 1)))
    if not with_buffer:
        return g.L.gmx_indirect_group_export(g.h, first, count, None, 0, off), list(off)
    buf = np.full(max(cap or 1, 1), 0xAB, np.uint8)
    rc = g.L.gmx_indirect_group_export(g.h, first, count, buf.ctypes.data_as(C.c_void_p), cap or 0, off)
    return rc, list(off), buf


# ---- 1: the per-stream export's bytes -------------------------------------------------------------------------------
def test_same_bytes_as_per_stream_export(gpu, tabs):
    lengths = [300, 0, 157, 1, 2500]
    g = gpu.IndirectGroup(MODELS5, tabs[0], tabs[1], 5)
    b = gpu.IndirectBatch(g, 2500)
    b.fill_synthetic(seed=17, restart=True, ctx_mod=CTX_MOD)
    g.run_ragged(b, lengths)
    for _ in range(8):                      # the last stream grows until both branches of the format occur
        ref = per_stream(g)
        kinds = {dense for sec in ref for _, cnt, dense in parse(sec) if cnt}
        if kinds == {False, True}:
            break
        b.fill_synthetic(seed=17, restart=False, ctx_mod=CTX_MOD)
        g.run_ragged(b, [0, 0, 0, 0, 2500])
    assert kinds == {False, True}, "a sparse and a dense model among the sections"
    got = g.export_all()
    assert len(got) == 5
    for i in range(5):
        assert len(got[i]) == len(ref[i]) and got[i] == ref[i], i
    assert len(ref[1]) == 5 * 2052 and len(ref[4]) > len(ref[0]) > len(ref[1])
    b.close()
    g.close()


# ---- 2: the reference's bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ind_tiny_dense", "ind_nolearn_tail", "ind_stock41"])
def test_same_bytes_as_reference(gpu, oracle, name):
    meta, models, ctx, bc, bits, nolearn, z = goldenlib.ind_case(name)
    T, K = meta["T"], len(models)
    kw = meta["synth"]
    g = gpu.IndirectGroup(models, z["ns_next"], z["rm_next"], 3)
    chunk = 4096
    b = gpu.IndirectBatch(g, chunk)
    other = [oracle.ind_synth(K, T, seed=kw.get("seed", 0) + 1000 + s, ctx_mod=kw.get("ctx_mod", (0,) * 4))
             for s in range(2)]               # the others run something else
    streams = [other[0], (ctx, bc, bits), other[1]]
    stop = T if nolearn is None else nolearn
    t0 = 0
    while t0 < T:
        n = min(chunk, T - t0) if t0 >= stop else min(chunk, stop - t0)
        for s, (c_, b_, x_) in enumerate(streams):
            b.set_records(s, c_[t0:t0 + n], b_[t0:t0 + n], x_[t0:t0 + n])
        b.upload(n)
        g.run(b, n, learn=t0 < stop)
        b.wait()
        t0 += n
    secs = g.export_all()
    assert len(secs[1]) == meta["long_len"] and goldenlib.sha256(secs[1]) == meta["long_sha256"]
    assert secs[0] != secs[1] and secs[2] != secs[1]
    b.close()
    g.close()


# ---- 3: streams that never learned ----------------------------------------------------------------------------------
def test_never_learned_streams(gpu, tabs):
    g = gpu.IndirectGroup(MODELS5, tabs[0], tabs[1], 3)
    secs = g.export_all()
    assert len(secs) == 3
    for i, sec in enumerate(secs):
        assert sec == (bytes(4) + bytes(2048)) * 5      # u32 0, the logits as constructed
        assert sec == g.export(i)
    g.close()


# ---- 4: the branch threshold and misalignment -----------------------------------------------------------------------
def test_branch_threshold_and_misalignment(gpu, tabs):
    rng = np.random.default_rng(4)

    def background():
        return [some_keys(rng, size, int(rng.integers(0, 40))) for size in SIZES5]

    secs = []
    for j in (3, 1):                        # size 257 and size 769
        size = SIZES5[j]
        assert size in (257, 769)
        for cnt in (size // 3 - 1, size // 3, size // 3 + 1, size):
            st = background()
            st[j] = some_keys(rng, size, cnt)
            secs.append(craft(st, rng))
            assert parse(secs[-1])[j][1:] == (cnt, cnt >= size // 3)
    secs.append(craft([np.array([0])] * 5, rng))                          # cnt = 1, the first entry
    secs.append(craft([np.array([size - 1]) for size in SIZES5], rng))    # cnt = 1, the last entry
    st = background()
    st[0] = some_keys(rng, SIZES5[0], 7)    # odd cnt in model 0: everything behind it sits at 2 mod 4
    secs.append(craft(st, rng))
    assert parse(secs[-1])[1][0] % 4 == 2
    st = background()
    st[0] = some_keys(rng, SIZES5[0], 30001)  # model 0 dense: its run-map bytes start at an odd offset
    secs.append(craft(st, rng))
    assert parse(secs[-1])[0][2] and (4 + SIZES5[0]) % 2 == 1
    st = [some_keys(rng, size, size) if size < 70000 else some_keys(rng, size, 3) for size in SIZES5]
    secs.append(craft(st, rng))             # every small model full
    round_trip(gpu, tabs, secs)


# ---- 5: chunk edges -------------------------------------------------------------------------------------------------
def test_chunk_edges(gpu, tabs):
    rng = np.random.default_rng(5)
    size, Cn = SIZES5[4], CKPT_CHUNK
    assert size % Cn == 1 and size > 2 * Cn     # the last chunk holds one entry: size - 1
    empty = [np.array([], np.uint32)] * 4
    secs = [craft(empty + [np.array(keys)], rng) for keys in (
        [0, Cn - 1, Cn, 2 * Cn - 1, size - 2, size - 1],
        [size - 1],                             # the only live entry in the last, partial chunk
        [size - 2],
        [Cn - 1, Cn],
        # every entry of a chunk, and of the iterations at its two ends
        list(range(3 * Cn, 4 * Cn)) + list(range(5 * Cn - 2048, 5 * Cn + 2048)),
    )]
    round_trip(gpu, tabs, secs)


# ---- 6: ranges, sizing and capacity ---------------------------------------------------------------------------------
def test_ranges_sizing_and_capacity(gpu, tabs):
    g = learned_group(gpu, tabs, [100, 200, 0, 300, 50])
    ref = per_stream(g)
    assert g.export_all() == ref
    assert g.export_all(first=1, count=2) == ref[1:3]
    assert g.export_all(first=4) == ref[4:]
    assert g.export_all(first=0, count=0) == [] and g.export_all(first=5, count=0) == []
    rc, off = raw_export(g, 2, 0, with_buffer=False)
    assert rc == 0 and off[0] == 0
    for first, count in ((-1, 1), (0, -1), (0, 6), (5, 1), (6, 0), (3, 3)):
        assert raw_export(g, first, count, with_buffer=False)[0] == INVALID, (first, count)
    assert g.L.gmx_indirect_group_export(g.h, 0, 1, None, 0, None) == INVALID
    sizes = [len(s) for s in ref[1:4]]
    want = [0, sizes[0], sizes[0] + sizes[1], sum(sizes)]
    rc, off = raw_export(g, 1, 3, with_buffer=False)       # sizing
    assert rc == 0 and off == want
    rc, off, buf = raw_export(g, 1, 3, cap=sum(sizes) - 1)  # too small: off filled, nothing written
    assert rc == INVALID and off == want
    assert (buf == 0xAB).all()
    rc, off, buf = raw_export(g, 1, 3, cap=sum(sizes))
    assert rc == 0 and off == want and buf.tobytes() == b"".join(ref[1:4])
    rc, off, buf = raw_export(g, 1, 3, cap=sum(sizes) + 7)  # room to spare stays as it was
    assert rc == 0 and buf[:sum(sizes)].tobytes() == b"".join(ref[1:4]) and (buf[sum(sizes):] == 0xAB).all()
    # import: the same range checks
    for first, count in ((-1, 1), (0, 6), (5, 1)):
        with pytest.raises(gpu.GmxError) as e:
            g.import_all(ref[:1] * count, first=first)
        assert e.value.status == INVALID
    off1 = (C.c_size_t * 2)(0, len(ref[0]))
    one = np.frombuffer(ref[0], np.uint8)
    assert g.L.gmx_indirect_group_import(g.h, 0, 1, one.ctypes.data_as(C.c_void_p), None) == INVALID
    assert g.L.gmx_indirect_group_import(g.h, 0, 1, None, off1) == INVALID
    g.import_all([], first=2)
    assert per_stream(g) == ref
    g.close()


# ---- 7: slices ------------------------------------------------------------------------------------------------------
def test_slices(gpu, tabs, monkeypatch):
    A = learned_group(gpu, tabs, [300, 0, 157, 1, 2500])
    whole = A.export_all()
    assert whole == per_stream(A)
    sizes = sorted(len(s) for s in whole)
    # 1 byte: every stream a slice of its own (5 slices); between one and two sections: slices of one and of several
    for cap in (1, sizes[-1] + sizes[0] + 1):
        assert cap == 1 or sizes[-1] < cap < sizes[-1] + sizes[-2]
        monkeypatch.setenv("GMX_CKPT_STAGE_BYTES", str(cap))
        assert A.export_all() == whole
        assert A.export_all(first=1, count=3) == whole[1:4]
        B = learned_group(gpu, tabs, [40] * 5, seed=2)
        B.import_all(whole)
        monkeypatch.delenv("GMX_CKPT_STAGE_BYTES")
        assert per_stream(B) == whole
        B.close()
    A.close()


# ---- 8: import replaces and isolates --------------------------------------------------------------------------------
def test_import_replaces_and_isolates(gpu, oracle, tabs):
    K, T1, T2 = len(MODELS5), 900, 200
    A = learned_group(gpu, tabs, [T1, T1 - 333], seed=11)
    secs = A.export_all()
    G = learned_group(gpu, tabs, [500, 600, 700, 800], seed=99, ctx_mod=(7, 3, 50, 0))   # has learned something else
    before = per_stream(G)
    assert before[1] != secs[0]
    G.import_all(secs, first=1)
    after = per_stream(G)
    assert after[0] == before[0] and after[3] == before[3]
    assert after[1:3] == secs               # entries absent from a section are back to never-seen
    assert G.export_all() == [before[0]] + secs + [before[3]]
    twin = learned_group(gpu, tabs, [500, 600, 700, 800], seed=99, ctx_mod=(7, 3, 50, 0))
    for i in range(2):
        twin.import_(secs[i], stream=1 + i)
    for s in range(4):
        assert np.array_equal(u32(G.slot_values(s)), u32(twin.slot_values(s))), s
    # 200 more bits on the restored streams and on the ones the sections came from.  The blackboard slots are not part
    # of a checkpoint (a silent model repeats its slot): the caller carries them over, as between any two surfaces.
    for i in range(2):
        G.set_slot_values(A.slot_values(i), 1 + i)
    recs = [oracle.ind_synth(K, T2, seed=300 + i, ctx_mod=CTX_MOD) for i in range(2)]
    bA, bG = gpu.IndirectBatch(A, T2), gpu.IndirectBatch(G, T2)
    for i in range(2):
        bA.set_records(i, *recs[i])
        bG.set_records(1 + i, *recs[i])
    for g, b, n in ((A, bA, [T2, T2]), (G, bG, [0, T2, T2, 0])):
        b.upload(T2)
        g.run_ragged(b, n)
        b.download(T2)
        b.wait()
    assert np.array_equal(u32(bA.predictions[:, :T2]), u32(bG.predictions[1:3, :T2]))
    assert np.array_equal(bA.active[:, :T2], bG.active[1:3, :T2])
    assert bA.active[:, :T2].any()
    assert per_stream(A) == per_stream(G, 1, 2) and A.export_all() == G.export_all(1, 2)
    assert per_stream(G, 0, 1) == before[:1] and per_stream(G, 3, 1) == before[3:]
    for x in (bA, bG, A, G, twin):
        x.close()


# ---- 9: malformed input changes nothing -----------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["truncated", "trailing_byte", "cnt_above_size", "key_out_of_range", "equal_keys",
                                  "swapped_keys"])
def test_malformed_input_changes_nothing(gpu, tabs, what):
    A = learned_group(gpu, tabs, [300, 200, 400])
    secs = A.export_all()
    B = learned_group(gpu, tabs, [80, 0, 120], seed=9)
    before = per_stream(B)
    sec = bytearray(secs[2])
    j, (hdr, cnt, _d) = next((j, m) for j, m in enumerate(parse(sec)) if not m[2] and m[1] >= 2)   # a sparse model
    r0, r1 = hdr + 4, hdr + 10
    if what == "truncated":
        del sec[-5:]
    elif what == "trailing_byte":
        sec += bytes(1)
    elif what == "cnt_above_size":
        struct.pack_into("<I", sec, parse(sec)[3][0], SIZES5[3] + 1)
    elif what == "key_out_of_range":
        struct.pack_into("<I", sec, hdr + 4 + 6 * (cnt - 1), SIZES5[j])
    elif what == "equal_keys":
        sec[r1:r1 + 4] = sec[r0:r0 + 4]
    elif what == "swapped_keys":
        sec[r0:r0 + 4], sec[r1:r1 + 4] = sec[r1:r1 + 4], sec[r0:r0 + 4]
    with pytest.raises(gpu.GmxError) as e:
        B.import_all(secs[:2] + [bytes(sec)])
    assert e.value.status == FORMAT
    assert per_stream(B) == before and B.export_all() == before
    B.import_all(secs)                      # and the intact sections still go in
    assert per_stream(B) == secs
    A.close()
    B.close()


# ---- 10: a forward in flight survives an export ---------------------------------------------------------------------
@pytest.mark.parametrize("sessions", [1, 0])
def test_forward_in_flight_survives_an_export(gpu, oracle, tabs, sessions):
    K, T = len(MODELS5), 60
    G = gpu.IndirectGroup(MODELS5, tabs[0], tabs[1], 2)
    W = gpu.IndirectGroup(MODELS5, tabs[0], tabs[1], 2)      # the twin nobody checkpoints
    for g in (G, W):
        g.L.gmx_debug_indirect_use_sessions.argtypes = [C.c_void_p, C.c_int]
        assert g.L.gmx_debug_indirect_use_sessions(g.h, sessions) == 0
    ctx, bc, bits = oracle.ind_synth(K, T, seed=5, ctx_mod=CTX_MOD)
    for t in range(T):
        s = t % 2
        pG, aG = G.forward(ctx[t], bc[t], stream=s)
        pW, aW = W.forward(ctx[t], bc[t], stream=s)
        assert np.array_equal(u32(pG), u32(pW)) and np.array_equal(aG, aW), t
        if t == 10:
            assert (G.L.gmx_debug_open_sessions() > 0) == bool(sessions)   # the path under test is the one in use
        if t in (7, 20, 41):                # between a forward and its learn
            assert G.export_all() == per_stream(G)
        G.learn(bits[t], stream=s)
        W.learn(bits[t], stream=s)
        if t == 30:                         # after a learn that is only noted so far
            assert G.export_all() == per_stream(G)
    got = G.export_all()
    assert got == per_stream(W) and len(got[0]) > 5 * 2052
    G.close()
    W.close()
