"""gmx_ctx_group_export / _import / _blackboard_get / _blackboard_set (gmx_ctx_ckpt.hip): the checkpoint of a whole
context group in one call, against the per-stream calls (unchanged code), tests/helpers/ctx_ref.c and the fixtures the
reference recorded (tests/golden/ctx_*.npz).  Tolerance 0 everywhere: sections and boards are compared byte for byte,
values as uint32.  The counts that make a case meaningful are asserted from ctx_ref.c before the device is compared."""
import ctypes as C
import struct

import numpy as np
import pytest

import ctx_common as cc
import ctx_harness
import ctx_shapes as cs
from gmix_amd import GmxError
from gmix_amd._lib import CtxBlackboard
from gmix_amd.ctx import CKPT_CHUNK

pytestmark = pytest.mark.gpu
GMX_ERR_INVALID, GMX_ERR_STATE, GMX_ERR_FORMAT = -1, -5, -6
# round trips the calls document (gmx_ctx_ckpt.inc), with every stream in one slice
OPS_EXPORT, OPS_SIZING, OPS_IMPORT, OPS_BOARDS = 5 + 3, 4, 4 + 3, 4
MIXED, MIXED_SIZES = "v63_h15", [1000, 257, 65536, 255, 16384, 1000, 1, 256, 4096, 5, 4096, 32769, 257, 4096, 255]
MIXED_BITS = [0, 3, 605, 2600, 8013]
_state = {}


def boards_bytes(boards):
    return [cc.board_bytes(b) for b in boards]


def run_ragged_to(gpu, g, streams, counts, chunk=8192):
    """Stream s of g codes the first counts[s] bits of streams[s]."""
    done = [0] * g.S
    b = gpu.CtxBatch(g, min(chunk, max(max(counts), 1)), values=False)
    while any(d < c for d, c in zip(done, counts)):
        n = [min(b.max_bits, c - d) for d, c in zip(done, counts)]
        for s in range(g.S):
            b.bits[s, :n[s]] = streams[s][done[s]:done[s] + n[s]]
        b.upload(max(n))
        g.run_ragged(b, n)
        b.wait()
        g.sync()
        done = [d + k for d, k in zip(done, n)]
    b.close()


def split(sec, off, sizes):
    """[(table size, count, dense)] of one stream's sections."""
    parts = [sec[off[h]:off[h + 1]] for h in range(len(sizes))]
    return [(t, ctx_harness.section_count(p), ctx_harness.is_dense(p, t)) for t, p in zip(sizes, parts)]


def mixed(gpu):
    """Five streams of v63_h15 run ragged for 0, 3, 605, 2 600 and 8 013 bits: ctx_ref.c's sections and boards, and the
    bank, which the tests that only read it share."""
    if "mixed" in _state:
        return _state["mixed"]
    descs = cs.as_descs(cs.descs(MIXED))
    assert [d.table_size for d in descs if d.kind == 6] == MIXED_SIZES
    bits = np.unpackbits(cs.stream(MIXED))
    streams = [bits[8 * o:] for o in cs.offsets(5)]
    refs = []
    for s, n in enumerate(MIXED_BITS):
        r = cc.Ref(descs)
        r.run(streams[s][:n], values=False)
        refs.append(r)
    want = [r.export() for r in refs]
    g = gpu.CtxGroup(descs, 5)
    run_ragged_to(gpu, g, streams, MIXED_BITS)
    x = dict(descs=descs, g=g, want=want, boards=boards_bytes([r.board() for r in refs]),
             tabs=[split(sec, off, MIXED_SIZES) for sec, off in want])
    _state["mixed"] = x
    return x


def joined(want, first, count):
    secs = [want[s][0] for s in range(first, first + count)]
    off = [0]
    for sec in secs:
        off.append(off[-1] + len(sec))
    return b"".join(secs), off, [want[s][1] for s in range(first, first + count)]


# ---- 1. both branches, empty tables, a branch that flips between streams: one call ------------------------------------
def test_mixed_branches_in_one_call_equal_the_per_stream_call_and_ctx_ref(gpu):
    x = mixed(gpu)
    g, want, tabs = x["g"], x["want"], x["tabs"]
    # what ctx_ref.c says the case holds
    for s in (0, 1):
        assert all((n, d) == (0, t == 1) for t, n, d in tabs[s]), (s, tabs[s])
    k1000 = [i for i, t in enumerate(MIXED_SIZES) if t == 1000]
    assert [tabs[3][i][1:] for i in k1000] == [(276, False), (274, False)]
    assert [tabs[4][i][1:] for i in k1000] == [(623, True), (621, True)]
    i64k, i257 = MIXED_SIZES.index(65536), MIXED_SIZES.index(257)
    assert (tabs[3][i64k][1:], tabs[4][i64k][1:]) == ((322, False), (984, False))
    assert (tabs[3][i257][1:], tabs[4][i257][1:]) == ((128, True), (157, True))
    for s in (3, 4):
        assert any(d for _, _, d in tabs[s]) and any(not d and n for _, n, d in tabs[s]), s
    per = [g.export(s) for s in range(5)]
    assert per == want
    outside = {(0, 5): [], (1, 3): [0, 4], (4, 1): [0, 3]}
    for (first, count), others in outside.items():
        data, off, var = g.group_export(first, count)
        assert (data, off, var) == joined(want, first, count), (first, count)
        assert [g.export(s) for s in others] == [want[s] for s in others], (first, count)
    assert x["boards"] == boards_bytes(g.group_blackboards()) == boards_bytes([g.blackboard(s) for s in range(5)])


# ---- 2. sizing and capacity ---------------------------------------------------------------------------------------
def test_sizing_capacity_and_a_bank_without_hash_variables(gpu):
    x = mixed(gpu)
    g = x["g"]
    data, off, var = joined(x["want"], 0, 5)
    assert g.group_sizes() == (off, var)
    assert g.group_ops() == OPS_SIZING
    canary = np.full(off[-1] + 64, 0xA5, np.uint8)
    o = (C.c_size_t * 6)()
    rc = g.L.gmx_ctx_group_export(g.h, 0, 5, canary.ctypes.data_as(C.c_void_p), off[-1] - 1, o, None)
    assert rc == GMX_ERR_INVALID and (canary == 0xA5).all() and list(o) == off
    assert g.L.gmx_ctx_group_export(g.h, 0, 5, canary.ctypes.data_as(C.c_void_p), off[-1], o, None) == 0
    assert canary[:off[-1]].tobytes() == data and (canary[off[-1]:] == 0xA5).all()
    # H = 0: empty sections, nothing launched
    g0 = gpu.CtxGroup(cs.as_descs(cs.descs("v64_h0")), 3)
    assert g0.H == 0 and g0.export(1) == (b"", [0])
    assert g0.group_export() == (b"", [0, 0, 0, 0], [[0], [0], [0]]) and g0.group_ops() == 0
    g0.group_import(b"", [0, 0, 0, 0])
    assert g0.group_ops() == 0
    with pytest.raises(GmxError) as e:
        g0.group_import(b"\0\0\0\0", [0, 0, 0, 4])
    assert e.value.status == GMX_ERR_FORMAT
    g0.close()


# ---- 3. slices -----------------------------------------------------------------------------------------------------
def test_slices_give_the_same_bytes_both_ways(gpu):
    x = mixed(gpu)
    g = x["g"]
    data, off, var = joined(x["want"], 0, 5)
    lens = [off[i + 1] - off[i] for i in range(5)]
    three = off[3]   # streams 0-2 fit together; stream 3 fits with neither neighbour
    assert lens[3] > three and lens[3] + lens[4] > three and min(lens) > 16
    fresh = cc.Ref(x["descs"]).export()
    for stage, slices in ((16, 5), (three, 3), (None, 1)):
        assert g.group_export(stage_bytes=stage) == (data, off, var), stage
        assert g.group_ops() == 5 + 3 * slices, stage
        g2 = gpu.CtxGroup(x["descs"], 6)
        g2.group_import(b"\xEE" * 7 + data, [o + 7 for o in off], first=1, stage_bytes=stage)
        assert g2.group_ops() == 4 + 3 * slices, stage
        assert g2.group_export(1, 5) == (data, off, var), stage
        assert g2.export(0) == fresh, stage
        g2.close()


# ---- 4. tables of more than one chunk ----------------------------------------------------------------------------------
def test_big_tables_both_branches_import_and_continue(gpu):
    name = "big_tables"
    descs = cs.as_descs(cs.descs(name))
    sizes = [d.table_size for d in descs if d.kind == 6]
    assert sizes == cs.BIG_TABLE_SIZES
    bits = np.unpackbits(cs.stream(name))
    counts = [8 * cs.BIG_MID_BYTES, 8 * cs.BIG.n_bytes]
    tail = np.unpackbits(np.random.default_rng(77).integers(0, 256, 64, dtype=np.uint8))
    refs = [cc.Ref(descs), cc.Ref(descs)]
    for r, n in zip(refs, counts):
        r.run(bits[:n], values=False)
    want = [r.export() for r in refs]
    mid, end = split(*want[0], sizes), split(*want[1], sizes)
    # (tests/test_gpu_ctx_shapes.py asserts the same counts from ctx_ref.c)
    assert sorted(n for t, n, d in mid if not d and n > CKPT_CHUNK) == [18552, 19637, 20721], mid
    assert sorted(t for t, n, d in end if d and t > CKPT_CHUNK) == [16385, 32769, 40000, 49999], end
    assert [(t, n) for t, n, d in end if not d and n > CKPT_CHUNK] == [(65536, 29826)], end
    boards = [r.board() for r in refs]
    tail_want = [r.run(tail) for r in refs]
    g = gpu.CtxGroup(descs, 2)
    run_ragged_to(gpu, g, [bits, bits], counts)
    full = g.group_export()
    assert full == joined(want, 0, 2) and [g.export(s) for s in range(2)] == want
    g2 = gpu.CtxGroup(descs, 3)
    g2.group_import(full[0], full[1], first=1)
    assert g2.group_export(1, 2) == full
    assert g2.export(0) == cc.Ref(descs).export()
    # the boards across, then both banks go on for 64 bytes
    got = g.group_blackboards()
    assert boards_bytes(got) == boards_bytes(boards)
    g2.set_group_blackboards(got, first=1)
    n = len(tail)
    b1, b2 = gpu.CtxBatch(g, n), gpu.CtxBatch(g2, n)
    b1.bits[:, :n] = tail
    b2.bits[1:, :n] = tail
    b1.upload(n)
    b2.upload(n)
    g.run(b1, n)
    g2.run_ragged(b2, [0, n, n])
    for b in (b1, b2):
        b.download(n)
        b.wait()
    for s in range(2):
        assert np.array_equal(b1.values[s], tail_want[s]) and np.array_equal(b2.values[s + 1], tail_want[s]), s
    after = joined([r.export() for r in refs], 0, 2)
    assert g.group_export() == after and g2.group_export(1, 2) == after
    assert boards_bytes(g.group_blackboards()) == boards_bytes(g2.group_blackboards(1, 2)) \
        == boards_bytes([r.board() for r in refs])
    for h in (b1, b2, g, g2):
        h.close()


# ---- 5. chunk edges and the branch boundary, hand-made ------------------------------------------------------------------
HAND_SIZES = [40000, 1000, 5, 2, 1]
HAND_DESCS = [("h%d" % t, "indirect_hash", dict(outer_order=2, table_size=t, inner_order=2)) for t in HAND_SIZES] \
    + [("bit_context", "bit_context", {})]
EDGE_KEYS = [0, CKPT_CHUNK - 1, CKPT_CHUNK, CKPT_CHUNK + 1, 2 * CKPT_CHUNK - 1, 2 * CKPT_CHUNK, 39999]


def table_section(size, entries, outer_context, outer_hash):
    """IndirectHash::WriteToDisk of a table holding `entries` {key: non-zero value}."""
    keys = sorted(entries)
    assert all(0 <= k < size and entries[k] for k in keys)
    out = struct.pack("<I", len(keys))
    if len(keys) < size // 2:
        out += b"".join(struct.pack("<II", k, entries[k]) for k in keys)
    else:
        out += b"".join(struct.pack("<I", entries.get(k, 0)) for k in range(size))
    return out + struct.pack("<QI", outer_context, outer_hash)


def first_keys(n, seed):
    return {k: 0x01000000 * seed + k + 1 for k in range(n)}


def hand_streams():
    """Three streams of HAND_SIZES: [per-table sections].  Stream 0 stands below every branch boundary, stream 1 on it,
    stream 2 mixes a sparse multi-chunk table with a dense 1 000-entry one."""
    edge = {k: 0xC0000000 + i for i, k in enumerate(EDGE_KEYS)}
    s0 = [edge, first_keys(499, 1), {3: 7}, {}, {}]
    s1 = [{}, {2 * k: k + 1 for k in range(500)}, {0: 1, 4: 0xFFFFFFFF}, {1: 9}, {0: 0x80000000}]
    s2 = [edge, first_keys(500, 2), {}, {}, {}]
    return [[table_section(t, e, 0x0102030405060708 + 16 * s + i, 0xABCD0000 + 16 * s + i)
             for i, (t, e) in enumerate(zip(HAND_SIZES, tabs))] for s, tabs in enumerate((s0, s1, s2))]


def through_ctx_ref(descs, sec):
    r = cc.Ref(descs)
    r.import_(sec)
    return r.export()


def test_hand_made_chunk_edges_and_branch_boundaries(gpu):
    descs = cs.as_descs(HAND_DESCS)
    parts = hand_streams()
    secs = [b"".join(p) for p in parts]
    want = [through_ctx_ref(descs, sec) for sec in secs]   # cref_import -> cref_export: the same bytes
    assert [w[0] for w in want] == secs
    tabs = [split(*w, HAND_SIZES) for w in want]
    assert [(n, d) for _, n, d in tabs[0]] == [(7, False), (499, False), (1, False), (0, False), (0, True)]
    assert [(n, d) for _, n, d in tabs[1]] == [(0, False), (500, True), (2, True), (1, True), (1, True)]
    assert [(n, d) for _, n, d in tabs[2][:2]] == [(7, False), (500, True)]
    full = joined(want, 0, 3)
    g = gpu.CtxGroup(descs, 3)
    g.group_import(full[0], full[1])
    assert g.group_export() == full
    assert [g.export(s) for s in range(3)] == want
    # once more over the same bank, the branches the other way round: what a sparse import must clear is cleared
    swapped = joined(want[::-1], 0, 3)
    g.group_import(swapped[0], swapped[1])
    assert g.group_export() == swapped
    g.close()


# ---- 6. a bad section anywhere leaves every bank alone --------------------------------------------------------------------
def test_a_damaged_last_section_leaves_every_stream_alone(gpu):
    descs = cs.as_descs(HAND_DESCS)
    parts = hand_streams()
    secs = [b"".join(p) for p in parts]
    good = b"".join(secs)
    off = [0, len(secs[0]), len(secs[0]) + len(secs[1]), len(good)]
    t0 = off[2]                       # stream 2's 40 000-entry table: sparse, 7 pairs
    t1 = t0 + len(parts[2][0])        # its 1 000-entry table: dense, 500 entries

    def patched(at, fmt, *v):
        x = bytearray(good)
        struct.pack_into(fmt, x, at, *v)
        return bytes(x), off

    sparse_500 = struct.pack("<I", 500) + b"".join(struct.pack("<II", k, k + 1) for k in range(500)) + parts[2][1][-12:]
    assert len(sparse_500) == len(parts[2][1])   # (8 x 500 = 4 x 1 000: only the count of non-zero words tells)
    cases = {
        "truncated": (good[:-5], off[:3] + [off[3] - 5]),
        "one byte too long": (good + b"\0", off[:3] + [off[3] + 1]),
        "keys not ascending": patched(t0 + 4, "<IIII", EDGE_KEYS[1], 5, EDGE_KEYS[0], 6),
        "a key equal to table_size": patched(t0 + 4 + 8 * 6, "<I", 40000),
        "a zero value in a sparse record": patched(t0 + 4 + 8 * 3 + 4, "<I", 0),
        "dense body against its count": patched(t1 + 4 + 4 * 17, "<I", 0),
        "the sparse branch at a dense count": (good[:t1] + sparse_500 + good[t1 + len(sparse_500):], off),
    }
    assert struct.unpack_from("<I", good, t1 + 4 + 4 * 17)[0] != 0
    g = gpu.CtxGroup(descs, 3)
    rot = joined([(s, None) for s in secs[1:] + secs[:1]], 0, 3)   # something else in every stream first
    g.group_import(rot[0], rot[1])
    streams = [np.unpackbits(np.random.default_rng(5 + s).integers(0, 256, 8, dtype=np.uint8)) for s in range(3)]
    run_ragged_to(gpu, g, streams, [13, 0, 29])
    before = (g.group_export(), boards_bytes(g.group_blackboards()), [g.export(s) for s in range(3)])
    for what, (data, o) in cases.items():
        with pytest.raises(GmxError) as e:
            g.group_import(data, o)
        assert e.value.status == GMX_ERR_FORMAT, what
        assert (g.group_export(), boards_bytes(g.group_blackboards()), [g.export(s) for s in range(3)]) == before, what
    g.group_import(good, off)
    assert g.group_export()[:2] == (good, off) and boards_bytes(g.group_blackboards()) == before[1]
    g.close()


# ---- 7. blackboards -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.FIXTURES)
def test_blackboards_at_the_recorded_positions_and_resume_inside_a_byte(gpu, name):
    f = cc.fixture(name)
    idx = [0, 1, f.positions.index(8 * 1001 + 5)]
    pos = [f.positions[p] for p in idx]
    assert pos == [0, 3, 8013]
    g = gpu.CtxGroup(f.descs, 3)
    run_ragged_to(gpu, g, [f.bits] * 3, pos)
    boards = g.group_blackboards()
    assert g.group_ops() == OPS_BOARDS
    assert boards_bytes(boards) == boards_bytes([g.blackboard(s) for s in range(3)]) \
        == boards_bytes([f.boards[p] for p in idx])
    assert boards[0].first_prediction == 1 and boards[2].rotating_history_pos == 1 and boards[2].recent_bits > 1
    data, off, var = g.group_export()
    assert [data[off[i]:off[i + 1]] for i in range(3)] == [f.section(p) for p in idx]
    # a fresh bank takes sections and boards, streams in another place, and both banks go on
    g2 = gpu.CtxGroup(f.descs, 4)
    g2.group_import(data, off, first=1)
    assert boards_bytes(g2.group_blackboards()) == boards_bytes([f.boards[0]] * 4)   # import leaves the boards alone
    g2.set_group_blackboards(boards, first=1)
    assert g2.group_ops() == OPS_BOARDS
    n = 100
    b1, b2 = gpu.CtxBatch(g, n), gpu.CtxBatch(g2, n)
    for s in range(3):
        b1.bits[s, :n] = b2.bits[s + 1, :n] = f.bits[pos[s]:pos[s] + n]
    b1.upload(n)
    b2.upload(n)
    g.run(b1, n)
    g2.run_ragged(b2, [0, n, n, n])
    for b in (b1, b2):
        b.download(n)
        b.wait()
    for s in range(3):
        want = f.values()[pos[s]:pos[s] + n]
        assert np.array_equal(b1.values[s], want) and np.array_equal(b2.values[s + 1], want), s
    assert g2.group_export(1, 3) == g.group_export()
    assert boards_bytes(g2.group_blackboards(1, 3)) == boards_bytes(g.group_blackboards())
    if name == "ctx_tiny":   # (ctx_ref.c over the stock tables: 201 MB a stream to walk)
        for s in range(3):
            r = cc.Ref(f.descs)
            r.import_(f.section(idx[s]))
            r.set_board(f.boards[idx[s]])
            r.run(f.bits[pos[s]:pos[s] + n], values=False)
            assert g2.export(s + 1) == r.export() and cc.board_bytes(g2.blackboard(s + 1)) == cc.board_bytes(r.board())
    # one bad board in the window: nothing is written
    before = boards_bytes(g2.group_blackboards())

    def bad(**kw):
        bb = CtxBlackboard.from_buffer_copy(boards[2])
        for k, v in kw.items():
            setattr(bb, k, v)
        return [boards[0], boards[1], bb]

    for what, bs in (("last_byte", bad(last_byte=(boards[2].last_byte + 1) & 255)),
                     ("recent_bits 0", bad(recent_bits=0)),
                     ("first_prediction inside a byte", bad(first_prediction=1, recent_bits=5))):
        with pytest.raises(GmxError) as e:
            g2.set_group_blackboards(bs, first=0)
        assert e.value.status == GMX_ERR_INVALID, what
        assert boards_bytes(g2.group_blackboards()) == before, what
    for h in (b1, b2, g, g2):
        h.close()


# ---- 8. round trips do not depend on the stream count ------------------------------------------------------------------
def test_round_trips_are_the_documented_ones_for_one_stream_and_for_five(gpu):
    x = mixed(gpu)
    g = x["g"]
    g2 = gpu.CtxGroup(x["descs"], 5)
    for count in (1, 5):
        first = 5 - count   # (stream 4 is the longest: one stream or five, one slice)
        data, off, _ = g.group_export(first, count)
        assert g.group_ops() == OPS_EXPORT, count
        g.group_sizes(first, count)
        assert g.group_ops() == OPS_SIZING, count
        g2.group_import(data, off, first)
        assert g2.group_ops() == OPS_IMPORT, count
        boards = g.group_blackboards(first, count)
        assert g.group_ops() == OPS_BOARDS, count
        g2.set_group_blackboards(boards, first)
        assert g2.group_ops() == OPS_BOARDS, count
    assert g2.group_export() == g.group_export()
    g2.close()


# ---- 9. beside the lock step -------------------------------------------------------------------------------------------
def test_beside_the_lock_step(gpu, oracle):
    import test_gpu_chainstep_ctx as tc
    f = tc.tiny()
    S, T, offsets = 3, 200, [0, 61, 500]
    x = tc.chain(oracle, S, T + 8, offsets, False, tc.MIXER_ROUTE, seed=120)
    cg = gpu.CtxGroup(f.descs, S)
    mg = gpu.MixerGroup(tc.TOPO, S)
    step = gpu.ChainStep(mg)
    step.attach_ctx(cg, tc.MIXER_ROUTE)
    tc.drive(step, x, 0, T)     # (its last step is a Learn alone)
    refs = []
    for s in range(S):
        r = cc.Ref(f.descs)
        r.run(x["bits"][s][:T], values=False)
        refs.append(r)
    want = joined([r.export() for r in refs], 0, S)
    assert cg.group_export() == want
    assert boards_bytes(cg.group_blackboards()) == boards_bytes([r.board() for r in refs])

    def records(i):
        step.predictions[:, :x["other"].shape[2]] = x["other"][:, i]
        step.active_mask[:] = x["maskw"][:, i]
        step.contexts[:] = x["mctx_host"][:, i]

    # stream 0 between its Predict and its Learn
    records(T)
    step.what[:], step.bits[:] = [tc.PREDICT, 0, 0], 0
    step.step()
    canary = (CtxBlackboard * S)()
    C.memset(canary, 0x5A, C.sizeof(canary))
    assert cg.L.gmx_ctx_group_blackboard_get(cg.h, 0, S, canary) == GMX_ERR_STATE
    assert bytes(canary) == b"\x5A" * C.sizeof(canary)
    assert boards_bytes(cg.group_blackboards(1, 2)) == boards_bytes([r.board() for r in refs[1:]])
    # the tables alone: allowed.  (Bit T opens a byte, so stream 0's Predict has moved its tables: they are what
    # ctx_ref.c holds once it has predicted that bit, whatever the bit turns out to be.)
    assert T % 8 == 0
    ahead = cc.Ref(f.descs)
    ahead.run(x["bits"][0][:T + 1], values=False)
    assert ahead.export() != refs[0].export()
    assert cg.group_export() == joined([ahead.export()] + [r.export() for r in refs[1:]], 0, S)
    assert cg.group_export(1, 2) == joined([r.export() for r in refs], 1, 2)
    # new tables and boards for every stream, inside a byte: the object reads the boards again before its next step
    start, n_more = 13, 20
    src = [f.bits[8 * o:] for o in (700, 20, 333)]
    refs2 = []
    for s in range(S):
        r = cc.Ref(f.descs)
        r.run(src[s][:start], values=False)
        refs2.append(r)
    sec = joined([r.export() for r in refs2], 0, S)
    cg.group_import(sec[0], sec[1])
    set_boards = [r.board() for r in refs2]
    cg.set_group_blackboards(set_boards)
    assert boards_bytes(cg.group_blackboards()) == boards_bytes(set_boards)   # (set cleared stream 0's flag)
    # stream 0's outstanding Learn repeats the bit its new board already holds; then every stream predicts
    step.what[:] = [tc.LEARN | tc.PREDICT, tc.PREDICT, tc.PREDICT]
    step.bits[:] = [set_boards[0].new_bit, 0, 0]
    for t in range(n_more):
        records(t)
        step.step()
        step.what[:] = tc.LEARN
        step.bits[:] = [src[s][start + t] for s in range(S)]
        step.step()
        for s in range(S):
            refs2[s].run(src[s][start + t:start + t + 1], values=False)
        assert boards_bytes(cg.group_blackboards()) == boards_bytes([r.board() for r in refs2]), t
        step.what[:], step.bits[:] = tc.PREDICT, 0
    assert start + n_more > 24   # two bytes were opened on the way
    assert cg.group_export() == joined([r.export() for r in refs2], 0, S)
    step.close()
    cg.close()
    mg.close()


def test_zz_release_the_shared_bank():
    x = _state.pop("mixed", None)
    if x:
        x["g"].close()
