"""gmx_match_group_export / gmx_match_group_import (gmx_match_ckpt.hip): the checkpoint of a whole Match group in one
call, against the per-stream calls (unchanged code), the bytes the reference recorded (tests/golden/match_*.npz) and
tests/helpers/match_ref.c.  Tolerance 0 everywhere: sections are compared byte for byte, floats as bit patterns."""
import ctypes as C
import struct

import numpy as np
import pytest

import match_common as mc
from gmix_amd import GmxError
from gmix_amd.match import CKPT_CHUNK

pytestmark = pytest.mark.gpu
GMX_ERR_INVALID, GMX_ERR_FORMAT = -1, -6
_state = {}


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cap_for(f):
    return len(f.data) + 64


def positions(f):
    """Bits each stream of the group has run: never run, inside the first byte, 1 000 bits, the whole fixture, 40 000
    bits (match_stock: three streams, to keep memory and time small)."""
    if f.name == "match_stock":
        return [0, 3, f.T]
    return [0, 3, 1000, f.T, min(40000, f.T)]


def run_to(gpu, g, f, pos, start=None, chunk=8192):
    """Stream s runs bits [start[s], pos[s]) of the fixture through gmx_match_run_ragged; -> slots, act, longest per
    stream."""
    S = g.S
    done = np.array(start if start is not None else [0] * S, np.int64)
    pos = np.asarray(pos, np.int64)
    b = gpu.MatchBatch(g, chunk)
    P = [[] for _ in range(S)]
    A = [[] for _ in range(S)]
    Lm = [[] for _ in range(S)]
    while (done < pos).any():
        n = np.minimum(chunk, pos - done).astype(np.uint64)
        for s in range(S):
            k, d = int(n[s]), int(done[s])
            b.set_records(s, f.ctx[d:d + k], f.bc[d:d + k], f.bits[d:d + k])
        b.upload(int(n.max()))
        g.run_ragged(b, n)
        b.download(int(n.max()))
        b.wait()
        for s in range(S):
            k = int(n[s])
            P[s].append(u32(b.predictions[s, :k]).copy())
            A[s].append(b.active[s, :k].copy())
            Lm[s].append(b.longest[s, :k].copy())
        done += n.astype(np.int64)
    b.close()
    return [np.concatenate(p) if p else np.zeros((0, g.K), np.uint32) for p in P], \
           [np.concatenate(a) if a else np.zeros((0, g.K), np.uint8) for a in A], \
           [np.concatenate(l) if l else np.zeros(0, np.uint32) for l in Lm]


def ref_at(f, p):
    r = mc.Ref(f.models())
    r.run(f.ctx[:p], f.bc[:p], f.bits[:p])
    return r


def state(gpu, name):
    """A group of the fixture's models with its streams at positions(f), computed once: the group call's result, the
    per-stream calls' and match_ref.c's.  The small groups stay alive for the tests that only read them."""
    if name in _state:
        return _state[name]
    f = mc.fixture(name)
    pos = positions(f)
    g = gpu.MatchGroup(f.models(), cap_for(f), len(pos))
    run_to(gpu, g, f, pos)
    x = dict(f=f, pos=pos, full=g.export_all(), per=[g.export(s) for s in range(len(pos))],
             slots=[g.slot_values(s) for s in range(len(pos))], ref=[ref_at(f, p).export() for p in pos], g=g)
    if name == "match_stock":   # (92 MiB of tables a stream)
        g.close()
        x["g"] = None
    _state[name] = x
    return x


def sections(full, K):
    lb, off, sb = full
    return [(lb[off[i]:off[i + 1]], sb[11 * K * i:11 * K * (i + 1)]) for i in range(len(off) - 1)]


def join(secs):
    off = [0]
    for l, _ in secs:
        off.append(off[-1] + len(l))
    return b"".join(l for l, _ in secs), off, b"".join(s for _, s in secs)


def parse(sec, tables):
    """-> history size, [(count, dense, offset of the body, bytes of the body)] of a long section"""
    hs = struct.unpack_from("<Q", sec, 0)[0]
    p = 8 + hs
    out = []
    for t in tables:
        c = struct.unpack_from("<I", sec, p)[0]
        dense = not (c < (5.0 / 9.0) * t)
        body = 5 * t if dense else 9 * c
        out.append((c, dense, p + 4, body))
        p += 4 + body + 2048
    assert p == len(sec)
    return hs, out


def ops(g):
    v = C.c_uint64(0)
    g.L.gmx_debug_match_group_ops.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    assert g.L.gmx_debug_match_group_ops(g.h, C.byref(v)) == 0
    return v.value


# ---- 1. equal to the per-stream call and to the reference's bytes ---------------------------------------------------
@pytest.mark.parametrize("name", ["match_tiny", "match_k8", "match_stock"])
def test_equals_the_per_stream_call_and_the_reference(gpu, name):
    x = state(gpu, name)
    f, pos = x["f"], x["pos"]
    lb, off, sb = x["full"]
    assert off[0] == 0 and len(off) == len(pos) + 1 and off[-1] == len(lb) and len(sb) == 11 * f.K * len(pos)
    assert all(off[i] < off[i + 1] for i in range(len(pos)))
    for i, sec in enumerate(sections(x["full"], f.K)):
        assert sec == x["per"][i], (i, "group call != gmx_match_export")
        assert sec == x["ref"][i], (i, "group call != match_ref.c at bit", pos[i])
        if pos[i] == f.T:
            assert sec == (f.long, f.short), (i, "group call != the reference's recorded bytes")
    assert f.T in pos


def test_the_fixtures_reach_both_branches_and_an_empty_model(gpu):
    """A condition on the inputs of the test above: across the three fixtures a sparse model with records, a dense one
    and a model with count 0 have all been written by the group call."""
    seen = set()
    for name in ["match_tiny", "match_k8", "match_stock"]:
        x = state(gpu, name)
        for l, _ in sections(x["full"], x["f"].K):
            for c, dense, _, _ in parse(l, x["f"].tables)[1]:
                seen.add("dense" if dense else ("empty" if c == 0 else "sparse"))
    assert seen == {"dense", "sparse", "empty"}, seen


# ---- 2. sizing, capacity, windows -------------------------------------------------------------------------------------
def test_sizing_capacity_and_windows(gpu):
    x = state(gpu, "match_k8")
    g, f = x["g"], x["f"]
    S, K, L = g.S, f.K, g.L
    lb, off, sb = x["full"]
    vp = C.c_void_p
    # the sizing call fills long_off and writes nothing (there is nothing it could write to)
    o = (C.c_size_t * (S + 1))(*([77] * (S + 1)))
    assert L.gmx_match_group_export(g.h, 0, S, None, 0, o, None) == 0
    assert list(o) == off
    # one byte short: refused, the canaries stand, long_off is filled all the same
    need = off[-1]
    big = np.full(need + 64, 0xA5, np.uint8)
    small = np.full(11 * K * S + 64, 0x5A, np.uint8)
    o = (C.c_size_t * (S + 1))(*([77] * (S + 1)))
    assert L.gmx_match_group_export(g.h, 0, S, big.ctypes.data_as(vp), need - 1, o, small.ctypes.data_as(vp)) \
        == GMX_ERR_INVALID
    assert (big == 0xA5).all() and (small == 0x5A).all() and list(o) == off
    # exactly enough: written, and nothing behind it
    assert L.gmx_match_group_export(g.h, 0, S, big.ctypes.data_as(vp), need, o, small.ctypes.data_as(vp)) == 0
    assert big[:need].tobytes() == lb and (big[need:] == 0xA5).all()
    assert small[:11 * K * S].tobytes() == sb and (small[11 * K * S:] == 0x5A).all()
    # a window
    wl, woff, ws = g.export_all(first=1, count=2)
    assert woff == [0, off[2] - off[1], off[3] - off[1]]
    assert wl == lb[off[1]:off[3]] and ws == sb[11 * K:33 * K]
    wl, woff, ws = g.export_all(first=S - 1)
    assert (wl, ws) == x["per"][S - 1] and woff == [0, len(wl)]
    # arguments
    for first, count in [(-1, 1), (0, 0), (0, -1), (0, S + 1), (S, 1), (S - 1, 2)]:
        assert L.gmx_match_group_export(g.h, first, count, None, 0, o, None) == GMX_ERR_INVALID, (first, count)
        assert L.gmx_match_group_import(g.h, first, count, big.ctypes.data_as(vp), o, small.ctypes.data_as(vp)) \
            == GMX_ERR_INVALID, (first, count)
    assert L.gmx_match_group_export(g.h, 0, S, None, 0, None, None) == GMX_ERR_INVALID
    assert L.gmx_match_group_export(g.h, 0, S, big.ctypes.data_as(vp), need, o, None) == GMX_ERR_INVALID
    assert L.gmx_match_group_import(g.h, 0, S, None, o, small.ctypes.data_as(vp)) == GMX_ERR_INVALID
    assert L.gmx_match_group_import(g.h, 0, S, big.ctypes.data_as(vp), o, None) == GMX_ERR_INVALID
    assert L.gmx_match_group_import(g.h, 0, S, big.ctypes.data_as(vp), None, small.ctypes.data_as(vp)) == GMX_ERR_INVALID
    with pytest.raises(GmxError) as e:
        g.export_all(first=2, count=S)
    assert e.value.status == GMX_ERR_INVALID
    assert g.export_all() == x["full"]   # nothing of all that moved the banks


# ---- 3. import round trip and continuation ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["match_tiny", "match_k8", "match_stock"])
def test_import_round_trip_and_continuation(gpu, name):
    x = state(gpu, name)
    f, pos = x["f"], x["pos"]
    K = f.K
    secs = sections(x["full"], K)[1:]       # streams 1.. of the group go to streams 0.. of a fresh one
    n = len(secs)
    g = gpu.MatchGroup(f.models(), cap_for(f), n + 1)
    fresh = g.export(n)
    slots = [((np.arange(K) + 1) * (0.25 + s)).astype(np.float32) for s in range(n + 1)]
    for s in range(n + 1):
        g.set_slot_values(slots[s], s & 1, stream=s)
    g.import_all(*join(secs))
    for s in range(n + 1):
        v, nb = g.slot_values(s)
        assert np.array_equal(u32(v), u32(slots[s])) and nb == (s & 1), s   # the import left them alone
    assert g.export_all(count=n) == join(secs)
    assert [g.export(s) for s in range(n)] == secs
    assert g.export(n) == fresh and g.history_size(n) == 0                # the stream behind the window was not touched
    # 64 more bytes, beside match_ref.c restored from the same sections
    more = 512
    start = [p if p + more <= f.T else 0 for p in pos[1:]]
    refs = []
    for s in range(n):
        r = mc.Ref(f.models())
        r.import_(*secs[s])
        r.set_slots(slots[s], s & 1)
        refs.append(r)
    P, A, Lm = run_to(gpu, g, f, [a + more for a in start] + [0], start=start + [0])
    for s in range(n):
        a = start[s]
        wp, wa, wl = refs[s].run(f.ctx[a:a + more], f.bc[a:a + more], f.bits[a:a + more])
        assert np.array_equal(P[s], wp), s
        assert np.array_equal(A[s], wa) and np.array_equal(Lm[s], wl), s
        assert g.history_size(s) == refs[s].history_size(), s
        assert g.export(s) == refs[s].export(), s
    g.close()


# ---- 4. chunk edges and the branch boundary, with hand-made sections ------------------------------------------------
def make_section(rng, hist, tables, valid):
    """valid[j]: {key: pointer} of model j -> (long section, short section) as the reference writes them"""
    out = [struct.pack("<Q", len(hist)), bytes(hist)]
    for t, v in zip(tables, valid):
        ks = sorted(v)
        keys = np.array(ks, np.uint32)
        ptrs = np.array([v[k] for k in ks], np.uint32)
        out.append(struct.pack("<I", len(keys)))
        if len(keys) < (5.0 / 9.0) * t:
            rec = np.zeros((len(keys), 9), np.uint8)
            rec[:, 0:4] = keys.view(np.uint8).reshape(-1, 4)
            rec[:, 4:8] = ptrs.view(np.uint8).reshape(-1, 4)
        else:
            full = np.zeros(t, np.uint32)
            full[keys] = ptrs
            rec = np.zeros((t, 5), np.uint8)
            rec[:, 0:4] = full.view(np.uint8).reshape(-1, 4)
        out.append(rec.tobytes())
        out.append(rng.integers(0, 1 << 32, 512, dtype=np.uint64).astype(np.uint32).tobytes())  # 256 floats, 256 ints
    short = b""
    for j in range(len(tables)):
        cm = int(rng.integers(0, len(hist))) if len(hist) else 0
        short += struct.pack("<QBBB", cm, int(rng.integers(0, 256)), [0, 1, 2, 4, 8, 16, 32, 64, 128][(j + cm) % 9],
                             int(rng.integers(0, 256)))
    return b"".join(out), short


def test_chunk_edges_and_the_branch_boundary(gpu):
    rng = np.random.default_rng(5)
    big, nine, small = 40000, 2304, 100          # 2 chunks + 7 232 entries; 9 x 256; less than a chunk
    tables = [big, nine, small]
    assert big > 2 * CKPT_CHUNK and big % CKPT_CHUNK and nine == 9 * 256

    def ptr(k):
        return 1 + (7 * k) % 63                  # pointers 1..63 into a 64-byte history

    edge = {k: ptr(k) for k in (0, CKPT_CHUNK - 1, CKPT_CHUNK, 2 * CKPT_CHUNK - 1, 2 * CKPT_CHUNK, big - 1)}
    some = rng.permutation(nine)
    hist = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    secs = [
        make_section(rng, hist, tables, [edge, {int(k): ptr(int(k)) for k in some[:1279]}, {}]),
        make_section(rng, hist, tables, [edge, {int(k): ptr(int(k)) for k in some[:1280]}, {k: ptr(k) for k in range(small)}]),
        make_section(rng, hist, tables, [{k: ptr(k) for k in range(t)} for t in tables]),   # every entry valid
        make_section(rng, b"", tables, [{}, {}, {}]),                                       # empty tables, no history
    ]
    shape = [[(c, d) for c, d, _, _ in parse(l, tables)[1]] for l, _ in secs]
    assert shape[0] == [(6, False), (1279, False), (0, False)]      # 1 279 < 5/9 x 2 304 = 1 280: sparse
    assert shape[1] == [(6, False), (1280, True), (small, True)]    # 1 280: dense
    assert shape[2] == [(big, True), (nine, True), (small, True)] and shape[3] == [(0, False)] * 3
    g = gpu.MatchGroup([(t, 60) for t in tables], 64, len(secs) + 1)
    fresh = g.export(len(secs))
    g.import_all(*join(secs))
    assert g.export_all(count=len(secs)) == join(secs)
    assert [g.export(s) for s in range(len(secs))] == secs
    assert g.export(len(secs)) == fresh
    assert [g.history_size(s) for s in range(len(secs))] == [64, 64, 64, 0]
    # the other order and a window inside: sections land where `first` says, over what the banks held
    g.import_all(*join([secs[3], secs[2]]), first=1)
    assert g.export_all() == join([secs[0], secs[3], secs[2], secs[3], fresh])
    g.close()


# ---- 5. all or nothing ------------------------------------------------------------------------------------------------
def test_a_bad_section_anywhere_leaves_every_bank_alone(gpu):
    x = state(gpu, "match_k8")
    f = x["f"]
    K, S = f.K, len(x["pos"])
    good = sections(x["full"], K)
    lb, off, sb = x["full"]
    cap = cap_for(f)
    g = gpu.MatchGroup(f.models(), cap, S)
    run_to(gpu, g, f, [8 * 700 * s + 2000 for s in range(S)], start=[8 * 700 * s for s in range(S)])  # other state
    before = g.export_all()
    assert before != x["full"]

    def first_sparse(i, least):
        for c, dense, at, _ in parse(good[i][0], f.tables)[1]:
            if not dense and c >= least:
                return off[i] + at
        raise AssertionError(("no sparse model with records in section", i))

    bad = {}
    a = first_sparse(S - 1, 2)
    y = bytearray(lb)
    y[a:a + 9], y[a + 9:a + 18] = lb[a + 9:a + 18], lb[a:a + 9]
    bad["a key pair swapped in the last stream"] = (bytes(y), off, sb)
    a = first_sparse(2, 1)
    y = bytearray(lb)
    struct.pack_into("<I", y, a + 4, parse(good[2][0], f.tables)[0])
    bad["a pointer at the history size in the middle stream"] = (bytes(y), off, sb)
    a = first_sparse(3, 1)
    y = bytearray(lb)
    y[a + 8] = 1
    bad["a fifth pointer byte"] = (bytes(y), off, sb)
    y = bytearray(sb)
    y[11 * K * 1 + 9] = 3
    bad["bit_pos_ 3 in a short section"] = (lb, off, bytes(y))
    o = list(off)
    o[2] -= 5
    bad["an offset that truncates a section"] = (lb, o, sb)
    y = bytearray(lb)
    struct.pack_into("<Q", y, off[0], cap + 1)
    bad["a history above the capacity"] = (bytes(y), off, sb)
    for what, args in bad.items():
        with pytest.raises(GmxError) as e:
            g.import_all(*args)
        assert e.value.status == GMX_ERR_FORMAT, what
        assert g.export_all() == before, what
    g.import_all(lb, off, sb)
    assert g.export_all() == x["full"]
    g.close()


# ---- 6. round trips do not grow with the stream count ---------------------------------------------------------------
def test_round_trips_do_not_depend_on_the_stream_count(gpu):
    x = state(gpu, "match_k8")
    f = x["f"]
    S = len(x["pos"])
    src = x["g"]
    g = gpu.MatchGroup(f.models(), cap_for(f), S)
    cost = {}
    for count in (1, S):
        n0 = ops(src)
        part = src.export_all(count=count)
        n1 = ops(src)
        m0 = ops(g)
        g.import_all(*part)
        m1 = ops(g)
        cost[count] = (n1 - n0, m1 - m0)
    assert cost[1] == cost[S], cost
    assert cost[1][0] > 0 and cost[1][1] > 0, cost
    assert g.export_all() == x["full"]
    g.close()


# ---- 7. beside the lock step ------------------------------------------------------------------------------------------
def test_beside_the_lock_step(gpu, oracle):
    import test_gpu_chainstep_match as csm
    f = mc.fixture("match_tiny")
    S, T, half = 3, 400, 203
    xs = csm.small_chain(oracle, f, S, T, [61 * s for s in range(S)], [31, 32, 39], False, 60)
    g = gpu.MatchGroup(xs["models"], 1024, S)
    mg = gpu.MixerGroup(xs["topo"], S)
    cs = gpu.ChainStep(mg)
    cs.attach_match(g, csm.COLS)
    csm.lockstep(gpu, cs, xs, 0, half)
    per = [g.export(s) for s in range(S)]
    assert g.export_all() == join(per)
    for s in range(S):
        r = mc.Ref(f.models())
        r.run(xs["mctxw"][s, :half], xs["bc"][s, :half], xs["bits"][s, :half])
        assert per[s] == r.export(), s
    csm.lockstep(gpu, cs, xs, half, T)
    cs.close()
    csm.assert_match_state(g, [m["ref"] for m in xs["m"]])
    assert g.export_all() == join([m["ref"].export() for m in xs["m"]])
    g.close()
    mg.close()
