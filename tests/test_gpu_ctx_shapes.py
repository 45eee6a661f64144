"""The context banks on the device (gmix_amd/csrc/gmx_ctx.hip) away from the two recorded descriptor lists: the seeded
cases of tests/ctx_shapes.py -- 0 / 1 / 16 hash tables, 1 / 64 variables, random interval maps and skips,
byte_plus_recent and recent_byte at every index -- one launch longer than the 1 000-byte history ring, tables of several
checkpoint chunks in both WriteToDisk branches, a ragged run into 64 Indirect models.  Expected values come from
tests/helpers/ctx_ref.c, which tests/test_oracle_ctx_shapes.py pins to the reference on the same cases (for
byte_plus_recent with index 2..9, which the reference does not have, ctx_ref.c is the definition include/gmxmix.h
documents: (recent_bytes[index] << 8) + bit_context).  Tolerance 0: values as uint32, sections and boards as bytes."""
import numpy as np
import pytest

import ctx_common as cc
import ctx_harness
import ctx_shapes as cs
import goldenlib
from test_gpu_ctx import chunks_of, run_chunks

pytestmark = pytest.mark.gpu

POISON = 0xFFFFFFFF
_refs = {}


def reference(name, offset, T):
    """ctx_ref.c over T bits of the case's stream from byte `offset`: (values, (section, offsets), board).  Shared;
    never modified."""
    key = (name, offset, T)
    if key not in _refs:
        r = cc.Ref(cs.as_descs(cs.descs(name)))
        v = r.run(np.unpackbits(cs.stream(name))[8 * offset:8 * offset + T])
        v.setflags(write=False)
        _refs[key] = (v, r.export(), cc.board_bytes(r.board()))
    return _refs[key]


def assert_state(g, s, ref, tag):
    """Export, per-table offsets and blackboard of stream s against a cc.Ref (or reference()'s pair)."""
    sec, off = ref.export() if isinstance(ref, cc.Ref) else ref[0]
    board = cc.board_bytes(ref.board()) if isinstance(ref, cc.Ref) else ref[1]
    data, goff = g.export(s)
    assert goff == off, (tag, s)
    assert data == sec, (tag, s)
    assert cc.board_bytes(g.blackboard(s)) == board, (tag, s)


@pytest.mark.parametrize("name", list(cs.CASES))
def test_case_in_chunks_streams_offset_against_each_other(gpu, name):
    c = cs.case(name)
    named = cs.descs(name)
    descs = cs.as_descs(named)
    bits = np.unpackbits(cs.stream(name))
    T, offs = cs.GPU_BITS, cs.offsets(c.S)
    cap, launch = c.chunking
    assert launch % 8 and launch <= cap and 8 * offs[-1] + T <= len(bits)
    g = gpu.CtxGroup(descs, c.S)
    assert (g.V, g.H) == (c.V, c.H)
    b = gpu.CtxBatch(g, cap)
    got = run_chunks(g, b, [bits[8 * o:8 * o + T] for o in offs], chunks_of(T, launch))
    for s, o in enumerate(offs):
        want, exp, board = reference(name, o, T)
        bad = np.argwhere(got[s] != want)
        assert len(bad) == 0, (name, s, "first differing (bit, variable):", bad[:5], [named[v][0] for _, v in bad[:5]])
        assert_state(g, s, (exp, board), name)
    if c.H == 0:
        assert g.export(0) == (b"", [0])
        g.import_(b"")
        assert cc.board_bytes(g.blackboard(0)) == reference(name, offs[0], T)[2]
    b.close()
    g.close()


def test_one_launch_longer_than_the_ring(gpu):
    """9 001 bits complete 1 125 bytes: more than the ring holds, so the commit kernel writes only the newest 1 000 (its
    c0 branch).  Stream 0 is fresh; stream 1 has coded 1 003 bits, so its long run opens inside a byte with 125 bytes
    in the ring.  Then 77 bits more.  (Without that branch an older and a newer byte race for one slot and the newer
    usually lands last: this pins what the ring holds after such a run, it cannot pin the branch itself.)"""
    name = cs.LONG_RUN_CASE
    named = cs.descs(name)
    descs = cs.as_descs(named)
    assert (len(descs), sum(d.kind == 6 for d in descs)) == (64, 16)
    data = np.random.default_rng(31).integers(0, 256, (2, 1300), dtype=np.uint8)
    bits = [np.unpackbits(d) for d in data]
    pre, T1, T2 = 1003, 9001, 77
    g = gpu.CtxGroup(descs, 2)
    b = gpu.CtxBatch(g, T1)
    refs = [cc.Ref(descs) for _ in range(2)]
    b.bits[1, :pre] = bits[1][:pre]
    b.upload(pre)
    g.run_ragged(b, [0, pre])
    refs[1].run(bits[1][:pre], values=False)
    assert_state(g, 1, refs[1], "advance")
    at = [0, pre]
    for n in (T1, T2):
        for s in range(2):
            b.bits[s, :n] = bits[s][at[s]:at[s] + n]
        b.upload(n)
        g.run(b, n)
        b.download(n)
        b.wait()
        for s in range(2):
            want = refs[s].run(bits[s][at[s]:at[s] + n])
            bad = np.argwhere(b.values[s, :n] != want)
            assert len(bad) == 0, (n, s, bad[:5], [named[v][0] for _, v in bad[:5]])
            at[s] += n
            bb, rb = g.blackboard(s), refs[s].board()
            assert bb.rotating_history_pos == rb.rotating_history_pos == (at[s] - 1) // 8 % cs.RING, (n, s)
            assert bytes(bb.rotating_history) == bytes(rb.rotating_history), (n, s)
            assert_state(g, s, refs[s], n)
    b.close()
    g.close()


def test_big_tables_checkpoint_in_both_branches(gpu):
    """40 000 random bytes into sixteen tables, seven of them larger than or at one chunk of the checkpoint kernels:
    export at 25 000 and at 40 000 bytes, import into stream 1 of a second bank, both continued."""
    name = "big_tables"
    descs = cs.as_descs(cs.descs(name))
    sizes = [d.table_size for d in descs if d.kind == 6]
    bits = np.unpackbits(cs.stream(name))
    marks = [8 * cs.BIG_MID_BYTES, 8 * cs.BIG.n_bytes]
    tail = np.unpackbits(np.random.default_rng(77).integers(0, 256, 64, dtype=np.uint8))
    # ---- ctx_ref.c alone: the two exports and what the tables' counts say about them
    ref = cc.Ref(descs)
    want, at = [], 0
    for m in marks:
        ref.run(bits[at:m], values=False)
        at = m
        sec, off = ref.export()
        parts = [sec[off[h]:off[h + 1]] for h in range(len(sizes))]
        want.append((sec, off, cc.board_bytes(ref.board()), ref.board(),
                     [(t, ctx_harness.section_count(p), ctx_harness.is_dense(p, t)) for t, p in zip(sizes, parts)]))
    tail_want = ref.run(tail)
    mid, end = want[0][4], want[1][4]
    chunk = cs.CKPT_CHUNK
    assert sum(1 for t, n, d in mid if not d and n > chunk) >= 2, mid       # the scatter kernel's second pass, twice
    assert any(d and t > chunk and t % 256 for t, n, d in end), end         # a dense multi-chunk table, odd size
    assert any(not d and n > chunk for t, n, d in end), end
    assert any(d for _, _, d in end) and any(not d for _, _, d in end)
    # ---- the device
    g = gpu.CtxGroup(descs, 1)
    b = gpu.CtxBatch(g, cs.BIG.chunking[0], values=False)
    g2 = gpu.CtxGroup(descs, 2)
    at = 0
    for m, (sec, off, board, board_obj, _) in zip(marks, want):
        for n in chunks_of(m - at, cs.BIG.chunking[1]):
            b.bits[0, :n] = bits[at:at + n]
            b.upload(n)
            g.run(b, n)
            b.wait()
            at += n
        data, goff = g.export(0)
        assert goff == off and data == sec, m
        assert cc.board_bytes(g.blackboard(0)) == board, m
        g2.import_(data, stream=1)
        g2.set_blackboard(board_obj, stream=1)
        assert g2.export(1) == (sec, off), m
    b.close()
    fresh = cc.Ref(descs)
    assert g2.export(0) == fresh.export()    # import touched stream 1 alone
    # ---- both banks go on for 64 bytes
    n = len(tail)
    b1, b2 = gpu.CtxBatch(g, n), gpu.CtxBatch(g2, n)
    b1.bits[0, :n] = tail
    b2.bits[1, :n] = tail
    b1.upload(n)
    b2.upload(n)
    g.run(b1, n)
    g2.run_ragged(b2, [0, n])
    for x in (b1, b2):
        x.download(n)
        x.wait()
    assert np.array_equal(b1.values[0], tail_want) and np.array_equal(b2.values[1], tail_want)
    assert_state(g, 0, ref, "continued")
    assert_state(g2, 1, ref, "continued import")
    for x in (b1, b2, g, g2):
        x.close()


IND_MIX = [(256, 0.02), (3, 0.1), (4096, 0.005), (1, 0.5), (65536, 0.02)]   # tests/test_gpu_indirect.py's models


def test_ragged_run_with_targets_into_64_indirect_models(gpu, oracle):
    """gmx_ctx_run_ragged with targets, on the widest record the banks admit: 64 variables routed into the 64 columns
    of an Indirect batch, some to two or three columns, four columns left to the host.  A stream whose count is 0 keeps
    its context state, its Indirect state -- and its rows of the target batch, which a last round reads."""
    S, K = 5, 64
    named = cs.descs(cs.LONG_RUN_CASE)
    descs = cs.as_descs(named)
    V = len(descs)
    bc_var = [k for _, k, _ in named].index("bit_context")
    rt = cs.route(named, K, seed=9, unrouted=4, repeats=12)
    kinds = {named[v][1] for v in rt if v >= 0}
    assert kinds == {k for _, k, _ in named} and len(kinds) == 7
    reps = np.bincount([v for v in rt if v >= 0], minlength=V)
    assert (reps == 2).any() and (reps == 3).any() and rt.count(-1) == 4
    _, z = goldenlib.load("ind_tiny_dense")
    tabs = (z["ns_next"], z["rm_next"])
    # (two tables of 65 536 contexts, not thirteen: the oracle walks every table for each export it is asked for)
    models = [IND_MIX[i % len(IND_MIX)] if i % len(IND_MIX) != 4 or i in (4, 39) else IND_MIX[2] for i in range(K)]
    assert {t for t, _ in models} == {t for t, _ in IND_MIX}
    rounds = [[0, 13, 64, 1, 1000], [9, 0, 1000, 7, 0], [300] * 5]
    probe = 24   # the last round: stream 0 sits the context launch out, its Indirect models read what the host staged
    rng = np.random.default_rng(55)
    data = rng.integers(0, 256, (S, 300), dtype=np.uint8)
    bits = [np.unpackbits(d) for d in data]
    host_cols = rng.integers(0, 5000, (S, 1000 // 8 + 1, K)).astype(np.uint32)   # byte-held host pattern
    cg = gpu.CtxGroup(descs, S)
    cb = gpu.CtxBatch(cg, 1000, values=False)
    ig = gpu.IndirectGroup(models, *tabs, S)
    ib = gpu.IndirectBatch(ig, 1000)
    tg = cg.targets(indirect=ib, ind_route=rt)
    crefs = [cc.Ref(descs) for _ in range(S)]
    irefs = [oracle.IndirectBank(models, *tabs) for _ in range(S)]
    routed = np.array([c for c, v in enumerate(rt) if v >= 0])
    at = [0] * S

    def u32(a):
        return np.ascontiguousarray(a, np.float32).view(np.uint32)

    host_bits = np.unpackbits(rng.integers(0, 256, 8, dtype=np.uint8))   # what the host codes in the last round
    host_bc = cc.bit_contexts(np.packbits(host_bits))

    def stage(s, n, poison):
        """The host's records of stream s: its pattern in every column -- then POISON wherever the bank is to write, or
        (a stream that sits the context launch out) bit contexts and bits of the host's own."""
        ctx = np.repeat(host_cols[s], 8, axis=0)[:n].copy()
        if poison:
            ctx[:, routed] = POISON
        ib.contexts[s, :n] = ctx
        ib.bit_contexts[s, :n] = POISON if poison else host_bc[:n]
        ib.bits[s, :n] = 0xFF if poison else host_bits[:n]
        return ctx

    def one_round(ctx_counts, ind_counts, tag, last=False):
        staged = {}
        for s in range(S):
            n = max(ctx_counts[s], ind_counts[s])
            staged[s] = stage(s, n, poison=ctx_counts[s] > 0)
            cb.bits[s, :ctx_counts[s]] = bits[s][at[s]:at[s] + ctx_counts[s]]
        ib.predictions[:] = np.float32(-1)
        ib.upload(max(ind_counts))
        cb.upload(max(ctx_counts))
        cg.run_ragged(cb, ctx_counts, targets=tg)
        ig.run_ragged(ib, ind_counts)
        ib.download(max(ind_counts))
        ib.wait()
        for s in range(S):
            n = ind_counts[s]
            if ctx_counts[s]:
                vals = crefs[s].run(bits[s][at[s]:at[s] + n])
                at[s] += n
                ctx = staged[s]
                for c in routed:
                    ctx[:, c] = vals[:, rt[c]]
                p, a = irefs[s].run(ctx, vals[:, bc_var], bits[s][at[s] - n:at[s]])
            elif n:
                p, a = irefs[s].run(staged[s], host_bc[:n], host_bits[:n])
            if n:
                assert np.array_equal(u32(ib.predictions[s, :n]), u32(p)), (tag, s)
                assert np.array_equal(ib.active[s, :n], a), (tag, s)
            if n == 0 or last:   # (a stream that ran shows its state in the predictions of its next round)
                assert ig.export(s) == irefs[s].export(), (tag, s)
            assert_state(cg, s, crefs[s], tag)

    for counts in rounds:
        one_round(counts, counts, counts)
    one_round([0, 5, 5, 5, 5], [probe, 5, 5, 5, 5], "probe", last=True)
    for x in (cb, ib, cg, ig):
        x.close()
