"""The context banks on the device (gmx_ctx_*, gmix_amd/csrc/gmx_ctx.hip) against the fixtures the reference produced
(tests/golden/ctx_*.npz) and, for chunkings, stream offsets and positions the fixtures do not record, against
tests/helpers/ctx_ref.c, which tests/test_ctx_ref.py pins to those fixtures.  Tolerance 0: uint32 equality."""
import struct

import numpy as np
import pytest

import ctx_common as cc
from gmix_amd import GmxError

pytestmark = pytest.mark.gpu

GMX_ERR_INVALID, GMX_ERR_FORMAT = -1, -6
_refs = {}


def reference(name, offset, T):
    """ctx_ref.c over bits [0, T) of the fixture's stream from byte `offset`: (values, section, board).  Shared by the
    cases; never modified."""
    key = (name, offset, T)
    if key not in _refs:
        f = cc.fixture(name)
        r = cc.Ref(f.descs)
        v = r.run(f.bits[8 * offset:8 * offset + T])
        v.setflags(write=False)
        _refs[key] = (v, r.export()[0], cc.board_bytes(r.board()))
    return _refs[key]


def run_chunks(g, b, streams, chunks):
    """streams: the bit arrays of the S streams (equal lengths); chunks: bits per launch -> values [S][T][V]"""
    T = len(streams[0])
    out = np.zeros((g.S, T, g.V), np.uint32)
    at = 0
    for n in chunks:
        for s in range(g.S):
            b.bits[s, :n] = streams[s][at:at + n]
        b.upload(n)
        g.run(b, n)
        b.download(n)
        b.wait()
        out[:, at:at + n] = b.values[:, :n]
        at += n
    assert at == T
    return out


def chunks_of(T, n):
    return [n] * (T // n) + ([T % n] if T % n else [])


@pytest.mark.parametrize("chunk", [7, 64, 1000])
@pytest.mark.parametrize("name", cc.FIXTURES)
def test_whole_fixture_in_chunks(gpu, name, chunk):
    """Runs begin and end inside bytes (7), at byte boundaries (64), and inside bytes again with several tiles of the
    expand kernel per launch (1000)."""
    f = cc.fixture(name)
    g = gpu.CtxGroup(f.descs, 1)
    b = gpu.CtxBatch(g, 1000)
    got = run_chunks(g, b, [f.bits], chunks_of(f.T, chunk))
    want = f.values()
    bad = np.argwhere(got[0] != want)
    assert len(bad) == 0, (name, chunk, "first differing (bit, variable):", bad[:5], [f.names[v] for _, v in bad[:5]])
    last = f.positions.index(f.T)
    data, off = g.export(0)
    assert data == f.section(last)
    assert cc.board_bytes(g.blackboard(0)) == cc.board_bytes(f.boards[last])
    b.close()
    g.close()


@pytest.mark.parametrize("name", cc.FIXTURES)
def test_sections_and_blackboards_at_the_recorded_positions(gpu, name):
    """Never run, 3 bits in, 1 001 bytes + 5 bits, the end -- and for ctx_tiny the position at which the 100-entry
    table holds exactly table_size / 2 entries: the first count of the dense branch."""
    f = cc.fixture(name)
    g = gpu.CtxGroup(f.descs, 1)
    b = gpu.CtxBatch(g, 4096, values=False)
    assert g.bank_bytes >= sum(4 * f.descs[v].table_size for v in f.hash_vars)
    at = 0
    for p, pos in enumerate(f.positions):
        for n in chunks_of(pos - at, 4096):
            b.bits[0, :n] = f.bits[at:at + n]
            b.upload(n)
            g.run(b, n)
            b.wait()    # (the pinned bits are refilled for the next launch)
            at += n
        data, off = g.export(0)
        assert data == f.section(p), (name, p)
        assert [data[off[h]:off[h + 1]] for h in range(f.H)] == f.sections[p], (name, p)
        assert cc.board_bytes(g.blackboard(0)) == cc.board_bytes(f.boards[p]), (name, p)
    if f.boundary:
        sec = f.sections[f.boundary["position_index"]][f.boundary["hash"]]
        assert struct.unpack_from("<I", sec)[0] == f.boundary["table_size"] // 2
    with pytest.raises(GmxError):
        b.download(8)   # no values array without GMX_CTX_BATCH_VALUES
    with pytest.raises(GmxError):
        _ = b.values
    b.close()
    g.close()


@pytest.mark.parametrize("name,S", [("ctx_tiny", 1), ("ctx_stock", 5), ("ctx_tiny", 9), ("ctx_stock", 9)])
def test_streams_offset_against_each_other(gpu, name, S):
    """Partial waves of the chain kernel (four streams a wave); stream s begins 37 s + (s % 3) bytes into the data."""
    f = cc.fixture(name)
    T = 2600
    offs = [37 * s + s % 3 for s in range(S)]
    g = gpu.CtxGroup(f.descs, S)
    b = gpu.CtxBatch(g, 333)
    got = run_chunks(g, b, [f.bits[8 * o:8 * o + T] for o in offs], chunks_of(T, 333))
    for s, o in enumerate(offs):
        want, sec, board = reference(name, o, T)
        assert np.array_equal(got[s], want), (name, s)
        assert g.export(s)[0] == sec and cc.board_bytes(g.blackboard(s)) == board, (name, s)
    b.close()
    g.close()


def test_run_ragged(gpu):
    """One launch sequence for unequal counts; a stream with 0 sits the launch out and keeps its state."""
    f = cc.fixture("ctx_tiny")
    S = 5
    rounds = [[0, 13, 64, 1, 1000], [9, 0, 1000, 7, 0], [300, 300, 300, 300, 300]]
    g = gpu.CtxGroup(f.descs, S)
    b = gpu.CtxBatch(g, 1000)
    at = [0] * S
    refs = [cc.Ref(f.descs) for _ in range(S)]
    for counts in rounds:
        b.values[:] = 0xABABABAB
        for s, n in enumerate(counts):
            b.bits[s, :n] = f.bits[at[s]:at[s] + n]
        b.upload(max(counts))
        g.run_ragged(b, counts)   # (equal counts take the launch without a count list)
        b.download(max(counts))
        b.wait()
        for s, n in enumerate(counts):
            want = refs[s].run(f.bits[at[s]:at[s] + n])
            assert np.array_equal(b.values[s, :n], want), (counts, s)
            at[s] += n
            assert g.export(s)[0] == refs[s].export()[0], (counts, s)
            assert cc.board_bytes(g.blackboard(s)) == cc.board_bytes(refs[s].board()), (counts, s)
    with pytest.raises(GmxError) as e:
        g.run_ragged(b, [0, 0, 1001, 0, 0])
    assert e.value.status == GMX_ERR_INVALID
    b.close()
    g.close()


@pytest.mark.parametrize("name", cc.FIXTURES)
def test_import_and_resume_inside_a_byte(gpu, name):
    """The fixture's sections and blackboard of 1 001 bytes + 5 bits go into stream 2 of a fresh bank, which then codes
    64 more bytes; the other streams stay as constructed."""
    f = cc.fixture(name)
    p = f.positions.index(8 * 1001 + 5)
    g = gpu.CtxGroup(f.descs, 3)
    b = gpu.CtxBatch(g, 512)
    g.import_(f.section(p), stream=2)
    assert cc.board_bytes(g.blackboard(2)) == cc.board_bytes(f.boards[0])   # import leaves the blackboard alone
    g.set_blackboard(f.boards[p], stream=2)
    at = f.positions[p]
    b.bits[2, :512] = f.bits[at:at + 512]
    b.upload(512)
    g.run_ragged(b, [0, 0, 512])
    b.download(512)
    b.wait()
    assert np.array_equal(b.values[2, :512], f.values()[at:at + 512])
    ref = cc.Ref(f.descs)
    ref.run(f.bits[:at + 512], values=False)
    assert g.export(2)[0] == ref.export()[0]
    for s in (0, 1):
        assert g.export(s)[0] == f.section(0) and cc.board_bytes(g.blackboard(s)) == cc.board_bytes(f.boards[0])
    b.close()
    g.close()


def damaged_sections(f, good, off):
    """Five ways a section can be wrong, each in the sparse record of the 100-entry table."""
    h = f.names.index("hash_100")
    h = f.hash_vars.index(h)
    o = off[h]
    (cnt,) = struct.unpack_from("<I", good, o)
    assert 2 <= cnt < 50, "a sparse record with at least two pairs"
    out = {}
    out["truncated"] = good[:-5]
    x = bytearray(good)
    struct.pack_into("<I", x, o, cnt + 1)   # the count says one pair more than there is
    out["count"] = bytes(x)
    x = bytearray(good)
    x[o + 4:o + 12], x[o + 12:o + 20] = good[o + 12:o + 20], good[o + 4:o + 12]
    out["descending keys"] = bytes(x)
    x = bytearray(good)
    struct.pack_into("<I", x, o + 4 + 8 * (cnt - 1), 100)   # a key at the table's size
    out["key beyond the table"] = bytes(x)
    x = bytearray(good)
    struct.pack_into("<I", x, o + 8, 0)     # a zero value in a sparse record
    out["zero value"] = bytes(x)
    return out


def test_damaged_sections_leave_the_bank_unchanged(gpu):
    f = cc.fixture("ctx_tiny")
    T = 80
    donor = cc.Ref(f.descs)
    donor.run(f.bits[4000:4000 + T], values=False)
    good, off = donor.export()
    g = gpu.CtxGroup(f.descs, 2)
    b = gpu.CtxBatch(g, 600)
    b.bits[1, :597] = f.bits[:597]
    b.upload(597)
    g.run_ragged(b, [0, 597])
    before = (g.export(1)[0], cc.board_bytes(g.blackboard(1)))
    for what, sec in damaged_sections(f, good, off).items():
        with pytest.raises(GmxError) as e:
            g.import_(sec, stream=1)
        assert e.value.status == GMX_ERR_FORMAT, what
        assert (g.export(1)[0], cc.board_bytes(g.blackboard(1))) == before, what
    g.import_(good, stream=1)
    assert g.export(1)[0] == good and cc.board_bytes(g.blackboard(1)) == before[1]
    b.close()
    g.close()


def test_copy_reset_memory_usage(gpu):
    f = cc.fixture("ctx_tiny")
    T = 1003
    want, sec, board = reference("ctx_tiny", 0, T)
    g = gpu.CtxGroup(f.descs, 2)
    g2 = gpu.CtxGroup(f.descs, 3)
    b = gpu.CtxBatch(g, 1003)
    b2 = gpu.CtxBatch(g2, 64)
    b.bits[0, :T] = f.bits[:T]
    b.upload(T)
    g.run_ragged(b, [T, 0])
    g.copy_from(g, src_stream=0, dst_stream=1)      # within a bank
    g2.copy_from(g, src_stream=1, dst_stream=2)     # between banks
    for grp, s in ((g, 0), (g, 1), (g2, 2)):
        assert grp.export(s)[0] == sec and cc.board_bytes(grp.blackboard(s)) == board
    # the copy continues like the original (inside a byte: 1 003 = 125 bytes + 3 bits)
    b2.bits[2, :64] = f.bits[T:T + 64]
    b2.upload(64)
    g2.run_ragged(b2, [0, 0, 64])
    b2.download(64)
    b2.wait()
    assert np.array_equal(b2.values[2, :64], f.values()[T:T + 64])
    other = gpu.CtxGroup(f.descs[1:], 1)
    with pytest.raises(GmxError) as e:
        other.copy_from(g)
    assert e.value.status == GMX_ERR_INVALID
    other.close()
    g.reset()
    for s in range(2):
        assert g.export(s)[0] == f.section(0) and cc.board_bytes(g.blackboard(s)) == cc.board_bytes(f.boards[0])
    for v, d in enumerate(f.descs):
        want_bytes = {6: 36 + 4 * d.table_size, 4: 256 * 4 + 8 + 4, 5: 4 * d.n_bytes + 4}.get(d.kind, 0)
        assert g.memory_usage(v) == want_bytes, f.names[v]
    bb = g.blackboard(0)
    bb.last_byte = 5            # not what rotating_history holds
    with pytest.raises(GmxError):
        g.set_blackboard(bb)
    for x in (b, b2, g, g2):
        x.close()
