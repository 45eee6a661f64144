"""tests/helpers/ctx_ref.c, the plain-C restatement of the context variables, against the fixtures the reference
produced (values at every bit, IndirectHash sections and blackboards at the recorded positions) and against the numpy
MurmurHash3 of scripts/bench_match.py on the skip columns.  No device is needed."""
import importlib.util
import os

import numpy as np
import pytest

import ctx_common as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", cc.FIXTURES)
def test_values_sections_and_boards(name):
    f = cc.fixture(name)
    ref = cc.Ref(f.descs)
    want = f.values()
    at = 0
    for p, pos in enumerate(f.positions):
        got = ref.run(f.bits[at:pos])
        assert np.array_equal(got, want[at:pos]), (name, p)
        at = pos
        data, off = ref.export()
        assert data == f.section(p), (name, p)
        assert [data[off[h]:off[h + 1]] for h in range(f.H)] == f.sections[p]
        assert cc.board_bytes(ref.board()) == cc.board_bytes(f.boards[p]), (name, p)
    assert at == f.T


def test_fixture_coverage():
    tiny, stock = cc.fixture("ctx_tiny"), cc.fixture("ctx_stock")
    for f in (tiny, stock):
        assert f.meta["same_entry"] >= 20 and f.meta["wraps"] >= 1
        assert f.positions[:2] == [0, 3] and 8 * 1001 + 5 in f.positions and f.T in f.positions
    # both WriteToDisk branches, and the boundary count == table_size / 2 (the first dense count) for one table
    b = tiny.boundary
    sec = tiny.sections[b["position_index"]][b["hash"]]
    assert int.from_bytes(sec[:4], "little") == b["table_size"] // 2 and len(sec) == 4 + 4 * b["table_size"] + 12
    lens = [(len(s), f.descs[f.hash_vars[h]].table_size) for f in (tiny, stock) for row in f.sections
            for h, s in enumerate(row)]
    assert any(n == 16 + 4 * t for n, t in lens) and any(n != 16 + 4 * t for n, t in lens)
    # a SkipContext fires at the very first Predict
    assert all(stock.byte_vals[0][v] != 0 for v, k in enumerate(stock.kinds) if k == 5)


def test_resume_inside_a_byte_and_import():
    f = cc.fixture("ctx_tiny")
    a = cc.Ref(f.descs)
    a.run(f.bits[:8013], values=False)
    b = cc.Ref(f.descs)
    b.import_(a.export()[0])
    b.set_board(a.board())
    assert np.array_equal(b.run(f.bits[8013:9000]), f.values()[8013:9000])


def test_skip_columns_equal_the_numpy_murmur():
    spec = importlib.util.spec_from_file_location("bench_match", os.path.join(ROOT, "scripts", "bench_match.py"))
    bm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bm)
    f = cc.fixture("ctx_stock")
    hist = np.concatenate([np.zeros(16, np.uint64), f.data.astype(np.uint64)])
    n = len(f.data)
    for v, d in enumerate(f.descs):
        if d.kind != 5:
            continue
        # row i of byte_vals is the value while byte i is coded: GetRecentByte(k) is byte i - 1 - k
        key = np.zeros(n, np.uint64)
        for k in list(d.bytes_to_use)[:d.n_bytes]:
            key = (key << np.uint64(8)) + hist[16 - 1 - k:16 - 1 - k + n]
        assert np.array_equal(bm.murmur3_u64(key), f.byte_vals[:, v]), f.names[v]
