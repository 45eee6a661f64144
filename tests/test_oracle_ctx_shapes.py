"""tests/helpers/ctx_ref.c against the reference's own context objects (oracle/_ref/ref_ctx_harness, run live) on every
case of tests/ctx_shapes.py: seeded descriptor lists with 0 / 1 / 16 hash tables, 1 / 64 variables, random interval
maps, skips and byte indices, and big_tables' 40 000 random bytes into tables of several checkpoint chunks.  The GPU
tests of those shapes compare the kernels with ctx_ref.c; this pins ctx_ref.c to the reference where the two recorded
fixtures (tests/test_ctx_ref.py) do not reach.  Values at every bit, the IndirectHash sections with their per-table
split and the blackboards at every recorded position, byte for byte.  The recordings stay in a temporary directory.

byte_plus_recent keeps to index 0 / 1 here (reference_only): the reference has no other such field."""
import numpy as np
import pytest

import ctx_common as cc
import ctx_harness
import ctx_shapes as cs
from gmix_amd.ctx import desc_array


@pytest.fixture(scope="module")
def harness():
    if not ctx_harness.have_harness():
        pytest.skip(f"{ctx_harness.HARNESS} not built (needs the reference: make -C oracle/ref_build full)")
    return ctx_harness.HARNESS


@pytest.mark.parametrize("name", list(cs.CASES) + ["big_tables"])
def test_ctx_ref_equals_reference(harness, name):
    c = cs.case(name)
    named = cs.descs(name, reference_only=True)
    assert len(named) == c.V
    arr = desc_array(named)
    descs = [arr[i] for i in range(c.V)]
    H = sum(d.kind == 6 for d in descs)
    assert H == c.H
    data = cs.stream(name)
    assert len(data) == c.n_bytes
    bits = np.unpackbits(data)
    want = ctx_harness.record(data, arr, c.V, cs.positions(name), harness)
    assert want["positions"] == sorted(cs.positions(name)) and want["T"] == len(bits)
    ref = cc.Ref(descs)
    at = 0
    for p, pos in enumerate(want["positions"]):
        got = ref.run(bits[at:pos])
        bad = np.argwhere(got != want["values"][at:pos])
        assert len(bad) == 0, (name, "first differing (bit, variable):", bad[:5] + [at, 0],
                               [named[v][0] for _, v in bad[:5]])
        at = pos
        sec, off = ref.export()
        assert [sec[off[h]:off[h + 1]] for h in range(H)] == want["sections"][p], (name, pos)
        assert sec == b"".join(want["sections"][p]) and off[H] == len(sec), (name, pos)
        assert cc.board_bytes(ref.board()) == want["boards"][p].tobytes(), (name, pos)
    assert at == len(bits)
    if H > 0 and c.n_bytes > cs.RING:
        # the reference itself met a byte opening that stays on one table entry, and wrapped its history ring
        assert want["same_entry"] >= 1 and want["wraps"] >= 1, (name, want["same_entry"], want["wraps"])
    if name == "big_tables":
        # both WriteToDisk branches on tables of more than one chunk, by the reference's own counts
        sizes = [d.table_size for d in descs if d.kind == 6]
        end = want["dense"][-1]
        assert any(d and t > cs.CKPT_CHUNK for d, t in zip(end, sizes))
        assert any(not d and t > cs.CKPT_CHUNK for d, t in zip(end, sizes))
