"""tests/helpers/match_ref.c against what the reference itself recorded (tests/golden/match_*.npz): every slot
value (as the per-bit hash of their bit patterns), active flag and longest_match of every bit, both checkpoint
sections byte for byte, GetMemoryUsage; and a run split by the restatement's own export / import.  CPU only."""
import numpy as np
import pytest

import match_common as mc


@pytest.mark.parametrize("name", mc.FIXTURES)
def test_fixture_covers_the_hard_cases(name):
    f = mc.fixture(name)
    for key, least in mc.NEED.items():
        assert (name, key) in mc.EXEMPT or f.meta[key] >= least, (key, f.meta[key])
    if name in ("match_stock", "match_tiny"):
        assert f.meta["max_count"] == f.limit
    assert len(f.data) >= 6000


def test_both_checkpoint_branches_across_the_set():
    dense = sum((mc.fixture(n).dense for n in mc.FIXTURES), [])
    assert 0 in dense and 1 in dense


def test_stock_stream_shape():
    d = mc.fixture("match_stock").data
    runs = np.diff(np.flatnonzero(np.concatenate(([1], np.diff(d) != 0, [1]))))
    assert runs.max() >= 600 and len(d) >= 12000


@pytest.mark.parametrize("name", mc.FIXTURES)
def test_replay(name):
    f = mc.fixture(name)
    r = mc.Ref(f.models())
    slots, act, lm = r.run(f.ctx, f.bc, f.bits)
    bad = np.flatnonzero(mc.slot_hash(slots) != f.slot_hash)
    assert bad.size == 0, f"slot values differ first at bit {bad[0]}"
    assert (act == f.act).all()
    assert (lm == f.lm).all()
    lb, sb = r.export()
    assert lb == f.long
    assert sb == f.short
    assert [r.memory_usage(k) for k in range(f.K)] == f.usage


@pytest.mark.parametrize("name,cut", [("match_stock", 40003), ("match_tiny", 20001), ("match_k8", 8 * 2500)])
def test_split_run_through_own_checkpoint(name, cut):
    f = mc.fixture(name)
    a = mc.Ref(f.models())
    s0, a0, l0 = a.run(f.ctx[:cut], f.bc[:cut], f.bits[:cut])
    lb, sb = a.export()
    b = mc.Ref(f.models())
    b.import_(lb, sb)
    b.set_slots(*a.slots())  # ShortTermMemory's share: the blackboard slots and new_bit
    s1, a1, l1 = b.run(f.ctx[cut:], f.bc[cut:], f.bits[cut:])
    assert (mc.slot_hash(np.concatenate([s0, s1])) == f.slot_hash).all()
    assert (np.concatenate([a0, a1]) == f.act).all()
    assert (np.concatenate([l0, l1]) == f.lm).all()
    assert b.export() == (f.long, f.short)
