"""gmx_ctx_forward / gmx_ctx_learn: the context variables one bit at a time on the launch path (gmx_ctx_bit_kernel
around gmx_ctx_step.h).  Expected values: tests/helpers/ctx_ref.c.  Tolerance 0: uint32 patterns and == on exported
bytes.  Every case asserts on ctx_ref.c alone, before it looks at the device, that its bits reach what it is there for."""
import numpy as np
import pytest

import ctx_common as cc
import ctx_shapes
from gmix_amd import GmxError
from test_gpu_chainstep_ctx import assert_ctx_state, same_entry_openings, tiny

pytestmark = pytest.mark.gpu

GMX_ERR_INVALID, GMX_ERR_STATE = -1, -5
_refs = {}


def reference(name, descs, bits):
    """ctx_ref.c over `bits`: (values [T][V], the Ref behind the last bit); shared between the cases, never modified."""
    key = (name, len(bits), bits[:64].tobytes(), int(bits.sum()))
    if key not in _refs:
        ref = cc.Ref(descs)
        _refs[key] = (ref.run(bits), ref)
    return _refs[key]


def per_bit(cg, s, bits, vals, bc_var, t0, t1):
    for t in range(t0, t1):
        got, bc = cg.forward(s)
        assert np.array_equal(got, vals[t]), (s, t, np.flatnonzero(got != vals[t]))
        assert bc == vals[t][bc_var], (s, t)
        cg.learn(int(bits[t]), s)


@pytest.mark.parametrize("S", [1, 3])
def test_every_kind_bit_by_bit(gpu, S):
    """ctx_tiny (17 variables of every kind, hash tables of 1, 3, 7 and 100 entries): 2 000 bits per stream from bytes
    3 / 61 / 500, streams taking turns bit by bit; the values at every bit, the sections and the board at the end.
    (From byte 3 a single stream has a same-entry opening in every table of more than one entry.)"""
    f = tiny()
    T, offsets = 2000, [3, 61, 500][:S]
    bc_var = f.names.index("bit_context")
    bits = [f.bits[8 * o:8 * o + T] for o in offsets]
    same = np.sum([same_entry_openings(f, b) for b in bits], axis=0)
    sizes = [f.descs[v].table_size for v in f.hash_vars]
    assert all(n >= 1 for n, size in zip(same, sizes) if size > 1), (same, sizes)
    refs = [reference("ctx_tiny", f.descs, b) for b in bits]
    assert cc.Ref(f.descs).board().first_prediction == 1              # bit 0 is a first-Predict opening
    cg = gpu.CtxGroup(f.descs, S)
    for t in range(T):
        for s in range(S):
            got, bc = cg.forward(s)
            assert np.array_equal(got, refs[s][0][t]), (s, t, np.flatnonzero(got != refs[s][0][t]))
            assert bc == refs[s][0][t][bc_var], (s, t)
            cg.learn(int(bits[s][t]), s)
    assert_ctx_state(cg, [r[1] for r in refs])
    cg.close()


def test_hand_over_run_per_bit_run(gpu):
    """gmx_ctx_run over 1 001 bytes + 5 bits (the ring of 1 000 has wrapped), 300 bits through forward / learn from
    inside that byte, gmx_ctx_run again to the end: one stream, values everywhere, sections and board at the end."""
    f = tiny()
    T0, T1, T2 = 8 * 1001 + 5, 8 * 1001 + 305, 8 * 1100
    bits = f.bits[:T2]
    assert len(bits) == T2
    vals, ref = reference("ctx_tiny", f.descs, bits)
    bc_var = f.names.index("bit_context")
    assert vals[T0][bc_var] != 0 and vals[T1][bc_var] != 0           # both hand-overs fall inside a byte
    cg = gpu.CtxGroup(f.descs, 1)
    b = gpu.CtxBatch(cg, T0)
    b.bits[0] = bits[:T0]
    b.upload()
    cg.run(b)
    b.download()
    b.wait()
    assert np.array_equal(b.values[0], vals[:T0])
    assert cg.blackboard(0).rotating_history_pos == 1001 % 1000
    per_bit(cg, 0, bits, vals, bc_var, T0, T1)
    n = T2 - T1
    b.bits[0, :n] = bits[T1:]
    b.upload(n)
    cg.run(b, n)                                                      # (the noted learn of bit T1 - 1 is run first)
    b.download(n)
    b.wait()
    assert np.array_equal(b.values[0, :n], vals[T1:])
    assert_ctx_state(cg, [ref])
    b.close()
    cg.close()


def test_64_variables_16_hash_tables(gpu):
    """ctx_shapes' v64_h16 list: every lane of the block holds a variable, sixteen of them a hash table.  Two streams,
    1 200 bits each."""
    name = ctx_shapes.LONG_RUN_CASE
    named = ctx_shapes.descs(name)
    kinds = [k for _, k, _ in named]
    assert (len(named), kinds.count("indirect_hash")) == (64, 16)
    descs = ctx_shapes.as_descs(named)
    data = np.unpackbits(ctx_shapes.stream(name))
    T, S = 1200, 2
    bits = [data[8 * o:8 * o + T] for o in ctx_shapes.offsets(S)]
    refs = [reference(name, descs, b) for b in bits]
    bc_var = kinds.index("bit_context")
    moved = [v for v in range(64) if len(np.unique(refs[0][0][:, v])) > 1]
    # the variables move at all (a hash variable of a large, nearly empty table may keep hashing a fresh entry)
    assert len(moved) >= 48 and sum(kinds[v] == "indirect_hash" for v in moved) >= 10, moved
    cg = gpu.CtxGroup(descs, S)
    for t in range(T):
        for s in range(S):
            per_bit(cg, s, bits[s], refs[s][0], bc_var, t, t + 1)
    assert_ctx_state(cg, [r[1] for r in refs])
    cg.close()


def test_refusals_and_the_noted_learn(gpu, oracle):
    f = tiny()
    bits = f.bits[:64]
    vals, _ = reference("ctx_tiny", f.descs, bits)
    cg = gpu.CtxGroup(f.descs, 2)

    def refused(code, fn):
        with pytest.raises(GmxError) as e:
            fn()
        assert e.value.status == code, e.value

    refused(GMX_ERR_INVALID, lambda: cg.forward(2))
    refused(GMX_ERR_INVALID, lambda: cg.learn(2, 0))
    refused(GMX_ERR_INVALID, lambda: cg.learn(0, -1))
    got, _ = cg.forward(0)
    assert np.array_equal(got, vals[0])
    refused(GMX_ERR_STATE, lambda: cg.forward(0))                      # a second forward without a learn
    # between a forward and its learn: the rules of the lock step for the other surfaces
    refused(GMX_ERR_STATE, lambda: cg.blackboard(0))
    b = gpu.CtxBatch(cg, 8)
    b.bits[:] = 0
    b.upload()
    refused(GMX_ERR_STATE, lambda: cg.run(b))
    refused(GMX_ERR_STATE, lambda: cg.copy_from(cg, 0, 1))
    cg.run_ragged(b, [0, 8])                                           # (stream 0 sits the launch out: allowed)
    cg.learn(int(bits[0]), 0)
    # a noted learn is run before the board is read: new_bit is the learned bit
    ref = cc.Ref(f.descs)
    ref.run(bits[:1])
    assert cc.board_bytes(cg.blackboard(0)) == cc.board_bytes(ref.board())
    # the learn is a Perceive as well: the newest bit told wins
    got, _ = cg.forward(0)
    assert np.array_equal(got, vals[1])
    cg.learn(1 - int(bits[1]), 0)
    cg.learn(int(bits[1]), 0)
    got, _ = cg.forward(0)
    assert np.array_equal(got, vals[2])
    cg.learn(int(bits[2]), 0)
    # a bank attached to a gmx_chainstep refuses both calls
    import test_gpu_chainstep_ctx as tc
    mg = gpu.MixerGroup(tc.TOPO, 2)
    cs = gpu.ChainStep(mg)
    cs.attach_ctx(cg, tc.MIXER_ROUTE)
    refused(GMX_ERR_STATE, lambda: cg.forward(1))
    refused(GMX_ERR_STATE, lambda: cg.learn(0, 1))
    cs.close()
    mg.close()
    b.close()
    cg.close()
