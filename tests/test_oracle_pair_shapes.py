"""The oracle against the reference's own Mixer (oracle/_ref/ref_mixer_harness) on every shape
tests/test_gpu_pair_kernel.py runs through the register-resident kernel for any three-layer bank: that test
compares the kernel with the oracle, this one pins the oracle to the reference.  Every output, probability, the
checkpoint bytes and memory_usage, as bit patterns."""
import pytest

import kernel_shapes as ks
import pair_shapes

CASES = pair_shapes.cases()


@pytest.fixture(scope="module")
def harness():
    if not ks.have_reference():
        pytest.skip(f"{ks.HARNESS} not built (needs the reference: make -C oracle/ref_build full)")
    return ks.HARNESS


@pytest.mark.parametrize("cid", list(CASES))
def test_pair_shape_oracle_equals_reference(oracle, harness, cid):
    mk, T, seed, kw, nolearn = CASES[cid]
    topo = mk()
    ob, p, outs, _ = ks.oracle_run(oracle, topo, T, seed, kw, nolearn)
    d = ks.reference_run(topo, T, seed, kw, T, nolearn)
    ks.assert_oracle_is_reference(ob, p, outs, d, cid)


def test_scale_shape_oracle_equals_reference(oracle, harness):
    topo = pair_shapes.scale_topology()
    kw = dict(ctx_mode=0)
    ob, p, outs, _ = ks.oracle_run(oracle, topo, 256, 70000, kw)
    d = ks.reference_run(topo, 256, 70000, kw, 256)
    ks.assert_oracle_is_reference(ob, p, outs, d, "scale")
