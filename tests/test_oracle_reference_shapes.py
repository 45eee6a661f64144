"""The oracle against the reference's own Mixer (oracle/_ref/ref_mixer_harness) on the shapes every route of
the batched dispatcher takes -- the stock and wide shapes with tables that are not powers of two, moved skip
inputs and learning rates of their own; the 24/8/1 bank at input counts inside and just outside the unrolled
builds' ranges; single mixers -- and on test_gpu_random_topologies' own cases.  The GPU tests of those shapes
compare the kernels with the oracle; this pins the oracle to the reference where no golden fixture does.
Every output, probability, the checkpoint bytes and memory_usage, as bit patterns."""
import pytest

import kernel_shapes as ks

CASES = ks.route_cases()


@pytest.fixture(scope="module")
def harness():
    if not ks.have_reference():
        pytest.skip(f"{ks.HARNESS} not built (needs the reference: make -C oracle/ref_build full)")
    return ks.HARNESS


@pytest.mark.parametrize("cid", list(CASES))
def test_route_shape_oracle_equals_reference(oracle, harness, cid):
    mk, _route, T, seed, kw, nolearn = CASES[cid]
    topo = mk()
    ob, p, outs, _ = ks.oracle_run(oracle, topo, T, seed, kw, nolearn)
    d = ks.reference_run(topo, T, seed, kw, T, nolearn)
    ks.assert_oracle_is_reference(ob, p, outs, d, cid)


@pytest.mark.parametrize("seed", range(16))
def test_random_topology_oracle_equals_reference(oracle, harness, seed):
    """test_gpu_random_topologies' case `seed`, its first stream."""
    topo, T, kw, _ = ks.random_case(seed)
    ob, p, outs, _ = ks.oracle_run(oracle, topo, T, seed * 10 + 1, kw)
    d = ks.reference_run(topo, T, seed * 10 + 1, kw, T)
    ks.assert_oracle_is_reference(ob, p, outs, d, (seed, topo.mixers, topo.skip, kw))

