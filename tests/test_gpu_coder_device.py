"""gmx_coder.h as gfx950 runs it: gmx_coder_decode and gmx_coder_walk_predict on chosen operands, through the device probe
(gmx_debug_math_probe, what = 12 and 13: gmx_aux.hip calls the header's own functions).  The device build is not the
host's: Discretize is spelled with __fmul_rn / __fadd_rn, the quotient's division and gmx_logit are the device's, the
renormalisation loop and the byte reads are device code.  Exact everywhere: integers as integers, floats as bit patterns.
What the operands contain is counted off the GPU (tests/test_coder_census.py)."""
import os

import numpy as np
import pytest

import decoder_common as dc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DECODE_OUT = ("bit", "x1", "x2", "x", "consumed", "pr")


def assert_decodes(got, want, tup):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), [dict(
        x1_x2_x_p_next4_avail=[hex(v) for v in tup[i]],
        device={k: hex(v) for k, v in zip(DECODE_OUT, got[i])},
        expected={k: hex(v) for k, v in zip(DECODE_OUT, want[i])}) for i in bad[:5]])


def test_reference_trace_through_the_device(gpu):
    """Every bit of tests/golden/decoder_trace.npz as a tuple of its own: the state after bit t - 1, p[t] and the next
    four input bytes give the recorded bit and the recorded x1_, x2_, x_ after bit t -- the device build against the
    reference's Decoder directly, not through the host's build of the header.  No recorded x lies on xmid, so every
    bit that shifted nothing comes a second time with x on the boundary its recorded state names (x2_ after a 1, x1_
    after a 0): the recorded bit and range again (decoder_common.trace_tuples)."""
    tup, want = dc.trace_tuples(np.load(os.path.join(GOLDEN, "decoder_trace.npz")))
    assert_decodes(dc.probe_decode(gpu._lib.lib(), tup), want, tup)


def test_constructed_edges(gpu):
    """decoder_common.edge_tuples: pr at both clamps, around 0.5 and at their neighbours, each through the smallest and
    the largest p; ranges from 0 to 2^32 - 1 with the byte boundaries inside and outside; x at and around xmid; an
    input that ends after 0 .. 4 bytes.  Expected: PyDecoder."""
    tup = dc.edge_tuples()
    assert_decodes(dc.probe_decode(gpu._lib.lib(), tup), dc.decode_expected(tup), tup)


@pytest.mark.parametrize("seed", [2025, 2026, 2027, 2028])
def test_random_tuples(gpu, seed):
    """10^6 random tuples with x1 <= x <= x2 (decoder_common.random_tuples), a quarter per case: PyDecoder takes some
    microseconds for each.  Expected: PyDecoder."""
    tup = dc.random_tuples(250_000, seed)
    assert_decodes(dc.probe_decode(gpu._lib.lib(), tup), dc.decode_expected(tup), tup)


def test_range_walk(gpu):
    """All 255 ranges [bot, top] that eight bits can reach, over decoder_common.walk_distributions: wrote / slot /
    active of gmx_coder_walk_predict against PyWalk (float32 sums left to right, float32 division, Logit with libm's
    logf).  A range without mass writes nothing: the probe's sentinels come back."""
    dists = dc.walk_distributions()
    got = dc.probe_walk(gpu._lib.lib(), np.stack([ppm for _, ppm in dists]))
    pairs = dc.walk_pairs()
    bad = []
    for d, (name, ppm) in enumerate(dists):
        want, seen = dc.walk_expected(ppm)
        for i in np.nonzero((got[d] != want).any(axis=1))[0]:
            num, denom, p = seen[i]
            bad.append(dict(distribution=name, top_bot=pairs[i], num=float(num).hex(), denom=float(denom).hex(),
                            p=None if p is None else float(p).hex(), device_wrote_slot_active=[hex(v) for v in got[d][i]],
                            expected=[hex(v) for v in want[i]]))
    assert not bad, (len(bad), bad[:5])
