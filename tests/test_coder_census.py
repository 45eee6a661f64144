"""The operands tests/test_gpu_coder_device.py sends through the device's decoder and range walk, off the GPU: the Python
restatement they are judged by (decoder_common.PyDecoder) replays the reference's recorded trace, and the constructed
operands do contain the cases they are built for -- counted with PyDecoder / PyWalk alone, the code under test is not
consulted."""
import os

import numpy as np

import decoder_common as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


def test_pydecoder_replays_the_reference_trace():
    """Every bit and every x1_, x2_, x_ of decoder_trace.npz (trace_tuples asserts them), and the tuples made of it are
    self-consistent: one PyDecoder per tuple answers what the running one did."""
    tup, exp = dc.trace_tuples(np.load(os.path.join(GOLDEN, "decoder_trace.npz")))
    n_bits = 1600 + 1800 + 160
    assert len(tup) >= n_bits + 1000                                    # the trace's bits, and x on xmid / xmid + 1
    assert np.array_equal(dc.decode_expected(tup), exp)
    c = dc.decode_census(tup)
    assert c["x_is_xmid"] >= 100 and c["x_is_xmid_plus_1"] >= 100, c
    assert (exp[:, 4] <= tup[:, 5]).all()                               # `consumed` never passes the input's end ...
    assert c["reads_past_end"] >= 10                                    # ... which the trace's shifts do


def test_discretize_ends():
    for pr in dc.EDGE_PR:
        lo, hi = dc.p_ends(pr)
        assert lo < hi and int(dc.discretize(dc.u2f(lo))) == pr == int(dc.discretize(dc.u2f(hi)))
        assert int(dc.discretize(dc.u2f(lo - 1))) == pr - 1 and int(dc.discretize(dc.u2f(hi + 1))) == pr + 1
    assert int(dc.discretize(F32(0.0001))) == 7 and int(dc.discretize(F32(0.9999))) == 65528
    assert int(dc.discretize(F32(0.5))) == 32768


def test_census_of_the_constructed_decode_tuples():
    t = dc.edge_tuples()
    assert (t[:, 0] <= t[:, 2]).all() and (t[:, 2] <= t[:, 1]).all() and (t[:, 5] <= 4).all()
    assert set((t[:, 1].astype(np.int64) - t[:, 0]).tolist()) == set(dc.EDGE_RANGES)
    assert set(dc.discretize(t[:, 3].view(F32)).tolist()) >= set(dc.EDGE_PR)
    c = dc.decode_census(t)
    print(len(t), c)
    for n_shifts in range(5):
        assert c["shifts"][n_shifts] >= 100, (n_shifts, c)
    for what in ("x_is_xmid", "x_is_xmid_plus_1", "narrow", "reads_past_end"):
        assert c[what] >= 100, (what, c)


def test_census_of_the_walk_distributions():
    """At least one silent range (denom == 0), one p == 0.5, one p at each of Logit's clamps (below 0.0001, above
    0.9999), one subnormal denom, one subnormal quotient; every range that eight bits can reach."""
    pairs = dc.walk_pairs()
    assert (255, 0) in pairs and (1, 0) in pairs and (255, 254) in pairs and all(0 <= b < t <= 255 for t, b in pairs)
    dists = dc.walk_distributions()
    assert len(dists) >= 200
    flt_min = np.uint32(0x00800000).view(F32)
    c = dict(silent=0, half=0, clamp_low=0, clamp_high=0, subnormal_denom=0, subnormal_p=0, near_half=0)
    for _, ppm in dists:
        assert ppm.dtype == F32 and ppm.shape == (256,) and (ppm >= 0).all()
        for num, denom, p in dc.walk_expected(ppm)[1]:
            c["silent"] += p is None
            if p is None:
                continue
            c["half"] += p == F32(0.5)
            c["clamp_low"] += float(p) < 0.0001
            c["clamp_high"] += float(p) > 0.9999
            c["subnormal_denom"] += 0 < denom < flt_min
            c["subnormal_p"] += 0 < p < flt_min
            c["near_half"] += p != F32(0.5) and abs(int(p.view(np.uint32)) - 0x3F000000) <= 2
    print(c)
    assert all(v >= 1 for v in c.values()), c
