"""gmix_amd/csrc/gmx_analysis.h off the GPU, against this machine's libm (tests/cpp/analysis_check.cpp builds the header
for the host with strict floats): gmx_log2f equals log2f on every positive normal float -- the clamped domain
[0.01f, 0.99f] of UpdateEntropy among them -- on the subnormals and on the special values;
gmx_analysis_entropy_of_prob equals gmx::BatchedCompressor::AverageOfProb's arithmetic spelled out with libm over the
same clamped domain and around it; gmx_analysis_step is the reference's expression in IEEE doubles.  Exact everywhere."""
import ctypes as C
import math

import numpy as np

import analysis_common as ac

THREADS = 8


def u(x):
    return int(np.float32(x).view(np.uint32))


def sweep(fn, lo, hi):
    first = C.c_uint32(0)
    bad = fn(lo, hi, THREADS, C.byref(first))
    assert bad == 0, (bad, hex(first.value))


def test_log2f_on_every_positive_normal():
    L = ac.checker()
    assert u(0.99) + 1 - u(0.01) == 56203675 and 0x7f800000 - 0x00800000 == 2130706432
    sweep(L.an_sweep_log2f, u(0.01), u(0.99) + 1)          # (first, so that a failure names the domain that matters)
    sweep(L.an_sweep_log2f, 0x00800000, 0x7f800000)


def test_log2f_outside_the_normals():
    L = ac.checker()
    sweep(L.an_sweep_log2f, 0, 0x00800000)                 # +0 and the subnormals
    sweep(L.an_sweep_log2f, 0x7f800000, 0x7f800000 + 4096)  # +inf and NaNs
    sweep(L.an_sweep_log2f, 0x80000000, 0x80000000 + 4096)  # -0 and negative subnormals
    sweep(L.an_sweep_log2f, 0xbf800000 - 64, 0xbf800000 + 64)
    assert L.an_log2f(1.0) == 0.0 and L.an_log2f(0.0) == -math.inf and L.an_log2f(math.inf) == math.inf
    assert math.isnan(L.an_log2f(-1.0)) and math.isnan(L.an_log2f(math.nan))
    assert L.an_log2f(0.25) == -2.0 and L.an_log2f(8.0) == 3.0


def test_entropy_of_prob_equals_the_libm_spelling():
    L = ac.checker()
    sweep(L.an_sweep_prob, u(0.01), u(0.99) + 1)
    sweep(L.an_sweep_prob, u(0.001), u(0.01))              # below the clamp ...
    sweep(L.an_sweep_prob, u(0.99), u(1.0) + 64)           # ... and above it
    sweep(L.an_sweep_prob, 0, 4096)
    sweep(L.an_sweep_prob, 0x7f800000 - 64, 0x7f800000 + 64)
    sweep(L.an_sweep_prob, 0x80000000, 0x80000000 + 4096)
    lo, hi = np.float32(0.01), np.float32(1) - np.float32(0.01)
    assert L.an_entropy_of_prob(0.0, 1) == L.an_log2f(lo) and L.an_entropy_of_prob(0.0, 0) == L.an_log2f(np.float32(1) - lo)
    assert L.an_entropy_of_prob(1.0, 1) == L.an_log2f(hi) and L.an_entropy_of_prob(1.0, 0) == L.an_log2f(np.float32(1) - hi)


def test_entropy_is_entropy_of_prob_of_the_logistic():
    L = ac.checker()
    rng = np.random.default_rng(3)
    for x in np.concatenate([rng.standard_normal(2000).astype(np.float32) * np.float32(6), ac.thresholds(),
                             np.array(ac.SPECIALS, np.float32)]):
        for bit in (0, 1):
            got, want = L.an_entropy(x, bit), L.an_entropy_of_prob(L.an_logistic(x), bit)
            assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32), (x, bit)


def test_thresholds_sit_on_the_clamps():
    L = ac.checker()
    t = ac.thresholds()
    lo, hi = np.float32(0.01), np.float32(1) - np.float32(0.01)
    assert np.nextafter(t[0], np.float32(0)) == t[1] and np.nextafter(t[2], np.float32(9)) == t[3]
    assert L.an_logistic(t[0]) < lo <= L.an_logistic(t[1]) and L.an_logistic(t[2]) <= hi < L.an_logistic(t[3])
    assert abs(float(t[0]) + math.log(99)) < 1e-3 and abs(float(t[3]) - math.log(99)) < 1e-3


def test_step_is_the_reference_expression_in_doubles():
    L = ac.checker()
    rng = np.random.default_rng(4)
    alpha = 0.00001
    for e, x in zip(rng.standard_normal(5000) * 3, rng.standard_normal(5000).astype(np.float32) * np.float32(3)):
        want = (1 - alpha) * float(e) + alpha * float(x)   # (Python floats: IEEE doubles, nothing contracted)
        assert L.an_step(float(e), float(x)) == want
    assert L.an_step(0.0, -1.0) == -alpha and L.an_step(-1.0, 0.0) == -(1 - alpha)


def test_nan_gives_nan():
    L = ac.checker()
    for bit in (0, 1):
        assert math.isnan(L.an_entropy(math.nan, bit)) and math.isnan(L.an_entropy_of_prob(math.nan, bit))
    assert math.isnan(L.an_step(0.5, math.nan)) and math.isnan(L.an_step(math.nan, -1.0))
