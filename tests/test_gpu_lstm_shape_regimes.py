"""The general LSTM kernel (gmx_lstm_any.hip) where its hard branches run and at the corners of the range it is
advertised for: the case tables of tests/lstm_shape_common.py, whose regimes tests/test_lstm_shape_census.py counts on
the CPU.  Every test first recounts on the restatement -- softmax outputs exactly 0 (gmx_expf_tab underflowing),
silent bits (denom == 0 in the bit predictions), predictions at the logit clamp, elements moved by ClipGradients (the
clip bound a run-time value), backward passes and Adam steps -- and only then looks at the kernel.  Then the stock
kernel's own regime fixtures on a stock-shape bank of the general layout.  Tolerance 0 everywhere: floats are compared
as uint32, sections byte for byte."""
import numpy as np
import pytest

import lstm_shape_common as lsc
import test_gpu_lstm_regimes as stock_regimes
from golden.cases import LSTM_REGIMES
from test_gpu_lstm_shape import (assert_stream_equals_ref, build_any, chunks_for, make_streams,  # noqa: F401
                                 run_gpu)                                                       # (build_any: the fixture)

pytestmark = pytest.mark.gpu

_ids = lambda r: str(r["shape"])  # noqa: E731


@pytest.mark.parametrize("row", lsc.CORNER_ROWS, ids=_ids)
def test_corner_and_hot_shapes_equal_restatement(gpu, oracle, row):
    """N bytes in three launches (the first ends inside a horizon, the second on a backward pass): every bit prediction,
    flag and context, the gate weights, the output layer and both export sections."""
    shape, S, N = row["shape"], row["S"], row["N"]
    horizon = shape[1]
    streams = make_streams(oracle, S, N, seed=row["seed"])
    refs = lsc.run_refs(row, streams)
    for s, (r, _, out) in enumerate(refs):
        ev = lsc.regime_evidence(r, out)
        assert ev["backward_passes"] == ev["update_steps"] == N // horizon >= 2, (shape, s, ev)
        lsc.assert_needs(row, s, ev)
    g = gpu.LstmGroup(S, shape=shape)
    assert tuple(g.shape[:2]) == shape[:2] and g.shape[2] == np.float32(shape[2]) and g.shape[3] == np.float32(shape[3])
    for s in range(S):
        g.set_weights(refs[s][1], stream=s)
    assert g.memory_usage() == refs[0][0].memory_usage()
    P, A, Cx = run_gpu(gpu, g, streams, chunks_for(horizon, N))
    assert g.any_launches == 3
    for s, (r, _, out) in enumerate(refs):
        assert_stream_equals_ref(g, s, r, (P[s], A[s], Cx[s]), out, shape)
    g.close()


def test_hot_shape_ragged_generation_and_learn_switch(gpu, oracle):
    """(63, 4, 8.0, 0.5): one ragged launch of 0, 3 and 9 bytes, then 14 bytes with Learn, 7 without (Predict alone takes
    epoch_ across two horizon boundaries) and 20 with it again; after every launch each stream equals its restatement."""
    row = lsc.SWITCH_ROW
    shape, S, lens = row["shape"], row["S"], row["ragged"]
    streams = make_streams(oracle, S, max(lens) + sum(n for n, _ in row["schedule"]), seed=row["seed"])
    for s, ev in enumerate(lsc.switch_evidence(row, streams)):
        assert ev["backward_passes"] >= 4, (s, ev)
        lsc.assert_needs(row, s, ev)
    refs = [lsc.Ref(shape, seed=row["wseed"] + s) for s in range(S)]
    g = gpu.LstmGroup(S, shape=shape)
    for s in range(S):
        g.set_weights(refs[s].weights(), stream=s)
    b = gpu.LstmBatch(g, max(max(lens), max(n for n, _ in row["schedule"])))
    pos = [0] * S

    def step(ns, learn, where):
        for s, (ppm, data) in enumerate(streams):
            b.ppm[s, :ns[s]], b.bytes[s, :ns[s]] = ppm[pos[s]:pos[s] + ns[s]], data[pos[s]:pos[s] + ns[s]]
        b.upload(max(ns))
        if len(set(ns)) > 1:
            g.run_ragged(b, ns, learn=learn)
        else:
            g.run(b, ns[0], learn=learn)
        b.download(max(ns))
        b.wait()
        for s, (ppm, data) in enumerate(streams):
            n = ns[s]
            want = refs[s].run(ppm[pos[s]:pos[s] + n], data[pos[s]:pos[s] + n], learn=learn)
            assert_stream_equals_ref(g, s, refs[s], (b.predictions[s, :n], b.active[s, :n], b.contexts[s, :n]), want, where)
            pos[s] += n

    step(lens, True, "ragged")
    for n, learn in row["schedule"]:
        step([n] * S, learn, ("learn on" if learn else "learn off", n))
    assert g.any_launches == 1 + len(row["schedule"])
    b.close()
    g.close()


@pytest.mark.parametrize("row", lsc.LIMIT_ROWS, ids=_ids)
def test_many_passes_in_a_launch_and_the_update_limit(gpu, oracle, row):
    """6101 bytes at horizon 2: 2000 backward passes inside the first launch (2000 rows of its Adam table in use), the
    3000th -- where update_steps stops counting and Adam's scalars stay put -- inside the second; the second stream's
    launches are one byte off the first's.  Then both streams through export and import into a fresh group (the host's
    mirror of the step count restored at the limit) and 10 more learned bytes."""
    shape, S = row["shape"], len(lsc.LIMIT_LAUNCHES)
    (ppm, data), (ppm2, data2) = lsc.limit_inputs(oracle, row)
    refs = lsc.run_refs(row, [(ppm, data)] * S)
    for s, (r, _, out) in enumerate(refs):
        ev = lsc.regime_evidence(r, out)
        assert ev["backward_passes"] == row["passes"] == 3050 and ev["update_steps"] == row["steps"] == 3000, (s, ev)
        lsc.assert_needs(row, s, ev)
    g = gpu.LstmGroup(S, shape=shape)
    for s in range(S):
        g.set_weights(refs[s][1], stream=s)
    N = lsc.LIMIT_BYTES
    b = gpu.LstmBatch(g, max(max(launches) for launches in lsc.LIMIT_LAUNCHES))
    P, A, Cx = np.zeros((S, N, 8), np.float32), np.zeros((S, N, 8), np.uint8), np.zeros((S, N), np.uint32)
    pos = [0] * S
    for k in range(len(lsc.LIMIT_LAUNCHES[0])):
        ns = [lsc.LIMIT_LAUNCHES[s][k] for s in range(S)]
        for s in range(S):
            b.ppm[s, :ns[s]], b.bytes[s, :ns[s]] = ppm[pos[s]:pos[s] + ns[s]], data[pos[s]:pos[s] + ns[s]]
        b.upload(max(ns))
        g.run_ragged(b, ns)
        b.download(max(ns))
        b.wait()
        for s in range(S):
            P[s, pos[s]:pos[s] + ns[s]] = b.predictions[s, :ns[s]]
            A[s, pos[s]:pos[s] + ns[s]] = b.active[s, :ns[s]]
            Cx[s, pos[s]:pos[s] + ns[s]] = b.contexts[s, :ns[s]]
            pos[s] += ns[s]
    assert pos == [N] * S and g.any_launches == 3
    for s, (r, _, out) in enumerate(refs):
        assert_stream_equals_ref(g, s, r, (P[s], A[s], Cx[s]), out, (shape, "at the limit"))   # (.short carries update_steps)
    b.close()
    saved = [g.export(s) for s in range(S)]
    g.close()
    g2 = gpu.LstmGroup(S, shape=shape)
    for s in range(S):
        g2.import_(*saved[s], stream=s)
        assert g2.export(s) == saved[s], s
    P, A, Cx = run_gpu(gpu, g2, [(ppm2, data2)] * S, [len(data2)])
    for s, (r, _, _) in enumerate(refs):
        want = r.run(ppm2, data2)
        assert r.backward_passes() == row["passes"] + len(data2) // shape[1] and r.update_steps() == row["steps"]
        assert_stream_equals_ref(g2, s, r, (P[s], A[s], Cx[s]), want, (shape, "after import"))
    g2.close()


@pytest.mark.parametrize("name", lsc.ANY_FIXTURES)
def test_stock_fixtures_in_chunks_on_the_general_kernel(gpu, oracle, name, build_any):
    """The body of test_gpu_lstm_regimes.py's test_lstm_kernel_in_hard_regimes on a stock-shape bank of the general
    layout: the state files imported, launches of 120 bytes, against the oracle, the reference's dumped bytes, its
    checksum and its file hashes.  (lstm_short is no regime: the reference's three-pass run from the untouched model.)"""
    if name in LSTM_REGIMES:
        stock_regimes._assert_regime_reached(oracle, name)
    launches, counted = stock_regimes.replay_fixture_in_chunks(gpu, oracle, name)
    assert counted == launches == 3


def test_saturated_fixture_per_byte_on_the_general_kernel(gpu, oracle, build_any):
    """lstm_saturated through gmx_lstm_forward / gmx_lstm_perceive on such a bank: every call one launch of the general
    kernel with a single phase, the exact zeros of the distributions against the oracle's."""
    stock_regimes._assert_regime_reached(oracle, "lstm_saturated")
    calls, counted = stock_regimes.replay_saturated_per_byte(gpu, oracle, sessions=False)
    assert counted == calls
