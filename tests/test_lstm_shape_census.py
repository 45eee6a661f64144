"""Conditions on the INPUTS of tests/test_gpu_lstm_shape_regimes.py, checked with tests/lstm_shape_ref.c alone: every
row of the case tables in tests/lstm_shape_common.py reaches, on the restatement, the regimes it exists for -- softmax
outputs exactly 0, silent bits, predictions at the logit clamp, elements moved by ClipGradients --, runs the backward
passes and Adam steps it names, and meets no NaN on the way.  The GPU tests repeat these assertions before they look
at a kernel; here they run where no device is."""
import pytest

from oracle import gmxo

import lstm_shape_common as lsc
from test_gpu_lstm_shape import chunks_for, make_streams

_ids = lambda r: str(r["shape"])  # noqa: E731


@pytest.mark.parametrize("row", lsc.CORNER_ROWS, ids=_ids)
def test_corner_and_hot_rows_reach_their_regimes(row):
    cells, horizon = row["shape"][:2]
    assert 1 <= cells <= 256 and 2 <= horizon <= 256
    assert sum(chunks_for(horizon, row["N"])) == row["N"]
    if (horizon, row["N"]) == (256, 513):
        assert chunks_for(horizon, row["N"]) == [255, 257, 1]
    streams = make_streams(gmxo, row["S"], row["N"], seed=row["seed"])
    for s, (r, _, out) in enumerate(lsc.run_refs(row, streams)):
        ev = lsc.regime_evidence(r, out)
        assert ev["backward_passes"] == ev["update_steps"] == row["N"] // horizon >= 2, (row["shape"], s, ev)
        lsc.assert_needs(row, s, ev)


def test_the_pitches_the_corner_rows_exist_for():
    """lin = 257 + cells and hid = cells + 1 exactly fill their 64-float pitches at 63 and 255 cells; cp (cells rounded up
    to 64) is each of 64, 128, 192 and 256; both ends of the horizon range and a learning rate above 0.05 are there."""
    cells = [r["shape"][0] for r in lsc.CORNER_ROWS]
    for c in (63, 255):
        assert c in cells and (257 + c) % 64 == 0 and (c + 1) % 64 == 0
    assert {(c + 63) // 64 * 64 for c in cells} == {64, 128, 192, 256}
    assert max(r["shape"][1] for r in lsc.CORNER_ROWS) == 256 and {1, 256} <= set(cells)
    assert max(r["shape"][2] for r in lsc.CORNER_ROWS) > 0.05 and min(r["shape"][3] for r in lsc.CORNER_ROWS) < 0.05


def test_switch_row_reaches_its_regimes():
    row = lsc.SWITCH_ROW
    H, S = row["shape"][1], row["S"]
    n_sched = sum(n for n, _ in row["schedule"])
    streams = make_streams(gmxo, S, max(row["ragged"]) + n_sched, seed=row["seed"])
    off = [n for n, learn in row["schedule"] if not learn]
    assert off and all(n > H for n in off)              # the stretch without Learn crosses two horizon boundaries
    for s, ev in enumerate(lsc.switch_evidence(row, streams)):
        assert ev["backward_passes"] >= 4, (s, ev)
        lsc.assert_needs(row, s, ev)


@pytest.mark.parametrize("row", lsc.LIMIT_ROWS, ids=_ids)
def test_limit_rows_run_3050_passes_and_stop_counting_at_3000(row):
    (ppm, data), (ppm2, data2) = lsc.limit_inputs(gmxo, row)
    H = row["shape"][1]
    for s, launches in enumerate(lsc.LIMIT_LAUNCHES):
        assert sum(launches) == lsc.LIMIT_BYTES
        assert launches[0] // H == 2000                                   # backward passes inside the first launch
        assert launches[0] < 3000 * H <= launches[0] + launches[1]        # the 3000th falls inside the second
    assert lsc.LIMIT_LAUNCHES[0][0] % H != lsc.LIMIT_LAUNCHES[1][0] % H   # ... at other offsets for the two streams
    for s, (r, _, out) in enumerate(lsc.run_refs(row, [(ppm, data)] * len(lsc.LIMIT_LAUNCHES))):
        ev = lsc.regime_evidence(r, out)
        assert ev["backward_passes"] == row["passes"] and ev["update_steps"] == row["steps"], (s, ev)
        lsc.assert_needs(row, s, ev)
        ev = lsc.regime_evidence(r, r.run(ppm2, data2))
        assert ev["backward_passes"] == row["passes"] + 10 // H and ev["update_steps"] == row["steps"] and ev["nan"] == 0
