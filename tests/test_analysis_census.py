"""What the inputs of the analysis tests hold, checked on tests/golden/analysis_trace.npz alone: in `english` every
analysed column the device produces (everything but PPMd) has silent and active bits and sees both bit values either
way; `operands` holds values on both sides of both clamps, both infinities and both zeros, and the recorded results show
that the clamp took or did not take them."""
import numpy as np

import analysis_common as ac


def test_english_columns_are_silent_and_active_under_both_bits():
    t = ac.fixture()
    cols, names, act, bits = t["english_cols"], [str(n) for n in t["english_names"]], t["english_act"], t["english_bits"]
    assert set(bits.tolist()) == {0, 1}
    inputs = [(int(c), n) for c, n in zip(cols, names) if c < ac.N_INPUTS]
    assert "ppmd" in inputs[0][1].lower() and inputs[1][1] == "LSTM"
    assert len(inputs) == 32 and sum("Indirect(skip" in n for _, n in inputs) == 30
    assert names[-1] == "Mixer(final layer)"
    for c, n in inputs[1:]:                      # PPMd stays on the host
        a = act[:, c] != 0
        assert a.any() and (~a).any(), n
        assert set(bits[a].tolist()) == {0, 1} and set(bits[~a].tolist()) == {0, 1}, n
    # a silent slot of the recorded blackboard is the zero Predict put there
    pred = t["english_pred"].view(np.float32)
    for c, _ in inputs:
        assert not pred[act[:, c] == 0, c].any()
    assert pred[act != 0].any()


def test_operands_hold_the_edges():
    t = ac.fixture()
    x, bits = t["operands_x"].view(np.float32), t["operands_bits"]
    thr = t["operands_thresholds"].view(np.float32)
    assert len(x) >= 2000 + 2 * (len(ac.SPECIALS) + 4)
    have = {(int(v), int(b)) for v, b in zip(t["operands_x"], bits)}
    for v in list(np.array(ac.SPECIALS, np.float32)) + list(thr):
        for b in (0, 1):
            assert (int(np.float32(v).view(np.uint32)), b) in have, (v, b)
    assert thr[0] < thr[1] < 0 < thr[2] < thr[3]
    assert np.nextafter(thr[0], np.float32(0)) == thr[1] and np.nextafter(thr[2], np.float32(9)) == thr[3]
    # the recorded results tell which side of a clamp a value fell on: the step from 0 of a clamped value is that of -100
    # or of 100
    z = {(int(v), int(b)): int(r) for v, b, r in zip(t["operands_x"], bits, t["operands_from_zero"])}

    def key(v, b):
        return int(np.float32(v).view(np.uint32)), b
    for b in (0, 1):
        # (the neighbour inside may land on the clamp value itself: its result cannot tell)
        assert z[key(thr[0], b)] == z[key(-100.0, b)] == z[key(-np.inf, b)] == z[key(-20.0, b)]
        assert z[key(thr[3], b)] == z[key(100.0, b)] == z[key(np.inf, b)] == z[key(20.0, b)]
        assert z[key(0.0, b)] == z[key(-0.0, b)] == int(np.float64(-0.00001).view(np.uint64))   # log2f(0.5) = -1
        inside = (np.abs(x) < np.float32(4.5)) & (bits == b)
        assert inside.sum() > 200
        assert not np.isin(t["operands_from_zero"][inside], [z[key(-100.0, b)], z[key(100.0, b)]]).any()
    big = np.abs(x) > np.float32(4.6)
    assert big.sum() > 200 and (~big).sum() > 200 and set(bits[big].tolist()) == set(bits[~big].tolist()) == {0, 1}
