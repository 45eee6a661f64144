"""tests/lstm_shape_ref.c -- the LSTM byte model at any shape, what the shaped device banks are compared with -- pinned
on the CPU: to oracle.LstmModel at the stock shape, and to the reference's own Lstm class at six shapes, two of them in the hard regimes, through
tests/golden/lstm_shapes.npz (tests/golden/make_lstm_shape_golden.py).  Tolerance 0: floats are compared as uint32."""
import numpy as np
import pytest

from oracle import gmxo

import lstm_shape_common as lsc
from lstm_shape_common import u32

SEED = 0xDEADBEEF


def test_restatement_equals_oracle_at_the_stock_shape():
    """250 bytes with learn on (two backward passes), then 40 with learn off: probabilities, bit predictions, active
    flags, lstm_prediction_context, gate weights, output layer and both exports."""
    ppm, data = gmxo.lstm_synth(290, seed=21, mask=255, family=0)
    o = gmxo.LstmModel(SEED)
    r = lsc.Ref(lsc.STOCK, seed=SEED)
    assert np.array_equal(u32(r.weights()), u32(o.weights()))       # the same draw
    for a, b, learn in ((0, 250, True), (250, 290, False)):
        pred, act, ctx = o.run(ppm[a:b], data[a:b], learn=learn)
        got = r.run(ppm[a:b], data[a:b], learn=learn)
        assert np.array_equal(u32(got["pred"]), u32(pred)), (a, "bit predictions")
        assert np.array_equal(got["act"], act), (a, "active flags")
        assert np.array_equal(got["ctx"], ctx), (a, "contexts")
        if a == 0:                                                  # the distributions: a second oracle, byte by byte
            ob = gmxo.LstmModel(SEED)
            last = 0
            for n in range(a, b):
                probs, c = ob.predict_byte(ppm[n], last)
                assert np.array_equal(u32(probs), u32(got["probs"][n])), (n, "probs")
                assert c == got["ctx"][n]
                ob.perceive_byte(data[n])
                last = int(data[n])
        assert np.array_equal(u32(r.weights()), u32(o.weights())), (a, "gate weights")
        assert np.array_equal(u32(r.output_layer()), u32(o.output_layer())), (a, "output layer")
        assert r.export_long() == o.export_long(), (a, ".long")
        assert r.export_short() == o.export_short(), (a, ".short")
    assert r.backward_passes() == 2


def test_learning_switched_off_and_on_again_equals_oracle_at_the_stock_shape():
    """Learn on for 130 bytes, off for 210 (Predict alone takes epoch_ across the wraps at bytes 200 and 300: output
    layers no Perceive refreshes, no backward pass), on again for 180: the first Perceive after the gap finds an
    input_history_ and a ring that were filled without it, and the backward pass at byte 400 runs over epochs forwarded
    while Learn was off."""
    ppm, data = gmxo.lstm_synth(520, seed=23, mask=63, family=0)
    o = gmxo.LstmModel(SEED)
    r = lsc.Ref(lsc.STOCK, seed=SEED)
    passes = []
    for a, b, learn in ((0, 130, True), (130, 340, False), (340, 520, True)):
        pred, act, ctx = o.run(ppm[a:b], data[a:b], learn=learn)
        got = r.run(ppm[a:b], data[a:b], learn=learn)
        assert np.array_equal(u32(got["pred"]), u32(pred)), (a, "bit predictions")
        assert np.array_equal(got["act"], act), (a, "active flags")
        assert np.array_equal(got["ctx"], ctx), (a, "contexts")
        assert np.array_equal(u32(r.weights()), u32(o.weights())), (a, "gate weights")
        assert np.array_equal(u32(r.output_layer()), u32(o.output_layer())), (a, "output layer")
        assert r.export_long() == o.export_long(), (a, ".long")
        assert r.export_short() == o.export_short(), (a, ".short")
        passes.append(r.backward_passes())
    assert passes == [1, 1, 3] and r.update_steps() == 3


@pytest.mark.parametrize("case", lsc.golden(), ids=lambda c: c["name"])
def test_restatement_equals_the_reference_classes(case):
    """Every byte's distribution bit for bit, and the four hashes of the final state."""
    ppm, data = gmxo.lstm_synth(case["n_bytes"], seed=case["synth_seed"], mask=case["mask"], family=case["family"])
    r = lsc.Ref(case["shape"], seed=case["seed"])
    got = r.run(ppm, data, learn=True)
    assert np.array_equal(u32(got["probs"]), case["probs"])
    assert lsc.sha(r.weights().tobytes()) == case["sha_weights"]
    assert lsc.sha(r.output_layer().tobytes()) == case["sha_output_layer"]
    assert lsc.sha(r.export_long()) == case["sha_long"]
    assert lsc.sha(r.export_short()) == case["sha_short"]
    assert r.clip_counts() == case["clips"]
    assert r.backward_passes() == case["backward_passes"] >= 3


def test_the_low_clip_case_clips():
    """gradient_clip 0.05 binds in state_error_ and in stored_error_.  The third ClipGradients call sees hidden_error
    right after LstmLayer::BackwardPass has zeroed it, and only a layer above the first adds to it in between: in the
    one-layer model its counter cannot be anything but 0, for any seed."""
    (case,) = [c for c in lsc.golden() if c["shape"] == (65, 7, float(np.float32(0.01)), float(np.float32(0.05)))]
    assert case["clips"][0] >= 1 and case["clips"][1] >= 1
    for c in lsc.golden():
        assert c["clips"][2] == 0
        assert c["backward_passes"] >= 3
