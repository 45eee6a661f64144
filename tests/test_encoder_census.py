"""Conditions on the INPUTS of tests/test_gpu_encoder.py, checked with PyEncoder alone: the operand sets hold at least
100 bits of every emit count 0..3 and at least 20 of 4 (by chance a bit emits four bytes 29 times in 400 000 of the
mixture: the fours are constructed through reset), and p at both clamps, at 0, at 1 and at 0.5."""
import numpy as np

import encoder_common as ec


def test_mixture_statistics():
    hist = np.zeros(5, np.int64)
    for seed in range(20):
        p, bits = ec.mixture(20000, seed)
        hist += np.bincount(ec.emit_counts(bits, p), minlength=5)
    assert hist.sum() == 400000 and hist[4] < 200 and (hist[:4] > 2000).all(), hist


def test_gpu_operand_sets_hold_every_emit_count_and_every_special_p():
    p, bits, n = ec.gpu_operands()
    assert p.shape == bits.shape == (ec.S, ec.T) and n.shape == (ec.S,)
    assert set(ec.COUNTS) <= set(int(v) for v in n[:64]) and set(int(v) for v in n[64:]) >= {0, 1, 300}
    hist = np.zeros(5, np.int64)
    for s in range(ec.S):
        hist += np.bincount(ec.emit_counts(bits[s], p[s]), minlength=5)
    # the constructed rounds: every stream from KIN[s % 4] once, and from the four-byte state 25 times
    for s in range(ec.S):
        k = int(ec.emit_counts([1], [np.float32(0.5)], ec.KIN[s % 4])[0])
        assert k == s % 4 + 1
        hist[k] += 1
    assert int(ec.emit_counts([1], [np.float32(0.5)], ec.FOUR)[0]) == 4
    hist[4] += 25 * ec.S
    assert (hist[:4] >= 100).all() and hist[4] >= 20, hist
    pv = set(p.view(np.uint32).ravel().tolist())
    for v in (0.0, 1.0, 0.5, ec.LO, ec.HI):
        assert int(np.float32(v).view(np.uint32)) in pv, v
