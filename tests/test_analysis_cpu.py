"""gmix_amd/csrc/gmx_analysis.h off the GPU, against the reference: the host-built header (tests/analysis_common.py's
checker) replays the three cases of tests/golden/analysis_trace.npz, recorded from the reference's own Predictor with
analysis on (tests/golden/make_analysis_golden.py), and every recorded average matches as a uint64 pattern: the stock
Predictor's analysed columns over 1 200 bits of english text, all 123 entropy[] entries over the same run (the layer-0
and layer-1 branches of UpdateEntropy), and UpdateEntropy called directly on chosen operands."""
import numpy as np

import analysis_common as ac


def trace(t):
    f32 = np.float32
    return t["english_pred"].view(f32), t["english_act"], t["english_out"].view(f32), t["english_p"].view(f32), t["english_bits"]


def test_fixture_shape():
    t = ac.fixture()
    assert [str(n) for n in t["names"]] == ["english", "all_columns", "operands"]
    n = len(t["english_bits"])
    assert 8 * 150 <= n <= 8 * 300
    assert t["english_pred"].shape == (n, ac.N_INPUTS) and t["english_out"].shape == (n, ac.N_MIXERS)
    assert t["english_ctx"].shape == (n, ac.N_MIXERS)
    # bits_seen at Perceive is the count of bits before this one
    assert np.array_equal(t["english_seen"], np.arange(n, dtype=np.uint64))
    assert len(t["english_cols"]) == 33 and t["english_cols"][-1] == ac.N_INPUTS + ac.N_MIXERS - 1
    assert list(t["all_columns_cols"]) == list(range(ac.N_INPUTS + ac.N_MIXERS))
    assert list(t["english_kept"][:256]) == list(range(256)) and t["english_kept"][-1] == n - 1
    assert len(t["english_ema"]) == len(t["english_kept"]) and len(t["all_columns_ema"]) == len(t["all_columns_kept"])


def replay(t, case, final_from_p=False):
    pred, act, out, p, bits = trace(t)
    cols = ac.stock_columns(t[case + "_cols"])
    if final_from_p:
        cols[-1] = (ac.FINAL_P, 0)
    v, is_prob = ac.column_values(cols, pred, act, out, p)
    st = ac.Stream(len(cols), is_prob, ema=np.full(len(cols), ac.START), frequency=1)
    trail = st.run(v, bits, trail=True)
    kept = t[case + "_kept"]
    want = t[case + "_ema"]
    got = ac.u64(trail[kept])
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (case, len(bad), bad[:4])
    # F = 1: a row at every bit but the first, labelled bits_seen
    _, seen, rows, labels = st.take()
    assert seen == len(bits) and list(labels) == list(range(1, len(bits)))
    assert np.array_equal(ac.u64(rows), ac.u64(trail[1:]))


def test_english_matches_the_reference():
    replay(ac.fixture(), "english")


def test_all_columns_match_the_reference():
    replay(ac.fixture(), "all_columns")


def test_final_column_from_p_matches_the_reference():
    """The tighter clamp of the wider clamp is the tighter clamp: p instead of the final mixer's output."""
    t = ac.fixture()
    replay(t, "english", final_from_p=True)
    replay(t, "all_columns", final_from_p=True)


def test_operands_match_the_reference():
    t = ac.fixture()
    x, bits = t["operands_x"].view(np.float32), t["operands_bits"]
    L = ac.checker()
    chain = 0.0
    for i in range(len(x)):
        e = L.an_entropy(x[i], int(bits[i]))
        for start, key in ((0.0, "operands_from_zero"), (-1.0, "operands_from_minus_one")):
            got = np.float64(L.an_step(start, e)).view(np.uint64)
            assert got == t[key][i], (key, i, x[i], bits[i])
        chain = L.an_step(chain, e)
        assert np.float64(chain).view(np.uint64) == t["operands_chain"][i], ("chain", i, x[i])
    # ... and as the checker's walk runs the chain
    st = ac.Stream(1)
    trail = st.run(x.reshape(-1, 1), bits, trail=True)
    assert np.array_equal(ac.u64(trail[:, 0]), t["operands_chain"])
