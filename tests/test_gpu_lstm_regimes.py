"""The LSTM kernel where its hard branches run, and where its launcher chooses for itself.

The fixtures lstm_saturated / lstm_onehot / lstm_clipped (tests/golden/cases.py) were made from the REAL reference
LstmModel, started from a state file through its own ReadFromDisk; tests/test_oracle_lstm.py pins the oracle to them.
Here the HIP kernel replays them -- every instantiation of the batched kernel, and the per-byte session -- and is
compared bit for bit with both: silent bits, exact-zero softmax outputs, clamped logits, saturated gates and the
gradient clip at +-10 all run, which the oracle's own counts show before a kernel is looked at.  Then two launches
that leave GMX_LSTM_BUILD alone: one workgroup per CU at exactly the CU count, two per CU above it."""
import ctypes as C
import functools
import subprocess
import sys

import numpy as np
import pytest

import goldenlib
from golden.cases import LSTM_CASES, LSTM_REGIMES
from test_gpu_lstm import lstm_build, run_gpu, u32  # noqa: F401  (lstm_build: the fixture)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _evidence(name):
    from oracle import gmxo
    return goldenlib.lstm_regime_evidence(gmxo, LSTM_CASES[name][2], LSTM_REGIMES[name]["bytes"])[0]


@functools.lru_cache(maxsize=None)
def _cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process: torch brings a HIP
    runtime of its own, which finds no device in a process where libgmxmix.so's has already opened it."""
    out = subprocess.check_output([sys.executable, "-c", "import torch; "
                                   "print(torch.cuda.get_device_properties(0).multi_processor_count)"], timeout=120)
    return int(out.split()[-1])


def _assert_regime_reached(oracle, name):
    """From the oracle alone: the branches the regime exists for ran, as often as recorded beside the case."""
    reg = LSTM_REGIMES[name]
    ev = _evidence(name)
    for k in reg["needs"]:
        assert ev[k] > 0, (name, k, ev)
    if reg["counts"] is not None:
        assert ev == reg["counts"], name
    if "input_counts" in reg:
        assert goldenlib.lstm_input_evidence(oracle, LSTM_CASES[name][2], LSTM_CASES[name][0]) == reg["input_counts"]


def _start(gpu, oracle, kw, n_streams=1):
    """(oracle model, device group) at the fixture's starting state: the state files imported, or the weights set."""
    m, files = goldenlib.lstm_start_model(oracle, kw)
    g = gpu.LstmGroup(n_streams)
    for s in range(n_streams):
        if files:
            g.import_(*files, stream=s)
        else:
            g.set_weights(m.weights(), stream=s)
    return m, g


def _harness_checksum(oracle, P, A, Cx):
    """ref_lstm_harness's running FNV: per bit (prediction, active), per byte the context after bit 0."""
    N = len(Cx)
    rec = np.zeros((N, 8 * 5 + 4), np.uint8)
    for k in range(8):
        off = 5 * k + (4 if k > 0 else 0)
        rec[:, off:off + 4] = P[:, k].copy().view(np.uint8).reshape(N, 4)
        rec[:, off + 4] = A[:, k]
        if k == 0:
            rec[:, 5:9] = Cx.copy().view(np.uint8).reshape(N, 4)
    return oracle.fnv64_bytes(rec.reshape(-1))


def replay_fixture_in_chunks(gpu, oracle, name):
    """A fixture of tests/golden/cases.py from its starting state through the batched kernel in launches of 120 bytes,
    against the oracle and against the reference's own run.  The bank is created HERE: under GMX_LSTM_BUILD=any
    (tests/test_gpu_lstm_shape_regimes.py) it has the general layout and kernel.  Returns (launches, what
    gmx_debug_lstm_any_launches counted)."""
    meta, z = goldenlib.load(name)
    kw, N, D = meta["synth"], meta["bytes"], meta["dump"]
    ppm, data = oracle.lstm_synth(N, seed=kw.get("seed", 0), mask=kw.get("mask", 255), family=kw.get("family", 0))
    m, g = _start(gpu, oracle, kw)
    assert m.weights_hash() == meta["init_weights_hash"]
    pred, act, ctx = m.run(ppm, data)
    P, A, Cx = run_gpu(gpu, g, [(ppm, data)], chunk=120)      # launches that split the epochs: 120 + 120 + 90
    # against the oracle: every bit
    bad = np.argwhere(u32(P[0]) != u32(pred))
    assert len(bad) == 0, (len(bad), bad[:4], P[0][tuple(bad[0])], pred[tuple(bad[0])])
    assert np.array_equal(A[0], act) and np.array_equal(Cx[0], ctx)
    w, o = g.get_weights(0)
    assert np.array_equal(u32(w), u32(m.weights())) and np.array_equal(u32(o), u32(m.output_layer()))
    lng, sh = g.export(0)
    assert lng == m.export_long() and sh == m.export_short()
    # against the reference's own run: the dumped bytes, the checksum over all of them, its files at the end
    assert np.array_equal(u32(P[0, :D]), z["pred"]) and np.array_equal(A[0, :D], z["active"])
    assert np.array_equal(Cx[0, :D], z["ctx"])
    assert _harness_checksum(oracle, P[0], A[0], Cx[0]) == meta["h64"]
    assert len(sh) == meta["short_size"] and oracle.fnv64_bytes(sh) == meta["short_hash"]
    assert oracle.fnv64_bytes(lng) == meta["long_hash"]
    counted = g.any_launches
    g.close()
    return (N + 119) // 120, counted


@pytest.mark.parametrize("name", sorted(LSTM_REGIMES))
def test_lstm_kernel_in_hard_regimes(gpu, oracle, name, lstm_build):
    _assert_regime_reached(oracle, name)
    replay_fixture_in_chunks(gpu, oracle, name)


def replay_saturated_per_byte(gpu, oracle, sessions):
    """lstm_saturated one byte at a time through gmx_lstm_forward / gmx_lstm_perceive; sessions: through the persistent
    session, else as the bank itself decides (a bank of the general layout launches its kernel at every call).  Returns
    (calls, what gmx_debug_lstm_any_launches counted)."""
    name = "lstm_saturated"
    meta, z = goldenlib.load(name)
    kw, N = meta["synth"], 230
    ppm, data = oracle.lstm_synth(N, seed=kw.get("seed", 0), mask=kw.get("mask", 255), family=kw.get("family", 0))
    m, g = _start(gpu, oracle, kw)
    if sessions:
        g.L.gmx_debug_lstm_use_sessions.argtypes = [C.c_void_p, C.c_int]
        assert g.L.gmx_debug_lstm_use_sessions(g.h, 1) == 0
    last, zeros = 0, 0
    for n in range(N):
        probs, ctx = g.forward(ppm[n], last)
        p_ref, c_ref = m.predict_byte(ppm[n], last)
        assert np.array_equal(u32(probs), u32(p_ref)) and ctx == c_ref, n
        zeros += int((probs == 0).sum())
        pr, act, _ = m.bits_from_probs(probs, data[n])
        assert np.array_equal(u32(pr), z["pred"][n]) and np.array_equal(act, z["active"][n]) and ctx == z["ctx"][n], n
        g.perceive(int(data[n]))
        m.perceive_byte(int(data[n]))
        last = int(data[n])
    assert zeros > 0
    lng, sh = g.export(0)
    # (where a byte has ended the bank writes the range of its eighth bit; the oracle's byte-level calls never coded
    # the bits, its range is still the forward's: the first 12 bytes)
    assert lng == m.export_long() and sh[12:] == m.export_short()[12:]
    counted = g.any_launches
    g.close()
    return 2 * N, counted


def test_lstm_session_in_saturated_regime(gpu, oracle):
    """lstm_saturated one byte at a time through the persistent session (gmx_lstm_forward / gmx_lstm_perceive: the
    <154, 2, true> instantiation, another launch shape around the same code): the byte distributions with their exact
    zeros against the oracle's, the bits coded from them on the host against the reference's dump, two backward
    passes, the files at the end."""
    _assert_regime_reached(oracle, "lstm_saturated")
    replay_saturated_per_byte(gpu, oracle, sessions=True)


@pytest.mark.parametrize("over", [45, 0], ids=["above_the_cu_count", "at_the_cu_count"])
def test_lstm_launcher_own_build_choice_at_scale(gpu, oracle, over, monkeypatch):
    """No GMX_LSTM_BUILD: the launcher's rule n_streams <= CUs ? one workgroup per CU : two.  CUs + 45 streams (no
    multiple of the CU count or of 64) take the two-per-CU build with more workgroups than CUs, exactly CUs streams the
    last launch the one-per-CU build gets.  230 bytes, two backward passes, every stream its own seed; streams spread
    over the launch -- the first, the last, both sides of the CU boundary, three in between -- against the oracle."""
    monkeypatch.delenv("GMX_LSTM_BUILD", raising=False)
    cus = _cu_count()
    S, N, seed = cus + over, 230, 0x5EED
    assert cus > 64
    try:
        g = gpu.LstmGroup(S)
        b = gpu.LstmBatch(g, N)
    except gpu.GmxError as e:
        pytest.skip("banks of %d LSTM streams cannot be allocated: %s" % (S, e))
    w0 = oracle.LstmModel().weights()
    seeds = [(seed + s * 0x9E3779B97F4A7C15) & ((1 << 64) - 1) for s in range(S)]
    for s in range(S):
        g.set_weights(w0, stream=s)
        b.ppm[s], b.bytes[s] = oracle.lstm_synth(N, seed=seeds[s], mask=63 if s % 3 else 255, family=s % 2)
    b.upload(N)
    g.run(b, N, learn=True)
    b.download(N)
    b.wait()
    sampled = sorted({0, cus // 4, cus // 2, (3 * cus) // 4, cus - 1, min(cus, S - 1), S - 1})
    assert len(sampled) >= 5
    for s in sampled:
        m = oracle.LstmModel()
        pred, act, ctx = m.run(np.array(b.ppm[s]), np.array(b.bytes[s]))
        bad = np.argwhere(u32(b.predictions[s]) != u32(pred))
        assert len(bad) == 0, (s, len(bad), bad[:4])
        assert np.array_equal(b.active[s], act) and np.array_equal(b.contexts[s], ctx), s
        assert g.export(s) == (m.export_long(), m.export_short()), s
    for i, s in enumerate(sampled):
        for t in sampled[i + 1:]:
            assert not np.array_equal(u32(b.predictions[s]), u32(b.predictions[t])), (s, t)
    b.close()
    g.close()
