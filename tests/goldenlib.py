"""Shared helpers for tests that replay tests/golden/ fixtures."""
import hashlib
import json
import os

import numpy as np

from gmix_amd import topology

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, z


def topo_of(meta):
    return topology.Topology(meta["n"], [tuple(m) for m in meta["mixers"]], skip=meta["skip"])


def synth_kwargs(meta):
    kw = dict(meta.get("synth", {}))
    nolearn = kw.pop("nolearn_from", None)
    return kw, nolearn


def sha256(b):
    return hashlib.sha256(b).hexdigest()


def unpack_trace(z, meta):
    T, n = meta["T"], meta["n"]
    pred = z["pred"].view(np.float32)
    act = np.unpackbits(z["act"], axis=1, bitorder="little")[:, :n]
    bits = np.unpackbits(z["bits"], bitorder="little")[:T]
    return pred, act, z["ctx"], bits, z["outs"], z["p"]


def ind_case(name):
    """(meta, models, ctx, bit_context, bits, nolearn_from, z) of an Indirect fixture; the inputs
    are re-derived from the seed (oracle/gmx_ind_synth.h)."""
    from oracle import gmxo
    meta, z = load(name)
    models = [tuple(m) for m in meta["models"]]
    kw = dict(meta["synth"])
    nolearn = kw.pop("nolearn_from", None)
    ctx, bc, bits = gmxo.ind_synth(len(models), meta["T"], seed=kw.get("seed", 0), ctx_mod=kw.get("ctx_mod", (0,) * 4))
    return meta, models, ctx, bc, bits, nolearn, z


# ---- LSTM fixtures that start from a state file (tests/golden/cases.py, LSTM_CASES: the `state` entry) ----------------
_NC, _W, _H, _NO, _NI, _HID, _LIN = 50, 563, 100, 256, 256, 51, 307
_SHORT_GATES = 12 + 4 * (_NO + _H + _HID + _NC + _H * _LIN + _H * _NO + 1 + 3 * _NC + 3 * _H * _NC + 1 + 2)
_SHORT_GATE = 4 * (_NC + _H + 8 * _NC + _H * _NC + 3 * _NC * _W + (_W - _NO - _NI) * _NC + _H * _NC)
_SHORT_GAMMA = 4 * (_NC + _H)       # NeuronLayer::WriteToDisk: error_, ivar_, gamma_, ...


def lstm_start_state(gmxo, spec):
    """(long, short): the files a fixture's run starts from, in the reference's own checkpoint format -- the LSTM
    section of LongTermMemory::WriteToDisk and LstmModel::WriteToDisk.  Made with the oracle alone, so that the
    reference harness (its ReadFromDisk), the oracle and the device bank all start from the same bytes:
    the srand(0xDEADBEEF) model learns spec["warm"] = (bytes, seed, mask) of the smooth input family, the last of them
    byte 0 (a fresh ShortTermMemory's last_byte); then the layer-norm gains of the three gates are multiplied by
    spec["gain"] -- the layer norm undoes any scaling of the gate MATRICES, the gain is what sets the size of the
    pre-activations -- and the whole output-layer ring by spec["out_scale"] (it is all zeros before the model has
    learned, hence the warm-up)."""
    m = gmxo.LstmModel()
    n, seed, mask = spec["warm"]
    ppm, data = gmxo.lstm_synth(n, seed=seed, mask=mask)
    data[-1] = 0
    m.run(ppm, data)
    lng = np.frombuffer(m.export_long(), np.float32).copy()
    sh = np.frombuffer(m.export_short(), np.uint8).copy()
    assert len(sh) == _SHORT_GATES + 3 * _SHORT_GATE
    lng[:_H * _NO * _HID] *= np.float32(spec["out_scale"])
    for g in range(3):
        o = _SHORT_GATES + g * _SHORT_GATE + _SHORT_GAMMA
        gam = sh[o:o + 4 * _NC].view(np.float32)
        gam *= np.float32(spec["gain"])
    return lng.tobytes(), sh.tobytes()


def lstm_start_model(gmxo, kw):
    """The oracle's model at the start of an LSTM fixture (kw = its synth kwargs) and the state files, or None."""
    m = gmxo.LstmModel()
    if "state" not in kw:
        return m, None
    files = lstm_start_state(gmxo, kw["state"])
    m.import_state(*files)
    return m, files


def lstm_regime_evidence(gmxo, kw, n_bytes):
    """What the oracle itself says about a fixture's first n_bytes: how often each hard branch ran.
    silent_bits: bits where the model stayed silent (denom == 0: not active, the previous prediction repeated and not
    the 0 an inactive p == 0.5 stores); zero_probs: softmax outputs that are exactly 0.0f; clamped_logits: predictions
    at +-logit(0.9999f), Sigmoid::Logit's clamp; clipped: gradient elements ClipGradients moved to +-10;
    saturated_gates: input-node pre-activations norm * gamma + beta beyond +-22 (tanhf's saturated branch) among the
    epochs still in the ring when the run ends."""
    m, _ = lstm_start_model(gmxo, kw)
    ppm, data = gmxo.lstm_synth(n_bytes, seed=kw.get("seed", 0), mask=kw.get("mask", 255), family=kw.get("family", 0))
    pred = np.zeros((n_bytes, 8), np.float32)
    act = np.zeros((n_bytes, 8), np.uint8)
    zero_probs, last = 0, 0
    for n in range(n_bytes):
        probs, _ = m.predict_byte(ppm[n], last)
        zero_probs += int((probs == 0.0).sum())
        pred[n], act[n], _ = m.bits_from_probs(probs, data[n])
        m.perceive_byte(int(data[n]))
        last = int(data[n])
    flat, fact = pred.reshape(-1), act.reshape(-1)
    prev = np.concatenate([[np.float32(0)], flat[:-1]])
    silent = int(((fact == 0) & (flat.view(np.uint32) == prev.view(np.uint32)) & (flat != 0)).sum())
    clamp = np.float32(np.log(np.float32(np.float32(0.9999) / (np.float32(1) - np.float32(0.9999)))))
    clamped = int((np.abs(flat) >= clamp).sum())
    sh = np.frombuffer(m.export_short(), np.uint8)
    o = _SHORT_GATES + 1 * _SHORT_GATE                     # the input node (tanh)
    gam = sh[o + _SHORT_GAMMA:o + _SHORT_GAMMA + 4 * _NC].view(np.float32)
    bet = sh[o + _SHORT_GAMMA + 16 * _NC:o + _SHORT_GAMMA + 20 * _NC].view(np.float32)
    no = o + _SHORT_GATE - 4 * _H * _NC
    norm = sh[no:no + 4 * _H * _NC].view(np.float32).reshape(_H, _NC)
    live = norm[:n_bytes % _H] if n_bytes % _H else norm     # epochs forwarded since Adam last moved gamma / beta
    saturated = int((np.abs(live * gam + bet) >= 22).sum())
    return dict(silent_bits=silent, zero_probs=zero_probs, clamped_logits=clamped, clipped=m.clipped(),
                saturated_gates=saturated), (pred, act)


def lstm_input_evidence(gmxo, kw, n_bytes):
    """What the second input family puts before the model: counts of its exact values."""
    ppm, data = gmxo.lstm_synth(n_bytes, seed=kw.get("seed", 0), mask=kw.get("mask", 255), family=kw.get("family", 0))
    return dict(zeros=int((ppm == 0).sum()), ones=int((ppm == 1).sum()),
                uniform_rows=int((ppm == np.float32(1.0 / 256)).all(1).sum()),
                repeats=int((data[1:] == data[:-1]).sum()),
                true_byte_zero=int((ppm[np.arange(n_bytes), data] == 0).sum()))
