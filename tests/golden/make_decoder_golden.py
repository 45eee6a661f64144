"""Regenerates tests/golden/decoder_trace.npz from the reference's own Decoder (build container only: it needs the
reference's sources and g++).  ref_decoder_harness.cpp is compiled against coder/decoder.cpp where it lies, into a
temporary directory, with a stub Predictor that returns the seeded probabilities below; the fixture holds the inputs
and x1_, x2_, x_ and the bit after every Decode, nothing of the reference's program text.

    python tests/golden/make_decoder_golden.py [--ref /path/to/reference]

Three inputs: an encoded payload (oracle.encode of seeded bits under the same p, so the decoded bits are known twice),
64 random bytes (decoded until well past their end), and a 3-byte input (the four start bytes already read past its
end).  The p of every case hold both clamps of Predictor::Predict (1e-4f and 1 - 1e-4f) and 0.5.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import gmxo  # noqa: E402

EPS = np.float32(0.0001)
LO, HI = EPS, np.float32(1.0) - EPS


def seeded_p(rng, n):
    """Clamped probabilities as the mixers' kernel emits them: mostly confident ones, with both clamps and 0.5 among
    them."""
    u = rng.random(n, dtype=np.float32)
    p = np.where(rng.random(n) < 0.5, u * u * np.float32(0.1), np.float32(1.0) - u * u * np.float32(0.1)).astype(np.float32)
    mid = rng.random(n) < 0.2
    p[mid] = rng.random(int(mid.sum()), dtype=np.float32)
    p = np.clip(p, LO, HI).astype(np.float32)
    p[rng.integers(0, n, n // 16)] = LO
    p[rng.integers(0, n, n // 16)] = HI
    p[rng.integers(0, n, n // 16)] = np.float32(0.5)
    p[:3] = [LO, HI, np.float32(0.5)]
    return p


def cases():
    rng = np.random.default_rng(2024)
    n = 1600
    p = seeded_p(rng, n)
    bits = (rng.random(n) < p).astype(np.uint8)   # bits that follow p, as a decoder's do
    bits[::97] ^= 1                               # ... and some that do not
    yield "encoded", np.frombuffer(gmxo.encode(bits, p), np.uint8), p, bits
    yield "random64", rng.integers(0, 256, 64, dtype=np.uint8), seeded_p(rng, 1800), None
    yield "dry3", np.array([0x5a, 0x00, 0xc3], np.uint8), seeded_p(rng, 160), None


def record(exe, payload, p, td):
    fin, fp, fout, ck = (os.path.join(td, n) for n in ("in.bin", "p.f32", "out.bin", "ck.bin"))
    payload.tofile(fin)
    p.astype("<f4").tofile(fp)
    subprocess.check_call([exe, fin, fp, fout, ck])
    rows = np.fromfile(fout, "<u4").reshape(-1, 4)
    assert len(rows) == len(p)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("GMX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=HERE, help="directory the fixture is written to")
    a = ap.parse_args()
    gmxo.build()
    out = {}
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "ref_decoder_harness")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(a.ref, "src"), "-o", exe,
                               os.path.join(HERE, "ref_decoder_harness.cpp")])
        names = []
        for name, payload, p, bits in cases():
            rows = record(exe, payload, p, td)
            if bits is not None:
                assert np.array_equal(rows[:, 3], bits), "the reference decodes what the oracle's encoder coded"
            assert {int(v) for v in (LO.view(np.uint32), HI.view(np.uint32), np.float32(0.5).view(np.uint32))} <= set(
                p.view(np.uint32).tolist()), name
            names.append(name)
            out[name + "_input"] = payload
            out[name + "_p"] = p.view(np.uint32)
            out[name + "_state"] = rows[:, :3].astype(np.uint32)
            out[name + "_bits"] = rows[:, 3].astype(np.uint8)
            print(name, "input bytes", len(payload), "bits", len(p), "ones", int(rows[:, 3].sum()))
    np.savez_compressed(os.path.join(a.out, "decoder_trace.npz"), names=np.array(names), **out)


if __name__ == "__main__":
    main()
