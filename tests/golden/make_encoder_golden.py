"""Regenerates tests/golden/encoder_trace.npz from the reference's own Encoder (build container only: it needs the
reference's sources and g++).  ref_encoder_harness.cpp is compiled against coder/encoder.cpp where it lies, into a
temporary directory; the fixture holds the inputs and x1_, x2_ and the byte count after every Encode and the whole
output after Flush, nothing of the reference's program text.

    python tests/golden/make_encoder_golden.py [--ref /path/to/reference]

Three cases: trace_english.npz's 2 400 bits under their recorded p; 2 000 bits of the operand mixture
(tests/encoder_common.py); and a run resumed through ReadCheckpoint from {0x12ffffff, 0x13000000}, from which the first
1 bit emits four bytes.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import encoder_common as ec  # noqa: E402


def cases():
    z = np.load(os.path.join(HERE, "trace_english.npz"))
    yield "english", np.unpackbits(z["bits"]), z["p"].view(np.float32), None
    p, bits = ec.mixture(2000, 77)
    yield "mixture", bits, p, None
    p, bits = ec.mixture(400, 78)
    bits[0] = 1
    yield "resumed", bits, p, ec.FOUR


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("GMX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=HERE, help="directory the fixture is written to")
    a = ap.parse_args()
    out, names = {}, []
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "ref_encoder_harness")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(a.ref, "src"), "-o", exe,
                               os.path.join(HERE, "ref_encoder_harness.cpp")])
        fb, fp, fr, fo, ck = (os.path.join(td, n) for n in ("bits.u8", "p.f32", "rows.bin", "out.bin", "ck.bin"))
        for name, bits, p, start in cases():
            bits.astype(np.uint8).tofile(fb)
            p.astype("<f4").tofile(fp)
            subprocess.check_call([exe, fb, fp, fr, fo, ck] + ([] if start is None else [hex(v) for v in start]))
            rows = np.fromfile(fr, "<u4").reshape(-1, 3)
            assert len(rows) == len(p)
            names.append(name)
            out[name + "_bits"] = bits.astype(np.uint8)
            out[name + "_p"] = p.view(np.uint32)
            out[name + "_state"] = rows[:, :2].astype(np.uint32)
            out[name + "_count"] = rows[:, 2].astype(np.uint32)
            out[name + "_output"] = np.fromfile(fo, np.uint8)
            out[name + "_start"] = np.array((0, ec.M32) if start is None else start, np.uint32)
            print(name, "bits", len(p), "bytes", len(out[name + "_output"]), "first emit", int(rows[0, 2]))
    np.savez_compressed(os.path.join(a.out, "encoder_trace.npz"), names=np.array(names), **out)


if __name__ == "__main__":
    main()
