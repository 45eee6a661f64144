"""Regenerates tests/golden/ppmd_trace.npz from the reference's own ModPPMD (build container only: it needs the
reference's sources and g++).  ref_ppmd_harness.cpp is compiled against the reference where it lies, into a temporary
directory, and drives the model through Model's interface; the fixture holds recorded results only, nothing of the
reference's program text, and no input bytes: tests/ppmd_common.py regenerates those from the seed.

    python tests/golden/make_ppmd_golden.py [--ref /path/to/reference]

Per case of ppmd_common.CASES (order 20 unless the name says otherwise, arena 1 MB):
  <case>_used    [n] uint64   ModPPMD::GetMemoryUsage after every byte
  <case>_flushes [f] int64    the bytes at which the model flushed (ppmd_common.flushes: `used` falls by > 64 KiB)
  <case>_rows    [r] int64    the bytes whose whole answer is kept: the first 256 and 64 either side of every flush
  <case>_ppm     [r][256] uint32, <case>_slot [r] uint32   ppm_predictions and the model's slot at those bytes
  <case>_hash    [n // 256] uint64   the running FNV-1a over all ppm bytes after bytes 255, 511, ...
The recipe stops if a case named for a flush shows none.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ppmd_common as pc  # noqa: E402

SOURCES = ("models/mod_ppmd.cpp", "memory/short-term-memory.cpp", "memory/long-term-memory.cpp",
           "contexts/nonstationary.cpp", "contexts/run-map.cpp", "mixer/sigmoid.cpp")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("GMX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=HERE, help="directory the fixture is written to")
    a = ap.parse_args()
    src = os.path.join(a.ref, "src")
    out = {}
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "ref_ppmd_harness")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + src, "-o", exe,
                               os.path.join(HERE, "ref_ppmd_harness.cpp")] + [os.path.join(src, s) for s in SOURCES])
        for name, (_, n, order, must_flush) in pc.CASES.items():
            fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
            pc.case_bytes(name).tofile(fin)
            subprocess.check_call([exe, fin, str(order), str(pc.ARENA_MB), fout])
            rec = np.fromfile(fout, "<u4").reshape(-1, 262)
            assert len(rec) == n, name
            used = rec[:, 258:260].copy().view(np.uint64)[:, 0]
            h = rec[:, 260:262].copy().view(np.uint64)[:, 0]
            fl = pc.flushes(used)
            if must_flush and not fl:
                raise SystemExit("%s: named for a flush and shows none" % name)
            rows = pc.full_rows(n, fl)
            out[name + "_used"] = used
            out[name + "_flushes"] = np.array(fl, np.int64)
            out[name + "_rows"] = rows
            out[name + "_ppm"] = rec[rows, :256].astype(np.uint32)
            out[name + "_slot"] = rec[rows, 256].astype(np.uint32)
            out[name + "_hash"] = h[pc.HASH_EVERY - 1::pc.HASH_EVERY].copy()
            print(name, "bytes", n, "order", order, "flushes", fl, "used", int(used[fl[0] - 1]) if fl else "-", "->",
                  int(used[fl[0]]) if fl else "-", "last", int(used[-1]))
    np.savez_compressed(os.path.join(a.out, "ppmd_trace.npz"), names=np.array(list(pc.CASES)), **out)


if __name__ == "__main__":
    main()
