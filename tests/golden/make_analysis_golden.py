"""Regenerates tests/golden/analysis_trace.npz from the reference's own Predictor (build container only: it needs the
reference's sources and g++).  ref_analysis_harness.cpp is compiled against the reference where it lies, into a
temporary directory, and run there (EnableAnalysis creates analysis/ where it runs); the fixture holds the inputs and the
recorded averages, nothing of the reference's program text.

    python tests/golden/make_analysis_golden.py [--ref /path/to/reference] [--bytes 150]

Three cases (tests/test_analysis_cpu.py replays them, tests/test_analysis_census.py checks what they hold):
  english      analysis on over the first bytes of english_dic_30000.bin: per bit the blackboard, the active set, the
               gate contexts, the mixer outputs, p, the bit, bits_seen at Perceive; entropy[] of the analysed columns
  all_columns  the same run with model_enable_analysis forced true for all 123 entries (entropy[] only: the run's other
               records are english's, which the generator asserts)
  operands     UpdateEntropy called directly on tests/analysis_common.py's operand list
The averages of the two long cases are kept for the bits of `*_kept`: every bit of the first 256 (all_columns: 64), every
16th after that -- the file stays below the largest fixture here.
"""
import argparse
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import analysis_common as ac  # noqa: E402

LIMIT = 643397


def build(ref, td):
    src = os.path.join(ref, "src")
    tus = []
    for d, _, files in os.walk(src):
        if os.path.basename(d) in ("runner", "preprocess"):
            continue
        tus += [os.path.join(d, f) for f in sorted(files) if f.endswith(".cpp")]
    flags = ["g++", "-std=c++17", "-O2", "-w", "-include", "cstring", "-I" + src]
    jobs = [(t, os.path.join(td, "o%d.o" % i)) for i, t in enumerate(sorted(tus))]
    jobs.append((os.path.join(HERE, "ref_analysis_harness.cpp"), os.path.join(td, "harness.o")))
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(lambda j: subprocess.check_call(flags + ["-c", j[0], "-o", j[1]]), jobs))
    exe = os.path.join(td, "ref_analysis_harness")
    subprocess.check_call(["g++", "-o", exe] + [o for _, o in jobs])
    return exe


def read_trace(path):
    raw = open(path, "rb").read()
    n, M, C = np.frombuffer(raw, "<u4", 3)
    at = 12
    cols = np.frombuffer(raw, "<u4", C, at)
    at += 4 * C
    names = []
    for _ in range(C):
        k = int(np.frombuffer(raw, "<u4", 1, at)[0])
        names.append(raw[at + 4:at + 4 + k].decode())
        at += 4 + k
    rec = np.dtype([("pred", "<u4", (n,)), ("act", "u1", (n,)), ("ctx", "<u4", (M,)), ("out", "<u4", (M,)), ("p", "<u4"),
                    ("bit", "u1"), ("seen", "<u8"), ("ent", "<u8", (C,))])
    body = np.frombuffer(raw, rec, offset=at)
    assert at + body.nbytes == len(raw)
    return cols.astype(np.uint32), names, body


def kept(n_bits, dense):
    return np.array([t for t in range(n_bits) if t < dense or t % 16 == 15], np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("GMX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=HERE, help="directory the fixture is written to")
    ap.add_argument("--bytes", type=int, default=150, help="150..300 bytes of english_dic_30000.bin")
    a = ap.parse_args()
    assert 150 <= a.bytes <= 300
    text = os.path.join(HERE, "english_dic_30000.bin")
    out = {}
    with tempfile.TemporaryDirectory() as td:
        exe = build(a.ref, td)
        traces = {}
        for name, every in (("english", 0), ("all_columns", 1)):
            path = os.path.join(td, name + ".bin")
            subprocess.check_call([exe, "trace", text, str(a.bytes), str(every), path], cwd=td)
            traces[name] = read_trace(path)
        cols, names, eng = traces["english"]
        acols, _, full = traces["all_columns"]
        for key in ("pred", "act", "ctx", "out", "p", "bit", "seen"):
            assert np.array_equal(eng[key], full[key]), key
        assert list(acols) == list(range(ac.N_INPUTS + ac.N_MIXERS))
        n_bits = len(eng)
        out["english_pred"], out["english_act"], out["english_ctx"] = eng["pred"], eng["act"], eng["ctx"]
        out["english_out"], out["english_p"], out["english_bits"] = eng["out"], eng["p"], eng["bit"]
        out["english_seen"] = eng["seen"]
        out["english_cols"], out["english_names"] = cols, np.array(names)
        out["english_kept"] = kept(n_bits, 256)
        out["english_ema"] = eng["ent"][out["english_kept"]]
        out["all_columns_cols"] = acols
        out["all_columns_kept"] = kept(n_bits, 64)
        out["all_columns_ema"] = full["ent"][out["all_columns_kept"]]
        thr = ac.thresholds()
        x, bit = ac.operand_records(thr)
        rec = np.zeros(len(x), np.dtype([("x", "<f4"), ("bit", "<u4")]))
        rec["x"], rec["bit"] = x, bit
        fin, fout = os.path.join(td, "ops.in"), os.path.join(td, "ops.out")
        rec.tofile(fin)
        subprocess.check_call([exe, "operands", fin, fout], cwd=td)
        res = np.fromfile(fout, "<u8").reshape(len(x), 3)
        out["operands_x"], out["operands_bits"] = x.view(np.uint32), bit
        out["operands_thresholds"] = thr.view(np.uint32)
        out["operands_from_zero"], out["operands_from_minus_one"], out["operands_chain"] = res[:, 0], res[:, 1], res[:, 2]
    path = os.path.join(a.out, "analysis_trace.npz")
    np.savez_compressed(path, names=np.array(["english", "all_columns", "operands"]), **out)
    size = os.path.getsize(path)
    print("bits", n_bits, "columns", len(cols), "operands", len(x), "bytes", size)
    assert size <= LIMIT, size


if __name__ == "__main__":
    main()
