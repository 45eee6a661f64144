#!/usr/bin/env python3
"""Times the checkpoint of a whole Match group: gmx_match_group_export / gmx_match_group_import (valid entries counted,
every section assembled and scattered on the device, gmix_amd/csrc/gmx_match_ckpt.hip) against a loop of
gmx_match_export / gmx_match_import over the same streams on the same state, in the same process.  The per-stream
calls keep the host code (one round trip after the other) that the commit before the group calls had, so the loop
measures that path; their count and pack kernels walk the tables with gmx_ckpt_walk.h, as the group kernels do.

    python scripts/bench_match_checkpoint.py --out profiles/match_group_checkpoint.json

One process per case (a fresh child each; never two at a time).  A case creates the bank of the six stock models
(topology of predictor.cpp:187-208: tables 256, 65 536, 16 Mi, 3 x 2 Mi, limit 400), runs 2 048 bits of the fixtures'
stream generator (gmix_amd.match.match_stream, another seed per stream) through gmx_match_run, synchronises, and
times with the host's clock around calls that end in a synchronise themselves: 3 warm-up calls, then 10 timed ones,
the two paths alternating call by call.  The median and (max - min) / median of the ten are reported.

What is timed:
  group       sizing call + gmx_match_group_export into one buffer; gmx_match_group_import from it
  per_stream  per stream the sizing call + gmx_match_export; per stream one gmx_match_import
Both paths must produce the same bytes; the script asserts it before it times anything."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STOCK = [(256, 400), (65536, 400), (1 << 24, 400), (1 << 21, 400), (1 << 21, 400), (1 << 21, 400)]
CASES = {"stock_S16_2048": 16, "stock_S64_2048": 64}
BITS = 2048
WARMUP, TIMED = 3, 10


def hashes(data):
    """One context value per model and byte -- hashes of the last 1..6 bytes, as the reference's contexts are -- [n][6]"""
    import numpy as np
    h = np.zeros((len(data), len(STOCK)), np.uint32)
    acc = np.zeros(len(data), np.uint64)
    prev = np.concatenate((np.zeros(len(STOCK), np.uint8), data))
    for k in range(len(STOCK)):
        acc = (acc * np.uint64(0x2F0B4A27) + prev[len(STOCK) - 1 - k:len(prev) - 1 - k].astype(np.uint64) + np.uint64(1)) \
            & np.uint64(0xffffffff)
        h[:, k] = acc.astype(np.uint32)
    return h


def case(name):
    import numpy as np
    import gmix_amd
    from gmix_amd.match import match_stream, stream_bits
    S = CASES[name]
    g = gmix_amd.MatchGroup(STOCK, BITS // 8 + 64, S)
    b = gmix_amd.MatchBatch(g, BITS)
    for s in range(S):
        data = match_stream(100 + s, BITS // 8)
        bits, bc = stream_bits(data)
        b.set_records(s, np.repeat(hashes(data), 8, axis=0), bc, bits)
    b.upload(BITS)
    g.run(b, BITS)
    g.sync()
    b.close()
    L, K = g.L, g.K
    vp = C.c_void_p

    def p(a):
        return a.ctypes.data_as(vp)

    off = (C.c_size_t * (S + 1))()
    assert L.gmx_match_group_export(g.h, 0, S, None, 0, off, None) == 0
    need = off[S]
    gl, gs = np.zeros(need, np.uint8), np.zeros(11 * K * S, np.uint8)
    pl = [np.zeros(off[s + 1] - off[s], np.uint8) for s in range(S)]
    ps = [np.zeros(11 * K, np.uint8) for s in range(S)]

    def group_export():
        assert L.gmx_match_group_export(g.h, 0, S, None, 0, off, None) == 0
        assert L.gmx_match_group_export(g.h, 0, S, p(gl), gl.size, off, p(gs)) == 0

    def per_stream_export():
        for s in range(S):
            nl, ns = C.c_size_t(0), C.c_size_t(0)
            assert L.gmx_match_export(g.h, s, None, C.byref(nl), None, C.byref(ns)) == 0
            assert nl.value == pl[s].size and ns.value == ps[s].size
            assert L.gmx_match_export(g.h, s, p(pl[s]), C.byref(nl), p(ps[s]), C.byref(ns)) == 0

    def group_import():
        assert L.gmx_match_group_import(g.h, 0, S, p(gl), off, p(gs)) == 0

    def per_stream_import():
        for s in range(S):
            assert L.gmx_match_import(g.h, s, p(pl[s]), pl[s].size, p(ps[s]), ps[s].size) == 0

    group_export()
    per_stream_export()
    assert gl.tobytes() == b"".join(x.tobytes() for x in pl) and gs.tobytes() == b"".join(x.tobytes() for x in ps), \
        "the two paths do not write the same bytes"
    times = {"group_export": [], "per_stream_export": [], "group_import": [], "per_stream_import": []}
    legs = {"group_export": group_export, "per_stream_export": per_stream_export, "group_import": group_import,
            "per_stream_import": per_stream_import}
    for pair in (("group_export", "per_stream_export"), ("group_import", "per_stream_import")):
        for k in range(WARMUP + TIMED):
            for leg in pair:                      # alternating: both see the same moments of a shared host
                g.sync()
                t = time.perf_counter()
                legs[leg]()
                times[leg].append((time.perf_counter() - t) * 1e3)
    # the imports restored what was exported
    keep = gl.tobytes()
    group_export()
    assert gl.tobytes() == keep
    ops = C.c_uint64(0)
    L.gmx_debug_match_group_ops.argtypes = [vp, C.POINTER(C.c_uint64)]
    n0 = (L.gmx_debug_match_group_ops(g.h, C.byref(ops)), ops.value)[1]
    group_export()
    n1 = (L.gmx_debug_match_group_ops(g.h, C.byref(ops)), ops.value)[1]
    group_import()
    n2 = (L.gmx_debug_match_group_ops(g.h, C.byref(ops)), ops.value)[1]
    bank_bytes = int(g.bank_bytes)
    g.close()

    def stat(ms):
        ms = ms[WARMUP:]
        med = sorted(ms)[len(ms) // 2]
        return {"ms": [round(x, 3) for x in ms], "median_ms": round(med, 3),
                "spread": round((max(ms) - min(ms)) / med, 4)}

    res = {"case": name, "streams": S, "bits_per_stream": BITS, "section_bytes": int(need),
           "bank_bytes": S * bank_bytes, "group_export_device_ops": n1 - n0, "group_import_device_ops": n2 - n1,
           "build": L.gmx_build_info().decode()}
    res.update({k: stat(v) for k, v in times.items()})
    for op in ("export", "import"):
        gq, pq = res["group_" + op], res["per_stream_" + op]
        res[op + "_speedup"] = round(pq["median_ms"] / gq["median_ms"], 2)
        # faster by more than the two spreads together
        res[op + "_faster"] = bool(pq["median_ms"] - gq["median_ms"] >
                                   pq["median_ms"] * pq["spread"] + gq["median_ms"] * gq["spread"])
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        return case(a.case)
    rows = []
    for name in a.cases.split(","):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], capture_output=True,
                             text=True, timeout=a.timeout)
        if out.returncode != 0:   # nothing more is started on the device after a case that failed
            sys.stderr.write(out.stdout + out.stderr)
            sys.exit(f"{name}: exit status {out.returncode}")
        r = json.loads(out.stdout.strip().splitlines()[-1])
        rows.append(r)
        print(f"{name}: sections {r['section_bytes'] / 2**20:.2f} MiB of {r['bank_bytes'] / 2**20:.0f} MiB of banks; "
              f"export group {r['group_export']['median_ms']:.2f} ms (+-{r['group_export']['spread']:.2f}) / per stream "
              f"{r['per_stream_export']['median_ms']:.2f} ms (+-{r['per_stream_export']['spread']:.2f}) = "
              f"x{r['export_speedup']}; import group {r['group_import']['median_ms']:.2f} ms "
              f"(+-{r['group_import']['spread']:.2f}) / per stream {r['per_stream_import']['median_ms']:.2f} ms "
              f"(+-{r['per_stream_import']['spread']:.2f}) = x{r['import_speedup']}", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"warmup": WARMUP, "timed": TIMED, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
