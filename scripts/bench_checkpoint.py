#!/usr/bin/env python3
"""Times the checkpoint of a whole mixer group: gmx_group_export / gmx_group_import of this tree (learned rows found,
packed and scattered on the device, gmix_amd/csrc/gmx_ckpt.hip) against the PARENT commit's loop of gmx_bank_export /
gmx_bank_import over the same streams on the same state.

    python scripts/bench_checkpoint.py --parent <checkout of the parent commit, library built> \\
        --out profiles/checkpoint_bench.json

One process per leg and case (a fresh child each; never two at a time).  A leg creates the group, learns (records
generated on the device, gmx_batch_fill_synthetic; ctx_mode 4 -- a real run's row changes, as bench.py's
also.stock_real -- for the reference's topology, ctx_mode 0 for the one-mixer bank), synchronises, and times with
the host's clock around calls that are synchronous themselves: 1 warm-up, then 5 exports, then 5 imports of what was
exported (the state does not change).  The median and (max - min) / median of the five are reported.

What is timed per leg:
  this     sizing call + gmx_group_export into one buffer; gmx_group_import from it
  parent   per stream ONE gmx_bank_export into a buffer of bank_bytes + 1 MiB (no sizing call: that would fetch the
           dense bank twice); per stream one gmx_bank_import

The table shows whether the new path's time follows the live bytes (long_off[count]) and not the dense bytes
(streams x bank_bytes).  The one-mixer bank after 262 144 bits per stream is the unfavourable case on purpose: most of
its 65 536 rows are learned, there is little to skip, and the packed bytes are about the dense ones.  Measured
(profiles/checkpoint_bench.json): that case is 7x / 8x faster all the same (pinned slices
instead of one pageable bank at a time, no host scan); the sparse cases 10x to 130x; no case was slower."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (topology, streams, bits per stream, ctx_mode)
CASES = {
    "stock_S16_8k": ("stock", 16, 8192, 4),
    "stock_S64_8k": ("stock", 64, 8192, 4),
    "stock_S16_256k": ("stock", 16, 262144, 4),
    "stock_S64_256k": ("stock", 64, 262144, 4),
    "single_S256_8k": ("single", 256, 8192, 0),
    "single_S256_256k": ("single", 256, 262144, 0),
}
CHUNK = 8192
WARMUP, TIMED = 1, 5


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import gmix_amd
    from gmix_amd import topology
    kind, S, T, mode = CASES[a.case]
    topo = topology.stock(90) if kind == "stock" else topology.single(256, 1 << 16)
    g = gmix_amd.MixerGroup(topo, S)
    b = gmix_amd.Batch(g, CHUNK, outputs=False, mask=False)
    for t0 in range(0, T, CHUNK):
        b.fill_synthetic(CHUNK, seed=11, restart=(t0 == 0), ctx_mode=mode)
        g.run(b, CHUNK, learn=True)
    g.sync()
    b.close()
    L, m = g.L, topo.n_mixers
    bank_bytes = int(g.bank_bytes)
    vp = C.c_void_p
    ex, im = [], []
    if a.leg == "this":
        off = (C.c_size_t * (S + 1))()
        sb = np.zeros(S * 24 * m, np.uint8)
        lb = None
        for k in range(WARMUP + TIMED):
            g.sync()
            t = time.perf_counter()
            rc = L.gmx_group_export(g.h, 0, S, None, 0, off, None)
            assert rc == 0, rc
            if lb is None or lb.size < off[S]:
                lb = np.zeros(off[S], np.uint8)
            rc = L.gmx_group_export(g.h, 0, S, lb.ctypes.data_as(vp), lb.size, off, sb.ctypes.data_as(vp))
            ex.append((time.perf_counter() - t) * 1e3)
            assert rc == 0, rc
        live = int(off[S])
        for k in range(WARMUP + TIMED):
            g.sync()
            t = time.perf_counter()
            rc = L.gmx_group_import(g.h, 0, S, lb.ctypes.data_as(vp), off, sb.ctypes.data_as(vp))
            im.append((time.perf_counter() - t) * 1e3)
            assert rc == 0, rc
        check = g.export(S - 1)   # the per-stream path agrees with the last section after the imports
        assert check[0] == lb[off[S - 1]:off[S]].tobytes() and check[1] == sb[-24 * m:].tobytes()
    else:
        cap = bank_bytes + (1 << 20)
        bufs = [np.zeros(cap, np.uint8) for _ in range(S)]
        shorts = [np.zeros(24 * m, np.uint8) for _ in range(S)]
        sizes = [0] * S
        for k in range(WARMUP + TIMED):
            g.sync()
            t = time.perf_counter()
            for s in range(S):
                nl, ns = C.c_size_t(cap), C.c_size_t(24 * m)
                rc = L.gmx_bank_export(g.h, s, bufs[s].ctypes.data_as(vp), C.byref(nl), shorts[s].ctypes.data_as(vp),
                                       C.byref(ns))
                assert rc == 0, rc
                sizes[s] = nl.value
            ex.append((time.perf_counter() - t) * 1e3)
        live = sum(sizes)
        for k in range(WARMUP + TIMED):
            g.sync()
            t = time.perf_counter()
            for s in range(S):
                rc = L.gmx_bank_import(g.h, s, bufs[s].ctypes.data_as(vp), sizes[s], shorts[s].ctypes.data_as(vp), 24 * m)
                assert rc == 0, rc
            im.append((time.perf_counter() - t) * 1e3)
    g.close()

    def stat(ms):
        ms = ms[WARMUP:]
        med = sorted(ms)[len(ms) // 2]
        return {"ms": [round(x, 3) for x in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}

    print(json.dumps({"case": a.case, "leg": a.leg, "streams": S, "bits_per_stream": T, "ctx_mode": mode,
                      "live_bytes": live, "dense_bytes": S * bank_bytes, "export": stat(ex), "import": stat(im),
                      "build": L.gmx_build_info().decode()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per leg")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    rows = []
    for case in a.cases.split(","):
        row = {"case": case}
        for name, tree in (("this", ROOT), ("parent", a.parent)):
            if not tree:
                continue
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--tree", tree, "--case", case],
                                 capture_output=True, text=True, timeout=a.timeout)
            if out.returncode != 0:   # nothing more is started on the device after a leg that failed
                sys.stderr.write(out.stdout + out.stderr)
                sys.exit(f"{case} / {name}: exit status {out.returncode}")
            row[name] = json.loads(out.stdout.strip().splitlines()[-1])
        if "parent" in row:
            assert row["this"]["live_bytes"] == row["parent"]["live_bytes"], "the two legs did not reach the same state"
            for op in ("export", "import"):
                row[op + "_speedup"] = round(row["parent"][op]["median_ms"] / row["this"][op]["median_ms"], 2)
        rows.append(row)
        t = row["this"]
        print(f"{case}: live {t['live_bytes'] / 2**20:.1f} MiB of {t['dense_bytes'] / 2**20:.0f} MiB dense; "
              f"export {t['export']['median_ms']:.1f} ms (+-{t['export']['spread']:.2f}), "
              f"import {t['import']['median_ms']:.1f} ms (+-{t['import']['spread']:.2f})" +
              (f"; parent export {row['parent']['export']['median_ms']:.1f} ms (+-{row['parent']['export']['spread']:.2f}), "
               f"import {row['parent']['import']['median_ms']:.1f} ms (+-{row['parent']['import']['spread']:.2f}); "
               f"x{row['export_speedup']} / x{row['import_speedup']}" if "parent" in row else ""), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"warmup": WARMUP, "timed": TIMED, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
