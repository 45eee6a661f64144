#!/usr/bin/env python3
"""Times the checkpoint of a whole Indirect group: gmx_indirect_group_export / gmx_indirect_group_import of this tree
(live entries found, packed and scattered on the device, gmix_amd/csrc/gmx_ind_ckpt.hip) against the PARENT commit's
loop of gmx_indirect_export / gmx_indirect_import over the same streams on the same state.

    python scripts/bench_indirect_checkpoint.py --parent <checkout of the parent commit, library built> \\
        --out profiles/indirect_checkpoint_bench.json

One process per leg and case (a fresh child each; never two at a time).  A leg creates the group, learns (records
generated on the device, gmx_ind_batch_fill_synthetic with ctx_mod (300, 0, 70000, 5) for the 41 stock models and
ind_tiny_dense's (3, 2, 5, 1) for its four small models), synchronises, and times with the host's clock around calls
that are synchronous themselves: 1 warm-up, then 5 exports, then 5 imports of what was exported (the state does not
change).  The median and (max - min) / median of the five are reported.

What is timed per leg:
  this     sizing call + gmx_indirect_group_export into one buffer; gmx_indirect_group_import from it
  parent   per stream ONE gmx_indirect_export into a buffer that is large enough (export), the same behind its sizing
           call, which fetches and walks the dense bank once more (export_sized: what a caller that does not know the
           size pays); per stream one gmx_indirect_import

The table shows whether the new path's time follows the live bytes (off[count]) and not the dense bytes (streams x
bank_bytes).  tiny_S256_30k is the candidate for "no gain" on purpose: its tables are a few hundred entries, most of
them written dense, so there is nothing to skip and the per-stream calls move little."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (models, streams, bits per stream, ctx_mod)
CASES = {
    "stock_S16_8k": ("stock", 16, 8192, (300, 0, 70000, 5)),
    "stock_S64_8k": ("stock", 64, 8192, (300, 0, 70000, 5)),
    "stock_S16_256k": ("stock", 16, 262144, (300, 0, 70000, 5)),
    "stock_S64_256k": ("stock", 64, 262144, (300, 0, 70000, 5)),
    "tiny_S256_30k": ("tiny", 256, 30000, (3, 2, 5, 1)),
}
CHUNK = 8192
WARMUP, TIMED = 1, 5


def leg(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import gmix_amd
    from gmix_amd import topology
    kind, S, T, mod = CASES[a.case]
    models = topology.stock_indirect() if kind == "stock" else [(1, 0.02), (2, 0.005), (3, 0.1), (1, 0.5)]
    z = np.load(os.path.join(ROOT, "tests", "golden", "ind_tiny_dense.npz"))  # the two next-state tables
    g = gmix_amd.IndirectGroup(models, z["ns_next"], z["rm_next"], S)
    b = gmix_amd.IndirectBatch(g, CHUNK)
    for t0 in range(0, T, CHUNK):
        n = min(CHUNK, T - t0)
        b.fill_synthetic(n, seed=11, restart=(t0 == 0), ctx_mod=mod)
        g.run(b, n, learn=True)
    g.sync()
    b.close()
    L = g.L
    bank_bytes = int(g.bank_bytes)
    vp = C.c_void_p
    times = {"export": [], "import": []}
    if a.leg == "this":
        off = (C.c_size_t * (S + 1))()
        buf = None
        for k in range(WARMUP + TIMED):
            g.sync()
            t = time.perf_counter()
            rc = L.gmx_indirect_group_export(g.h, 0, S, None, 0, off)
            assert rc == 0, rc
            if buf is None or buf.size < off[S]:
                buf = np.zeros(off[S], np.uint8)
            rc = L.gmx_indirect_group_export(g.h, 0, S, buf.ctypes.data_as(vp), buf.size, off)
            times["export"].append((time.perf_counter() - t) * 1e3)
            assert rc == 0, rc
        live = int(off[S])
        for k in range(WARMUP + TIMED):
            g.sync()
            t = time.perf_counter()
            rc = L.gmx_indirect_group_import(g.h, 0, S, buf.ctypes.data_as(vp), off)
            times["import"].append((time.perf_counter() - t) * 1e3)
            assert rc == 0, rc
        # the per-stream path agrees with the last section after the imports
        assert g.export(S - 1) == buf[off[S - 1]:off[S]].tobytes()
    else:
        times["export_sized"] = []
        sizes = [0] * S
        for s in range(S):
            n = C.c_size_t(0)
            assert L.gmx_indirect_export(g.h, s, None, C.byref(n)) == 0
            sizes[s] = n.value
        bufs = [np.zeros(max(n, 1), np.uint8) for n in sizes]
        for what in ("export", "export_sized"):
            for k in range(WARMUP + TIMED):
                g.sync()
                t = time.perf_counter()
                for s in range(S):
                    n = C.c_size_t(sizes[s])
                    if what == "export_sized":
                        rc = L.gmx_indirect_export(g.h, s, None, C.byref(n))
                        assert rc == 0, rc
                    rc = L.gmx_indirect_export(g.h, s, bufs[s].ctypes.data_as(vp), C.byref(n))
                    assert rc == 0 and n.value == sizes[s], rc
                times[what].append((time.perf_counter() - t) * 1e3)
        live = sum(sizes)
        for k in range(WARMUP + TIMED):
            g.sync()
            t = time.perf_counter()
            for s in range(S):
                rc = L.gmx_indirect_import(g.h, s, bufs[s].ctypes.data_as(vp), sizes[s])
                assert rc == 0, rc
            times["import"].append((time.perf_counter() - t) * 1e3)
    g.close()

    def stat(ms):
        ms = ms[WARMUP:]
        med = sorted(ms)[len(ms) // 2]
        return {"ms": [round(x, 3) for x in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}

    res = {"case": a.case, "leg": a.leg, "streams": S, "bits_per_stream": T, "ctx_mod": list(mod), "live_bytes": live,
           "dense_bytes": S * bank_bytes, "build": L.gmx_build_info().decode()}
    res.update({op: stat(ms) for op, ms in times.items()})
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per leg")
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
                t, p = row["this"][op], row["parent"][op]
                row[op + "_speedup"] = round(p["median_ms"] / t["median_ms"], 2)
                # faster by more than the two spreads together
                row[op + "_faster"] = p["median_ms"] - t["median_ms"] > p["median_ms"] * p["spread"] + t["median_ms"] * t["spread"]
        rows.append(row)
        t = row["this"]
        print(f"{case}: live {t['live_bytes'] / 2**20:.1f} MiB of {t['dense_bytes'] / 2**20:.0f} MiB dense; "
              f"export {t['export']['median_ms']:.1f} ms (+-{t['export']['spread']:.2f}), "
              f"import {t['import']['median_ms']:.1f} ms (+-{t['import']['spread']:.2f})" +
              (f"; parent export {row['parent']['export']['median_ms']:.1f} ms (+-{row['parent']['export']['spread']:.2f}), "
               f"with sizing {row['parent']['export_sized']['median_ms']:.1f} ms, "
               f"import {row['parent']['import']['median_ms']:.1f} ms (+-{row['parent']['import']['spread']:.2f}); "
               f"x{row['export_speedup']} / x{row['import_speedup']}" if "parent" in row else ""), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"warmup": WARMUP, "timed": TIMED, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
