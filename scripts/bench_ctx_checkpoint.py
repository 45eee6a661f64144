#!/usr/bin/env python3
"""Times the checkpoint of a whole context group: gmx_ctx_group_export / _import and gmx_ctx_group_blackboard_get /
_set (non-zero entries counted, every section assembled and scattered on the device, gmix_amd/csrc/gmx_ctx_ckpt.hip)
against a loop of gmx_ctx_export / _import / _blackboard_get / _set over the same streams on the same state, in the
same process.  The per-stream calls keep the host code (one round trip after the other) that the commit before the
group calls had, but for the validation, a function both imports call, so the loop measures that path; their count and
pack kernels walk the tables with gmx_ckpt_walk.h, as the group kernels do.

    python scripts/bench_ctx_checkpoint.py --out profiles/ctx_group_checkpoint.json

One process per case (a fresh child each; never two at a time).  A case creates the stock bank (the 52 variables of
topology.stock_contexts(): nine hash tables, 201 MB a stream), runs 2 048 or 262 144 bits of scripts/bench_ctx.py's
stream generator (gmix_amd.match.match_stream(1000 + i), sixteen distinct streams) through gmx_ctx_run, synchronises,
and times with the host's clock around calls that end in a synchronise themselves: 3 warm-up calls, then 10 timed ones,
the two paths alternating call by call.  The median and (max - min) / median of the ten are reported.

What is timed:
  group       sizing call + gmx_ctx_group_export into one buffer; gmx_ctx_group_import from it; one
              gmx_ctx_group_blackboard_get; one gmx_ctx_group_blackboard_set
  per_stream  per stream the sizing call + gmx_ctx_export; per stream one gmx_ctx_import, _blackboard_get, _blackboard_set
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

CASES = {"stock_S16_2048": (16, 2048), "stock_S64_2048": (64, 2048),
         "stock_S16_262144": (16, 262144), "stock_S64_262144": (64, 262144)}
LAUNCH_BITS = 8192
DISTINCT = 16
WARMUP, TIMED = 3, 10
LEGS = ("export", "import", "boards_get", "boards_set")


def case(name):
    import numpy as np
    import gmix_amd
    from gmix_amd import topology
    from gmix_amd._lib import CtxBlackboard
    from gmix_amd.match import match_stream
    S, bits_total = CASES[name]
    descs = topology.stock_contexts()[0]
    g = gmix_amd.CtxGroup(descs, S)
    H = g.H
    n_launch = min(LAUNCH_BITS, bits_total)
    b = gmix_amd.CtxBatch(g, n_launch, values=False)
    bits = [np.unpackbits(match_stream(1000 + i, bits_total // 8)) for i in range(DISTINCT)]
    for t0 in range(0, bits_total, n_launch):
        for s in range(S):
            b.bits[s, :n_launch] = bits[s % DISTINCT][t0:t0 + n_launch]
        b.upload(n_launch)
        g.run(b, n_launch)
        b.wait()
    g.sync()
    b.close()
    L = g.L
    vp = C.c_void_p

    def p(a):
        return a.ctypes.data_as(vp)

    off = (C.c_size_t * (S + 1))()
    assert L.gmx_ctx_group_export(g.h, 0, S, None, 0, off, None) == 0
    need = off[S]
    gbuf = np.zeros(need, np.uint8)
    pbuf = [np.zeros(off[s + 1] - off[s], np.uint8) for s in range(S)]
    gboards = (CtxBlackboard * S)()
    pboards = (CtxBlackboard * S)()
    poff = (C.c_size_t * (H + 1))()

    def group_export():
        assert L.gmx_ctx_group_export(g.h, 0, S, None, 0, off, None) == 0
        assert L.gmx_ctx_group_export(g.h, 0, S, p(gbuf), gbuf.size, off, None) == 0

    def per_stream_export():
        for s in range(S):
            n = C.c_size_t(0)
            assert L.gmx_ctx_export(g.h, s, None, C.byref(n), poff) == 0
            assert n.value == pbuf[s].size
            assert L.gmx_ctx_export(g.h, s, p(pbuf[s]), C.byref(n), poff) == 0

    def group_import():
        assert L.gmx_ctx_group_import(g.h, 0, S, p(gbuf), off) == 0

    def per_stream_import():
        for s in range(S):
            assert L.gmx_ctx_import(g.h, s, p(pbuf[s]), pbuf[s].size) == 0

    def group_boards_get():
        assert L.gmx_ctx_group_blackboard_get(g.h, 0, S, gboards) == 0

    def per_stream_boards_get():
        for s in range(S):
            assert L.gmx_ctx_blackboard_get(g.h, s, C.byref(pboards[s])) == 0

    def group_boards_set():
        assert L.gmx_ctx_group_blackboard_set(g.h, 0, S, gboards) == 0

    def per_stream_boards_set():
        for s in range(S):
            assert L.gmx_ctx_blackboard_set(g.h, s, C.byref(pboards[s])) == 0

    group_export()
    per_stream_export()
    group_boards_get()
    per_stream_boards_get()
    assert gbuf.tobytes() == b"".join(x.tobytes() for x in pbuf), "the two paths do not write the same bytes"
    assert bytes(gboards) == bytes(pboards), "the two paths do not read the same boards"
    fns = {"group_export": group_export, "per_stream_export": per_stream_export, "group_import": group_import,
           "per_stream_import": per_stream_import, "group_boards_get": group_boards_get,
           "per_stream_boards_get": per_stream_boards_get, "group_boards_set": group_boards_set,
           "per_stream_boards_set": per_stream_boards_set}
    times = {k: [] for k in fns}
    ops = {}
    for leg in LEGS:
        for k in range(WARMUP + TIMED):
            for path in ("group_", "per_stream_"):       # alternating: both see the same moments of a shared host
                g.sync()
                t = time.perf_counter()
                fns[path + leg]()
                times[path + leg].append((time.perf_counter() - t) * 1e3)
                if path == "group_":
                    ops[leg] = L.gmx_debug_ctx_group_ops(g.h)
    # the imports and sets restored what was exported and read
    keep, keepb = gbuf.tobytes(), bytes(gboards)
    group_export()
    group_boards_get()
    assert gbuf.tobytes() == keep and bytes(gboards) == keepb
    bank_bytes = int(g.bank_bytes)
    g.close()

    def stat(ms):
        ms = ms[WARMUP:]
        med = sorted(ms)[len(ms) // 2]
        return {"ms": [round(x, 3) for x in ms], "median_ms": round(med, 3),
                "spread": round((max(ms) - min(ms)) / med, 4)}

    res = {"case": name, "streams": S, "bits_per_stream": bits_total, "section_bytes": int(need),
           "bank_bytes": S * bank_bytes, "group_device_ops": ops, "build": L.gmx_build_info().decode()}
    res.update({k: stat(v) for k, v in times.items()})
    for leg in LEGS:
        gq, pq = res["group_" + leg], res["per_stream_" + leg]
        res[leg + "_speedup"] = round(pq["median_ms"] / gq["median_ms"], 2)
        # faster by more than the two spreads together
        res[leg + "_faster"] = bool(pq["median_ms"] - gq["median_ms"] >
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
        print(f"{name}: sections {r['section_bytes'] / 2**20:.2f} MiB of {r['bank_bytes'] / 2**20:.0f} MiB of banks; " +
              "; ".join(f"{leg} group {r['group_' + leg]['median_ms']:.2f} ms (+-{r['group_' + leg]['spread']:.2f}) / "
                        f"per stream {r['per_stream_' + leg]['median_ms']:.2f} ms "
                        f"(+-{r['per_stream_' + leg]['spread']:.2f}) = x{r[leg + '_speedup']}" for leg in LEGS),
              flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"warmup": WARMUP, "timed": TIMED, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
