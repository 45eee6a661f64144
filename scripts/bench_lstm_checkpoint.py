#!/usr/bin/env python3
"""Times the checkpoint of a whole LSTM group: gmx_lstm_group_export / gmx_lstm_group_import (sections laid out on the
device, gmix_amd/csrc/gmx_lstm_ckpt.hip, and staged through pinned buffers) against the loop of gmx_lstm_export /
gmx_lstm_import over the same streams of the same process -- the per-stream calls are the parent commit's code path,
unchanged.

    python scripts/bench_lstm_checkpoint.py --out profiles/lstm_checkpoint_bench.json

One process per group size (a fresh child each; never two at a time).  A leg creates the group, gives every stream the
reference's initial weights and lets it learn 230 synthetic bytes (two backward passes and 30 bytes: the arrays a
backward pass leaves behind are not zero), synchronises, and times with the host's clock around calls that are
synchronous themselves: 1 warm-up, then 5 exports, then 5 imports of what was exported (the state does not change) --
first the group calls, then the per-stream loop.  The median and (max - min) / median of the five are reported.  For
scale the leg also times one pinned device-to-host copy of as many bytes as the group's checkpoint has (up to 256 MiB
at a time), the link's own rate."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = (16, 64, 256)
BYTES = 230
WARMUP, TIMED = 1, 5


def d2h_gbps(total):
    """One pinned hipMemcpy device -> host of `total` bytes, in pieces of at most 256 MiB: GB/s."""
    with open("/proc/self/maps") as f:         # the HIP runtime that libgmxmix.so has already brought in
        path = next(ln.split()[-1] for ln in f if "libamdhip64" in ln)
    hip = C.CDLL(path)
    piece = min(total, 256 << 20)
    d, h = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(piece)) == 0
    assert hip.hipHostMalloc(C.byref(h), C.c_size_t(piece), 0) == 0
    assert hip.hipMemset(d, 1, C.c_size_t(piece)) == 0
    best = None
    for k in range(WARMUP + TIMED):
        assert hip.hipDeviceSynchronize() == 0
        t = time.perf_counter()
        left = total
        while left > 0:
            n = min(left, piece)
            assert hip.hipMemcpy(h, d, C.c_size_t(n), 2) == 0  # hipMemcpyDeviceToHost
            left -= n
        dt = time.perf_counter() - t
        if k >= WARMUP and (best is None or dt < best):
            best = dt
    hip.hipFree(d)
    hip.hipHostFree(h)
    return total / best / 1e9


def leg(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import gmix_amd
    from oracle import gmxo
    S = a.streams
    g = gmix_amd.LstmGroup(S)
    w = gmxo.LstmModel().weights()
    b = gmix_amd.LstmBatch(g, BYTES)
    for s in range(S):
        g.set_weights(w, stream=s)
        ppm, data = gmxo.lstm_synth(BYTES, seed=1 + s % 16, mask=(255, 127, 63, 15)[s % 4])
        b.ppm[s] = ppm
        b.bytes[s] = np.roll(data, s // 16)       # (16 syntheses, rotated: no two streams alike)
    b.upload(BYTES)
    g.run(b, BYTES, learn=True)
    g.sync()
    b.close()
    L = g.L
    vp = C.c_void_p
    nl, ns = C.c_size_t(0), C.c_size_t(0)
    assert L.gmx_lstm_group_export(g.h, 0, S, None, 0, None, 0, C.byref(nl), C.byref(ns)) == 0
    nl, ns = nl.value, ns.value
    times = {"group_export": [], "group_import": [], "loop_export": [], "loop_import": []}
    bl, bs = np.zeros(S * nl, np.uint8), np.zeros(S * ns, np.uint8)
    for k in range(WARMUP + TIMED):
        g.sync()
        t = time.perf_counter()
        rc = L.gmx_lstm_group_export(g.h, 0, S, bl.ctypes.data_as(vp), bl.size, bs.ctypes.data_as(vp), bs.size, None, None)
        times["group_export"].append((time.perf_counter() - t) * 1e3)
        assert rc == 0, rc
    for k in range(WARMUP + TIMED):
        g.sync()
        t = time.perf_counter()
        rc = L.gmx_lstm_group_import(g.h, 0, S, bl.ctypes.data_as(vp), bl.size, bs.ctypes.data_as(vp), bs.size)
        times["group_import"].append((time.perf_counter() - t) * 1e3)
        assert rc == 0, rc
    # the per-stream loop, into and out of buffers of its own
    pl, ps = np.zeros(S * nl, np.uint8), np.zeros(S * ns, np.uint8)
    for k in range(WARMUP + TIMED):
        g.sync()
        t = time.perf_counter()
        for s in range(S):
            cl, cs = C.c_size_t(nl), C.c_size_t(ns)
            rc = L.gmx_lstm_export(g.h, s, pl[s * nl:].ctypes.data_as(vp), C.byref(cl), ps[s * ns:].ctypes.data_as(vp),
                                   C.byref(cs))
            assert rc == 0 and (cl.value, cs.value) == (nl, ns), rc
        times["loop_export"].append((time.perf_counter() - t) * 1e3)
    same = bool(np.array_equal(pl, bl) and np.array_equal(ps, bs))
    for k in range(WARMUP + TIMED):
        g.sync()
        t = time.perf_counter()
        for s in range(S):
            rc = L.gmx_lstm_import(g.h, s, pl[s * nl:].ctypes.data_as(vp), nl, ps[s * ns:].ctypes.data_as(vp), ns)
            assert rc == 0, rc
        times["loop_import"].append((time.perf_counter() - t) * 1e3)
    distinct = len({ps[s * ns:(s + 1) * ns].tobytes() for s in range(S)})
    g.close()
    total = S * (nl + ns)

    def stat(ms):
        ms = ms[WARMUP:]
        med = sorted(ms)[len(ms) // 2]
        return {"ms": [round(x, 3) for x in ms], "median_ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4)}

    res = {"streams": S, "bytes_learned": BYTES, "checkpoint_bytes": total, "group_equals_loop": same,
           "distinct_short_sections": distinct, "d2h_pinned_gbps": round(d2h_gbps(total), 2),
           "build": L.gmx_build_info().decode()}
    res.update({op: stat(ms) for op, ms in times.items()})
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default=",".join(str(s) for s in STREAMS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per leg")
    ap.add_argument("--leg", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg is not None:
        a.streams = a.leg
        return leg(a)
    rows = []
    for S in (int(x) for x in a.streams.split(",")):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", str(S)], capture_output=True, text=True,
                             timeout=a.timeout)
        if out.returncode != 0:   # nothing more is started on the device after a leg that failed
            sys.stderr.write(out.stdout + out.stderr)
            sys.exit(f"{S} streams: exit status {out.returncode}")
        row = json.loads(out.stdout.strip().splitlines()[-1])
        assert row["group_equals_loop"], "the group export and the per-stream loop disagree"
        for op in ("export", "import"):
            t, p = row["group_" + op], row["loop_" + op]
            row[op + "_speedup"] = round(p["median_ms"] / t["median_ms"], 2)
            # faster by more than the two spreads together
            row[op + "_faster"] = p["median_ms"] - t["median_ms"] > p["median_ms"] * p["spread"] + t["median_ms"] * t["spread"]
            row[op + "_group_gbps"] = round(row["checkpoint_bytes"] / t["median_ms"] / 1e6, 2)
        rows.append(row)
        print(f"S={S}: {row['checkpoint_bytes'] / 2**20:.0f} MiB; "
              f"export group {row['group_export']['median_ms']:.1f} ms (+-{row['group_export']['spread']:.2f}) "
              f"loop {row['loop_export']['median_ms']:.1f} ms (+-{row['loop_export']['spread']:.2f}) x{row['export_speedup']}; "
              f"import group {row['group_import']['median_ms']:.1f} ms (+-{row['group_import']['spread']:.2f}) "
              f"loop {row['loop_import']['median_ms']:.1f} ms (+-{row['loop_import']['spread']:.2f}) x{row['import_speedup']}; "
              f"pinned D2H {row['d2h_pinned_gbps']} GB/s", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"warmup": WARMUP, "timed": TIMED, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
