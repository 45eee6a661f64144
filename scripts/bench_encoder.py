"""Where the coder should run: the host loop against the device encoder.  Recorded, not gated.

    python scripts/bench_encoder.py [--rounds 3] [--reps 5] [--out profiles/encoder_bench.json]

Two shapes: BASELINE configs[1]'s (one 256-input mixer, 4 096 streams x 1 024 bits) and the stock bank's (1 024 x 1 024),
records from the device's synthetic fill.  Every round is a fresh process per shape; inside it the legs alternate:
  A  gmx_group_run, download of p, wait, then gmx_encoder_bit (gmx_encoder.h, scripts/encoder_host_leg.cpp) over the
     whole batch on 1 and on 16 host threads.  (The synthetic bits live on the device only; the host loop codes random
     bits under the downloaded p, and the link is charged the 4 bytes per bit of p that were actually copied, not the 5
     a caller with real records brings home.)
  B  gmx_group_run, gmx_encoder_encode_batch, gmx_encoder_flush, gmx_encoder_take.
Written down: wall time per launch of each leg, the encode kernel's time from kernel_ms beside the mixer kernel's own
of the same launch, bytes over the link per leg, and `make report-encoder`.  Spread: min / median / max over all
repetitions of all rounds."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"configs1_single256": ("single", 4096, 1024), "stock": ("stock", 1024, 1024)}


def helper(td):
    so = os.path.join(td, "encoder_host_leg.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "scripts", "encoder_host_leg.cpp")])
    L = C.CDLL(so)
    L.gmx_host_leg_encode.restype = C.c_uint64
    L.gmx_host_leg_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p,
                                      C.POINTER(C.c_double)]
    return L


def child(shape, reps):
    import numpy as np

    import gmix_amd
    from gmix_amd import topology
    kind, S, T = SHAPES[shape]
    topo = topology.single(256) if kind == "single" else topology.stock(90)
    g = gmix_amd.MixerGroup(topo, S)
    b = gmix_amd.Batch(g, T, outputs=False, mask=False)
    e = gmix_amd.Encoder(S, T)
    rows = []
    with tempfile.TemporaryDirectory() as td:
        H = helper(td)
        bits = np.random.default_rng(1).integers(0, 2, (S, T)).astype(np.uint8)
        scratch = np.zeros(S * (4 * T + 5), np.uint8)
        ns = C.c_double(0)

        def host(threads, p):
            n = H.gmx_host_leg_encode(p.ctypes.data, bits.ctypes.data, S, T, T, threads, scratch.ctypes.data, C.byref(ns))
            return ns.value * 1e-6, int(n)

        b.fill_synthetic(T, seed=3, restart=True, ctx_mode=3, ctx_mod=6, zero_mod=8, bit_mode=1)
        for rep in range(reps + 1):                      # (the first repetition warms up and is dropped)
            r = {}
            # leg A
            b.fill_synthetic(T, seed=3, restart=False, ctx_mode=3, ctx_mod=6, zero_mod=8, bit_mode=1)
            g.sync()
            t0 = time.perf_counter()
            g.run(b)
            b.download()
            b.wait()
            t1 = time.perf_counter()
            ms1, bytes1 = host(1, b.p)
            ms16, _ = host(16, b.p)
            r["a_run_download_ms"] = (t1 - t0) * 1e3
            r["a_host_1t_ms"], r["a_host_16t_ms"] = ms1, ms16
            r["a_wall_1t_ms"], r["a_wall_16t_ms"] = r["a_run_download_ms"] + ms1, r["a_run_download_ms"] + ms16
            r["a_host_ns_per_bit_1t"] = ms1 * 1e6 / (S * T)
            r["a_host_ns_per_bit_16t"] = ms16 * 1e6 / (S * T)
            r["a_link_bytes"] = 4 * S * T
            r["a_bytes_produced"] = bytes1
            # leg B
            b.fill_synthetic(T, seed=3, restart=False, ctx_mode=3, ctx_mod=6, zero_mod=8, bit_mode=1)
            g.sync()
            t0 = time.perf_counter()
            g.run(b)
            e.encode_batch(b, T)
            e.flush()
            out = e.take()
            t1 = time.perf_counter()
            r["b_wall_ms"] = (t1 - t0) * 1e3
            r["b_link_bytes"] = e.d2h_bytes()
            r["b_bytes_produced"] = sum(len(x) for x in out)
            e.reset()
            # the kernels' own times, one launch each
            b.fill_synthetic(T, seed=3, restart=False, ctx_mode=3, ctx_mod=6, zero_mod=8, bit_mode=1)
            r["mixer_kernel_ms"] = g.run(b, timed=True)
            r["encode_kernel_ms"] = e.encode_batch(b, T, timed=True)
            e.take()
            e.reset()
            if rep:
                rows.append(r)
    e.close()
    b.close()
    g.close()
    print("ROWS " + json.dumps(rows))


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_bench.json"))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    import gmix_amd
    result = {"build": gmix_amd._lib.lib().gmx_build_info().decode(), "rounds": a.rounds, "reps": a.reps, "shapes": {}}
    rows = {k: [] for k in SHAPES}
    for _ in range(a.rounds):
        for shape in SHAPES:                             # a fresh process per shape and round
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=500)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                return 1
            rows[shape] += json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")][-1][5:])
    for shape, (kind, S, T) in SHAPES.items():
        keys = rows[shape][0].keys()
        result["shapes"][shape] = {"topology": kind, "streams": S, "bits": T,
                                   **{k: spread([r[k] for r in rows[shape]]) for k in keys}}
        m = result["shapes"][shape]
        m["encode_over_mixer_kernel"] = m["encode_kernel_ms"]["median"] / m["mixer_kernel_ms"]["median"]
    rep = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gmix_amd", "csrc"), "report-encoder"],
                         capture_output=True, text=True)
    result["report_encoder"] = [ln.split("remark:")[-1].split("[-R")[0].strip() for ln in rep.stdout.splitlines()]
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["shapes"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
