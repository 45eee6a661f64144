"""Where the analysis averages should be kept: the host loop against the device object.
Recorded, not gated.

    python scripts/bench_analysis.py [--rounds 3] [--reps 3] [--out profiles/analysis_bench.json]

The stock 24/8/1 bank at 64 streams x 2 048 bits and 1 024 x 1 024, records from the device's synthetic fill, the 32
columns the device produces of the stock Predictor's analysed ones: the LSTM's slot, the 30 slots of the 15 skip-context
Indirect models and the final mixer (from p).  Every round is a fresh process per shape; inside it the legs alternate,
and the first repetition of each warms up and is dropped:
  A  what the compressor does today: gmx_group_run, download of p, a device-to-host copy of the size of the model
     predictions and active flags WantsModels asks for (450 bytes per bit and stream: the Indirect bank's [2 x 41]
     floats and flags, the Match bank's and the LSTM's; the banks themselves are not in this benchmark, the copy is a
     pinned one of that many bytes), then gmx_analysis_entropy / gmx_analysis_step (scripts/analysis_host_leg.cpp)
     for the 32 columns on 1 and on 16 host threads.  (The synthetic records live on the device only; the host loop
     averages seeded logits and the downloaded p.)
  B  gmx_group_run, gmx_analysis_update_batch, gmx_analysis_take.
Written down: wall time per launch of each leg, the update kernel's time from kernel_ms beside the mixer kernel's own
of the same batch, bytes over the link per leg, and `make report-analysis`.  Spread: min / median / max over all
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
SHAPES = {"stock_64x2048": (64, 2048), "stock_1024x1024": (1024, 1024)}
MODEL_BYTES_PER_BIT = 450
COLUMNS = [(0, 1)] + [(0, i) for i in range(36, 66)] + [(2, 0)]


def helper(td):
    so = os.path.join(td, "analysis_host_leg.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "scripts", "analysis_host_leg.cpp")])
    L = C.CDLL(so)
    L.gmx_host_leg_analysis.restype = None
    L.gmx_host_leg_analysis.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p,
                                        C.POINTER(C.c_double)]
    return L


def child(shape, reps):
    import numpy as np
    import torch

    import gmix_amd
    from gmix_amd import topology
    S, T = SHAPES[shape]
    nc = len(COLUMNS)
    g = gmix_amd.MixerGroup(topology.stock(90), S)
    b = gmix_amd.Batch(g, T, outputs=False, mask=True)
    an = gmix_amd.Analysis(S, COLUMNS, 0)
    models_dev = torch.zeros(MODEL_BYTES_PER_BIT * S * T, dtype=torch.uint8, device="cuda")
    models_host = torch.zeros(MODEL_BYTES_PER_BIT * S * T, dtype=torch.uint8).pin_memory()
    rows = []
    synth = dict(ctx_mode=3, ctx_mod=6, zero_mod=8, bit_mode=1)
    with tempfile.TemporaryDirectory() as td:
        H = helper(td)
        rng = np.random.default_rng(1)
        bits = rng.integers(0, 2, (S, T)).astype(np.uint8)
        values = (rng.standard_normal((S, T, nc)).astype(np.float32) * np.float32(3)).astype(np.float32)
        ema = np.zeros((S, nc), np.float64)
        ns = C.c_double(0)

        def host(threads):
            H.gmx_host_leg_analysis(values.ctypes.data, bits.ctypes.data, S, T, nc, threads, ema.ctypes.data, C.byref(ns))
            return ns.value * 1e-6

        b.fill_synthetic(T, seed=3, restart=True, **synth)
        for rep in range(reps + 1):                      # (the first repetition warms up and is dropped)
            r = {}
            # leg A
            b.fill_synthetic(T, seed=3, restart=False, **synth)
            g.sync()
            t0 = time.perf_counter()
            g.run(b)
            b.download()
            b.wait()
            t1 = time.perf_counter()
            models_host.copy_(models_dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            values[:, :, nc - 1] = b.p
            ms1 = host(1)
            ms16 = host(16)
            r["a_run_download_p_ms"] = (t1 - t0) * 1e3
            r["a_download_models_ms"] = (t2 - t1) * 1e3
            r["a_host_1t_ms"], r["a_host_16t_ms"] = ms1, ms16
            r["a_wall_1t_ms"], r["a_wall_16t_ms"] = (t2 - t0) * 1e3 + ms1, (t2 - t0) * 1e3 + ms16
            r["a_host_ns_per_bit_1t"] = ms1 * 1e6 / (S * T)
            r["a_host_ns_per_bit_16t"] = ms16 * 1e6 / (S * T)
            r["a_link_bytes"] = (4 + MODEL_BYTES_PER_BIT) * S * T
            # leg B
            b.fill_synthetic(T, seed=3, restart=False, **synth)
            g.sync()
            t0 = time.perf_counter()
            g.run(b)
            an.update_batch(b, T)
            an.take()
            t1 = time.perf_counter()
            r["b_wall_ms"] = (t1 - t0) * 1e3
            r["b_link_bytes"] = an.d2h_bytes()
            # the kernels' own times, one launch each
            b.fill_synthetic(T, seed=3, restart=False, **synth)
            r["mixer_kernel_ms"] = g.run(b, timed=True)
            r["update_kernel_ms"] = an.update_batch(b, T, timed=True)
            an.take()
            if rep:
                rows.append(r)
    an.close()
    b.close()
    g.close()
    print("ROWS " + json.dumps(rows))


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analysis_bench.json"))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    import gmix_amd
    result = {"build": gmix_amd._lib.lib().gmx_build_info().decode(), "rounds": a.rounds, "reps": a.reps,
              "columns": len(COLUMNS), "model_bytes_per_bit": MODEL_BYTES_PER_BIT, "shapes": {}}
    rows = {k: [] for k in SHAPES}
    for _ in range(a.rounds):
        for shape in SHAPES:                             # a fresh process per shape and round
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=500)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                return 1
            rows[shape] += json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")][-1][5:])
    for shape, (S, T) in SHAPES.items():
        keys = rows[shape][0].keys()
        result["shapes"][shape] = {"topology": "stock", "streams": S, "bits": T,
                                   **{k: spread([r[k] for r in rows[shape]]) for k in keys}}
        m = result["shapes"][shape]
        m["update_over_mixer_kernel"] = m["update_kernel_ms"]["median"] / m["mixer_kernel_ms"]["median"]
    rep = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gmix_amd", "csrc"), "report-analysis"],
                         capture_output=True, text=True)
    result["report_analysis"] = [ln.split("remark:")[-1].split("[-R")[0].strip() for ln in rep.stdout.splitlines()]
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["shapes"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
