"""Where PPMd should run: the host loop against the device bank.  Recorded, not gated.

    python scripts/bench_ppmd.py [--rounds 3] [--reps 2] [--out profiles/ppmd_bench.json]

Order 20, arena 64 MB, 16 384 bytes of `noisy500` and of `abcd` (tests/ppmd_common.py; stream s reads the input rotated
by 61 s bytes) at S = 1, 64 and 256 streams.  Every round is a fresh process per shape and input; inside it the legs
alternate, and the first repetition of each warms up and is dropped:
  A  gmix_amd/csrc/gmx_ppmd.h built for the host with -O2 (scripts/ppmd_host_leg.cpp) -- the restatement, not the
     reference's own build -- as batch records, a model per stream: on 1 thread over at most 8 of the streams, and on
     16 threads over all of them;
  B  gmx_ppmd_run of the same records: upload of the bytes, the launch, download of the predictions, flags and `used`
     (the distributions stay on the device, where gmx_ppmd_feed hands them on), wait.
Written down: microseconds per byte step (one byte of every stream) and per stream-byte for each leg, the kernel's time
from events (kernel_ms) in a pass of its own, whether the last distributions of both legs are bit for bit the same, and
`make report-ppmd`.  Spread: min / median / max over all repetitions of all rounds."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
STREAMS = (1, 64, 256)
INPUTS = ("noisy500", "abcd")
N, ORDER, ARENA_MB = 16384, 20, 64
ONE_THREAD_STREAMS = 8


def helper(td):
    so = os.path.join(td, "ppmd_host_leg.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "scripts", "ppmd_host_leg.cpp")])
    L = C.CDLL(so)
    L.gmx_host_leg_ppmd.restype = C.c_double
    L.gmx_host_leg_ppmd.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def child(S, name, reps):
    import numpy as np

    import gmix_amd
    import ppmd_common as pc
    from gmix_amd.bank import PPMD_PPM, PPMD_PREDICTIONS, PPMD_USED
    d = pc.case_bytes(name, N)
    data = np.stack([np.roll(d, -61 * s) for s in range(S)])
    g = gmix_amd.PpmdGroup(S, ORDER, ARENA_MB)
    b = gmix_amd.PpmdBatch(g, N)
    rows = []
    with tempfile.TemporaryDirectory() as td:
        H = helper(td)
        last = np.zeros((S, 256), np.float32)

        def host(n_streams, threads):
            ns = H.gmx_host_leg_ppmd(data.ctypes.data, n_streams, N, ORDER, ARENA_MB, threads, last.ctypes.data)
            assert ns > 0
            return ns * 1e-3

        for rep in range(reps + 1):                      # (the first repetition warms up and is dropped)
            r = {}
            s1 = min(S, ONE_THREAD_STREAMS)
            us1 = host(s1, 1)
            us16 = host(S, 16)
            r["a_1t_us_per_stream_byte"] = us1 / (s1 * N)
            r["a_16t_us_per_byte_step"] = us16 / N
            r["a_16t_us_per_stream_byte"] = us16 / (S * N)
            g.reset()
            g.sync()
            b.bytes[:] = data
            t0 = time.perf_counter()
            b.upload(N)
            g.run(b, N)
            b.download(N, PPMD_PREDICTIONS | PPMD_USED)
            b.wait()
            t1 = time.perf_counter()
            r["b_us_per_byte_step"] = (t1 - t0) * 1e6 / N
            r["b_us_per_stream_byte"] = (t1 - t0) * 1e6 / (S * N)
            b.download(N, PPMD_PPM)
            b.wait()
            r["same_last_distribution"] = int(np.array_equal(b.ppm[:, N - 1].view(np.uint32), last.view(np.uint32)))
            # the kernel's own time, in a pass of its own
            g.reset()
            g.sync()
            ms = g.run(b, N, timed=True)
            r["kernel_us_per_byte_step"] = ms * 1e3 / N
            r["kernel_us_per_stream_byte"] = ms * 1e3 / (S * N)
            r["restores"] = max(g.restores(s) for s in range(S))
            if rep:
                rows.append(r)
    b.close()
    g.close()
    print("ROWS " + json.dumps(rows))


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppmd_bench.json"))
    ap.add_argument("--streams", type=int, nargs="*", default=list(STREAMS))
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), a.child[1], a.reps)
    import gmix_amd
    result = {"build": gmix_amd._lib.lib().gmx_build_info().decode(), "rounds": a.rounds, "reps": a.reps, "bytes": N,
              "order": ORDER, "arena_mb": ARENA_MB, "leg_a": "gmx_ppmd.h built for the host (-O2), not the reference",
              "one_thread_streams": ONE_THREAD_STREAMS, "shapes": {}}
    shapes = [(S, name) for S in a.streams for name in INPUTS]
    rows = {k: [] for k in shapes}
    for _ in range(a.rounds):
        for S, name in shapes:                           # a fresh process per shape and round
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(S), name, "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                return 1
            rows[(S, name)] += json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")][-1][5:])
    for S, name in shapes:
        keys = rows[(S, name)][0].keys()
        result["shapes"]["%s_S%d" % (name, S)] = {"input": name, "streams": S,
                                                  **{k: spread([r[k] for r in rows[(S, name)]]) for k in keys}}
    rep = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gmix_amd", "csrc"), "report-ppmd"],
                         capture_output=True, text=True)
    result["report_ppmd"] = [ln.split("remark:")[-1].split("[-R")[0].strip() for ln in rep.stdout.splitlines()]
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["shapes"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
