#!/usr/bin/env python3
"""The three many-file drop-in builds against each other, end to end: `gmix_chain_many` (LSTM + Indirect models + mixers
on the device), `gmix_full_many` (... and the six Match models) and `gmix_dev_many` (... and the 38 context objects:
gmx::GpuCtxBank), on bench.py's also.e2e_S64 shape -- 64 files x 100 KB of this repository's documents, compressed
side by side, then restored side by side in lock step (`-d`).  COLD whole processes, exec to exit, the builds
alternating within a round, three rounds.

Per leg: wall seconds and bits/s; user + system CPU seconds of the child (wait4's rusage: the host's share, which is what
moving the context hashes to the device is about); its peak resident set (the stock Predictor keeps 201 MB of
IndirectHash tables per file on the host); md5 of every output -- the builds' compressed files must equal each other's
and every restored file its input.  Each process runs under its own `timeout`; the script stops at the first non-zero
status, and writes what it has after every leg.
  python scripts/e2e_dev.py [--files 64] [--bytes 100000] [--rounds 3] [--chunk 2048] [--limit 900] [--out profiles/dev_e2e.json]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_e2e import DROPIN, corpus, cpu_quota, host_cpu  # noqa: E402

BUILDS = ("gmix_chain_many", "gmix_full_many", "gmix_dev_many")


def md5_of(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def leg(exe, args, limit, tmp):
    """One cold process under `timeout`, waited for with wait4: (wall seconds, user + system seconds and peak RSS bytes of
    the process and its children, the driver's JSON line)."""
    cmd = ["timeout", "-k", "10", str(limit), os.path.join(DROPIN, exe)] + args
    with open(os.path.join(tmp, "stdout"), "w") as so, open(os.path.join(tmp, "stderr"), "w") as se:
        t0 = time.perf_counter()
        p = subprocess.Popen(cmd, stdout=so, stderr=se)
        _, status, ru = os.wait4(p.pid, 0)
        wall = time.perf_counter() - t0
    p.returncode = os.waitstatus_to_exitcode(status)
    if p.returncode != 0:
        raise SystemExit(f"{exe} {' '.join(args[:3])} ...: status {p.returncode}: {open(os.path.join(tmp, 'stderr')).read()[-800:]}")
    return wall, ru.ru_utime + ru.ru_stime, ru.ru_maxrss * 1024, open(os.path.join(tmp, "stdout")).read().strip().splitlines()[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--bytes", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--limit", type=int, default=900, help="seconds each process may take")
    ap.add_argument("--builds", default=",".join(BUILDS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dev_e2e.json"))
    a = ap.parse_args()
    builds = [b for b in a.builds.split(",") if b]
    for b in builds:
        if not os.path.exists(os.path.join(DROPIN, b)):
            raise SystemExit(f"{os.path.join(DROPIN, b)} missing (make -C dropin, needs the reference's sources)")
    S, n = a.files, a.bytes
    bits = 8.0 * S * n
    res = {"shape": f"{S} files x {n} bytes, {a.chunk}-bit chunks, cold whole processes, {a.rounds} rounds, builds alternating",
           "host_cpu": host_cpu(), "cpus_visible": os.cpu_count(), "cpu_quota_cores": cpu_quota(), "bits_per_leg": bits,
           "legs": []}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        files, src = [], None
        for k in range(S):
            data, src = corpus(n, 1531 * k)
            f = os.path.join(tmp, f"f{k}")
            open(f, "wb").write(data)
            files.append(f)
        res["corpus"] = src
        in_md5 = [md5_of(f) for f in files]
        coded_md5 = None
        for rnd in range(a.rounds):
            for exe in builds:
                for mode in ("compress", "decompress"):
                    out_dir = os.path.join(tmp, f"{exe}_{rnd}_{mode}")
                    coded = [os.path.join(tmp, f"{exe}_{rnd}_compress", f"{k}.gmix") for k in range(S)]
                    args = ["-T", str(a.chunk)] + (["-d"] if mode == "decompress" else []) + [out_dir] + (coded if mode == "decompress" else files)
                    wall, cpu_seconds, peak_rss, line = leg(exe, args, a.limit, tmp)
                    st = json.loads(line)
                    if st.get("failed"):
                        raise SystemExit(f"{exe} {mode}: {st['failed']} file(s) failed")
                    if mode == "compress":
                        got = [md5_of(c) for c in coded]
                        coded_md5 = coded_md5 or got
                        same = got == coded_md5
                    else:
                        same = [md5_of(os.path.join(out_dir, f"{k}.out")) for k in range(S)] == in_md5
                    e = {"round": rnd, "build": exe, "mode": mode, "wall_seconds": wall, "bits_per_s": bits / wall,
                         "cpu_seconds": cpu_seconds, "peak_rss_bytes": peak_rss, "outputs_identical": same,
                         "coding_loops_seconds": st.get("wall_seconds"), "launches": st.get("launches")}
                    res["legs"].append(e)
                    print(json.dumps(e), flush=True)
                    summarise(res, builds)
                    json.dump(res, open(a.out, "w"), indent=1)
                    if not same:
                        raise SystemExit(f"{exe} {mode}: outputs differ")
    print(json.dumps(res["summary"]))


def summarise(res, builds):
    res["summary"] = {}
    for exe in builds:
        for mode in ("compress", "decompress"):
            legs = [e for e in res["legs"] if e["build"] == exe and e["mode"] == mode]
            if not legs:
                continue
            s = {"legs": len(legs)}
            for key in ("wall_seconds", "bits_per_s", "cpu_seconds", "peak_rss_bytes"):
                v = [e[key] for e in legs if e[key] is not None]
                if v:
                    s[key] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
            s["outputs_identical"] = all(e["outputs_identical"] for e in legs)
            res["summary"][f"{exe} {mode}"] = s


if __name__ == "__main__":
    main()
