#!/usr/bin/env python3
"""Rates of the LSTM byte model at shapes other than the stock one (gmx_lstm_create_shaped, gmx_lstm_any.hip), beside
the stock kernel at the stock shape: bytes/s at 256 and 1 024 streams, Predict x 8 bits + Learn, one backward pass per
launch.  Recorded, not gated.

  python scripts/bench_lstm_shape.py [--streams 256,1024] [--rounds 3] [--out profiles/lstm_shape_bench.json]

Every leg's kernel time is the device-event pair gmx_lstm_run puts around its launch.  Each leg is warmed up with one
launch of the size it is timed at; the legs of a stream count are then timed in turn, round after round (alternating,
so that a drift of the machine lands on all of them), and the spread over the rounds is reported with the median.
Beside each device figure stands tests/lstm_shape_ref.c -- the plain-C restatement, NOT the reference's own build -- on
one host core of the machine the script runs on."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (label, cells, horizon, general kernel?, learn?)  The two legs without Learn split the (50, 100) figures into the
# forward half (Lstm::Predict + the 8 bit predictions) and the rest (Lstm::Perceive with its backward pass).
LEGS = [("stock kernel (50, 100)", 50, 100, False, True), ("general kernel (50, 100)", 50, 100, True, True),
        ("general kernel (100, 100)", 100, 100, True, True), ("general kernel (200, 100)", 200, 100, True, True),
        ("general kernel (256, 100)", 256, 100, True, True), ("general kernel (50, 20)", 50, 20, True, True),
        ("stock kernel (50, 100), Predict only", 50, 100, False, False),
        ("general kernel (50, 100), Predict only", 50, 100, True, False)]


def make_leg(gmix_amd, lsc, label, cells, horizon, general, learn, S, ppm, data):
    shape = (cells, horizon, 0.03, 10.0)
    old = os.environ.get("GMX_LSTM_BUILD")
    if general:
        os.environ["GMX_LSTM_BUILD"] = "any"     # (only matters at the stock shape)
    else:
        os.environ.pop("GMX_LSTM_BUILD", None)
    try:
        g = gmix_amd.LstmGroup(S, shape=shape)
    finally:
        if old is None:
            os.environ.pop("GMX_LSTM_BUILD", None)
        else:
            os.environ["GMX_LSTM_BUILD"] = old
    w = lsc.Ref(shape, seed=0xDEADBEEF).weights()
    for s in range(S):
        g.set_weights(w, stream=s)
    N = horizon                                   # one backward pass per launch
    b = gmix_amd.LstmBatch(g, N)
    rng = np.random.default_rng(0)
    for s in range(S):
        b.ppm[s] = ppm[:N]
        b.bytes[s] = np.roll(data[:N], int(rng.integers(0, N)))
    b.upload(N)
    return dict(label=label, shape=shape, general=general, learn=learn, g=g, b=b, N=N, ms=[])


def host_rate(lsc, shape, ppm, data, n):
    r = lsc.Ref(shape, seed=0xDEADBEEF)
    t0 = time.perf_counter()
    r.run(ppm[:n], data[:n])
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="256,1024")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_shape_bench.json"))
    a = ap.parse_args()
    import gmix_amd
    from gmix_amd import synth
    import lstm_shape_common as lsc
    assert gmix_amd.device_count() > 0, "no GPU: nothing is measured"
    ppm, data = synth.lstm_records(200, seed=1, mask=63)
    rows = []
    for S in [int(x) for x in a.streams.split(",")]:
        legs = [make_leg(gmix_amd, lsc, *leg, S, ppm, data) for leg in LEGS]
        for leg in legs:                          # warm-up at the timed size
            leg["g"].run(leg["b"], leg["N"], learn=leg["learn"])
            leg["g"].sync()
        for _ in range(a.rounds):
            for leg in legs:
                leg["ms"].append(leg["g"].run(leg["b"], leg["N"], learn=leg["learn"], timed=True))
        for leg in legs:
            ms = sorted(leg["ms"])
            med = ms[len(ms) // 2]
            rows.append({"streams": S, "leg": leg["label"], "num_cells": leg["shape"][0], "horizon": leg["shape"][1],
                         "learn": leg["learn"],
                         "kernel": "gmx_lstm_any_kernel" if leg["general"] else "gmx_lstm_kernel",
                         "general_launches": leg["g"].any_launches, "bytes_per_launch": S * leg["N"],
                         "kernel_ms": {"median": med, "min": ms[0], "max": ms[-1], "rounds": len(ms)},
                         "bytes_per_s": S * leg["N"] / (med * 1e-3),
                         "bytes_per_s_spread": [S * leg["N"] / (ms[-1] * 1e-3), S * leg["N"] / (ms[0] * 1e-3)],
                         "bank_bytes_per_stream": leg["g"].bank_bytes})
            leg["b"].close()
            leg["g"].close()
    host = {}
    for label, cells, horizon, _, _ in LEGS:
        shape = (cells, horizon, 0.03, 10.0)
        if (cells, horizon) not in host:
            host[(cells, horizon)] = host_rate(lsc, shape, ppm, data, 2 * horizon)
    for r in rows:
        r["host_restatement_one_core_bytes_per_s"] = host[(r["num_cells"], r["horizon"])]
    ratio = {}
    for S in sorted({r["streams"] for r in rows}):
        st = [r for r in rows if r["streams"] == S and r["leg"] == "stock kernel (50, 100)"][0]
        ge = [r for r in rows if r["streams"] == S and r["leg"] == "general kernel (50, 100)"][0]
        ratio[str(S)] = ge["bytes_per_s"] / st["bytes_per_s"]
    out = {"what": "LSTM byte model, Predict x 8 bits + Learn, one backward pass per launch; kernel time from device events",
           "build": gmix_amd._lib.lib().gmx_build_info().decode(), "rounds": a.rounds, "rows": rows,
           "general_over_stock_at_50_100": ratio,
           "host_note": "tests/lstm_shape_ref.c (the plain-C restatement, gcc -O2), one core of the benchmark host; "
                        "not the reference's own build"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for r in rows:
        print(f'{r["streams"]:5d} {r["leg"]:40s} {r["bytes_per_s"]:12.4g} bytes/s  [{r["bytes_per_s_spread"][0]:.4g}, '
              f'{r["bytes_per_s_spread"][1]:.4g}]  host 1 core {r["host_restatement_one_core_bytes_per_s"]:.4g}')
    print(json.dumps({"general_over_stock_at_50_100": ratio}))


if __name__ == "__main__":
    main()
