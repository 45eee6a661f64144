#!/usr/bin/env python3
"""Throughput of the context banks' launch (gmx_ctx.hip): the stock bank, --streams x --bits per launch, all three
targets attached (the mixers', the Indirect models' and the Match models' record batches), HIP events around the launch
and between its kernels.  Beside it tests/helpers/ctx_ref.c on one host core over the same bits: our restatement, not
the reference's binary.  Writes profiles/ctx_bench.json.

    python scripts/bench_ctx.py [--streams 64 256] [--bits 2048]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gmix_amd  # noqa: E402
from gmix_amd import topology  # noqa: E402
from gmix_amd.match import match_stream  # noqa: E402

# what the host writes into the three record arrays per stream-bit today: 4 * 33 gate contexts, 4 * 41 + 4 + 1 for the
# Indirect models, 4 * 6 + 4 + 1 for the Match models
BYTES_PER_STREAM_BIT = 4 * 33 + (4 * 41 + 4 + 1) + (4 * 6 + 4 + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--bits", type=int, default=2048)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctx_bench.json"))
    a = ap.parse_args()
    import ctx_common as cc
    import goldenlib
    rounds = a.warmup + a.launches
    nb = a.bits * rounds // 8 + 1
    distinct = 16
    bits = [np.unpackbits(match_stream(1000 + i, nb)) for i in range(distinct)]
    descs, mixer_route, ind_route, match_route = topology.stock_contexts()
    assert BYTES_PER_STREAM_BIT == 330
    _, z = goldenlib.load("ind_stock41")
    res = {"build": gmix_amd._lib.lib().gmx_build_info().decode(), "bits_per_launch": a.bits,
           "launches": a.launches, "warmup": a.warmup, "record_bytes_per_stream_bit": BYTES_PER_STREAM_BIT,
           "device": []}
    for S in a.streams:
        g = gmix_amd.CtxGroup(descs, S)
        b = gmix_amd.CtxBatch(g, a.bits, values=False)
        mg = gmix_amd.MixerGroup(topology.stock(90), S)
        # the targets are record batches: their shapes are the stock ones (33, 41 and 6 columns), the banks that own
        # them are built with 256-entry tables so that 256 streams of them fit beside 256 x 201 MB of hash tables
        ig = gmix_amd.IndirectGroup([(256, lr) for _, lr in topology.stock_indirect()], z["ns_next"], z["rm_next"], S)
        xg = gmix_amd.MatchGroup([(256, lim, slot) for _, lim, slot in topology.stock_match()], 1024, S)
        mb, ib, xb = gmix_amd.Batch(mg, a.bits), gmix_amd.IndirectBatch(ig, a.bits), gmix_amd.MatchBatch(xg, a.bits)
        tg = g.targets(mixers=mb, mixer_route=mixer_route, indirect=ib, ind_route=ind_route, match=xb,
                       match_route=match_route)
        ms, parts = [], []
        for r in range(rounds):
            t0 = r * a.bits
            for s in range(S):
                b.bits[s, :a.bits] = bits[s % distinct][t0:t0 + a.bits]
            b.upload(a.bits)
            b.wait()
            t = g.run(b, a.bits, targets=tg, timed=True)
            if r >= a.warmup:
                ms.append(t)
                parts.append(g.last_kernel_ms())
        med = float(np.median(ms))
        chain, expand, commit = (float(np.median([p[i] for p in parts])) for i in range(3))
        sb = S * a.bits
        res["device"].append({
            "streams": S, "launch_ms_median": med, "launch_ms_min": float(min(ms)), "launch_ms_max": float(max(ms)),
            "chain_kernel_ms": chain, "expand_kernel_ms": expand, "commit_kernel_ms": commit,
            "stream_bits_per_s": sb / (med * 1e-3), "us_per_stream_bit": med * 1e3 / sb,
            "chain_stream_bits_per_s": sb / (chain * 1e-3), "expand_stream_bits_per_s": sb / (expand * 1e-3),
            "record_bytes_per_s": sb * BYTES_PER_STREAM_BIT / (med * 1e-3),
            "expand_record_bytes_per_s": sb * BYTES_PER_STREAM_BIT / (expand * 1e-3),
            "device_bytes_per_stream": int(g.bank_bytes)})
        for x in (b, mb, ib, xb, g, mg, ig, xg):
            x.close()
    # our restatement on one host core over the bits of one stream
    f = cc.fixture("ctx_stock")
    ref = cc.Ref(f.descs)
    n = a.bits * rounds
    t0 = time.perf_counter()
    ref.run(bits[0][:n], values=True)
    dt = time.perf_counter() - t0
    res["host_restatement_one_core"] = {"what": "tests/helpers/ctx_ref.c (gcc -O2), not the reference's binary",
                                        "bits": n, "us_per_stream_bit": dt * 1e6 / n}
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
