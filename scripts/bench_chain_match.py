#!/usr/bin/env python3
"""Per-bit latency of the full chain Match -> Indirect -> mixers of the stock shape, one stream, three routes:

  a  gmx_chain_forward alone + gmx_indirect_learn + gmx_bank_learn           (no Match models: the floor)
  b  gmx_match_forward + gmx_chain_forward + the three learns                (the Match models a launch per call)
  c  gmx_chain_forward_match + the three learns                              (the Match models in the session wave)

    python scripts/bench_chain_match.py --label new --out profiles/chain_match_latency.json
    python scripts/bench_chain_match.py --label parent --routes a,b --tree <checkout of the parent commit> --out ...

One fresh child process per route (never two at a time).  A child builds the six stock Match models, the 41 stock
Indirect models and the stock mixers for ONE stream, brings the Match bank to bit 3 000 of tests/golden/match_stock.npz
with gmx_match_run, runs 2 000 warm-up bits of Predict + Learn through its route, and then three repeats of 20 000 bits
with the host's clock around each repeat (a synchronise of all three banks inside the clock).  The calls are made
through ctypes on arrays prepared beforehand; the interpreter's own cost per call (about a microsecond) is in every
figure, and route b makes one call more per bit than the others.  Reported: the median of the three repeats and
(max - min) / median, in microseconds per bit.  --label selects the entry of the output file that is written; the
other entries are kept, so the parent commit's figures and this commit's stand side by side."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, BITS, REPEATS, START = 2000, 20000, 3, 3000
MSLOTS, COLS = [2, 3, 4, 5, 6, 7], [6, 30]


def child(route, tree):
    sys.path.insert(0, tree)
    import numpy as np
    import gmix_amd
    from gmix_amd import topology
    from gmix_amd.match import stream_bits
    z = np.load(os.path.join(ROOT, "tests", "golden", "match_stock.npz"))
    zi = np.load(os.path.join(ROOT, "tests", "golden", "ind_stock41.npz"))
    data = z["data"]
    bits, bc = stream_bits(data)
    ctx = np.ascontiguousarray(np.repeat(z["ctx_bytes"], 8, axis=0), np.uint32)
    tables, limit = [int(t) for t in z["tables"]], int(z["limit"])
    T = START + WARMUP + REPEATS * BITS
    assert T <= len(bits)
    imodels = topology.stock_indirect()
    KI, KM, N, M = len(imodels), len(tables), 90, 33
    ig = gmix_amd.IndirectGroup(imodels, zi["ns_next"], zi["rm_next"], 1, slots=[(8 + 2 * i, 9 + 2 * i) for i in range(KI)])
    mg = gmix_amd.MixerGroup(topology.stock(90), 1)
    mt = gmix_amd.MatchGroup([(t, limit, s) for t, s in zip(tables, MSLOTS)], len(data) + 64, 1)
    b = gmix_amd.MatchBatch(mt, START)
    b.set_records(0, ctx[:START], bc[:START], bits[:START])
    b.upload()
    mt.run(b, START)
    mt.sync()
    if route == "c":
        ig.attach_match(mt, COLS)
    rng = np.random.default_rng(5)
    ictx = np.ascontiguousarray(np.repeat(rng.integers(0, 1 << 22, (T // 8 + 1, KI)), 8, axis=0)[:T], np.uint32)
    mctx = np.ascontiguousarray(np.repeat(rng.integers(0, 1 << 16, (T // 8 + 1, M)), 8, axis=0)[:T], np.uint32)
    pred = np.ascontiguousarray(rng.normal(0, 2, N), np.float32)
    host_active = np.array([0, 1], np.int32)
    L = ig.L
    vp = C.c_void_p
    p, lm = C.c_float(), C.c_uint32()
    out, ip, ia = np.zeros(M, np.float32), np.zeros(2 * KI, np.float32), np.zeros(2 * KI, np.uint8)
    mp, ma = np.zeros(KM, np.float32), np.zeros(KM, np.uint8)
    pr2, cx2, act2 = pred.copy(), np.zeros(M, np.uint32), np.zeros(N, np.int32)
    A = lambda a: a.ctypes.data_as(vp)
    a_pred, a_act, a_out, a_ip, a_ia, a_mp, a_ma = A(pred), A(host_active), A(out), A(ip), A(ia), A(mp), A(ma)
    a_pr2, a_cx2, a_act2 = A(pr2), A(cx2), A(act2)
    rows_i = [ictx[t].ctypes.data_as(vp) for t in range(T)]
    rows_m = [ctx[t].ctypes.data_as(vp) for t in range(T)]
    rows_x = [mctx[t].ctypes.data_as(vp) for t in range(T)]
    bcs, bs = [int(v) for v in bc[:T]], [int(v) for v in bits[:T]]
    ih, gh, mh = ig.h, mg.h, mt.h
    pp, plm = C.byref(p), C.byref(lm)

    def bit(t):
        if route == "a":
            rc = L.gmx_chain_forward(ih, gh, 0, rows_i[t], bcs[t], a_pred, a_act, 2, rows_x[t], pp, a_out, a_ip, a_ia)
        elif route == "b":
            rc = L.gmx_match_forward(mh, 0, rows_m[t], bcs[t], a_mp, a_ma, plm)
            pr2[MSLOTS] = mp   # what a caller of the two calls does between them
            on = [0, 1] + [s for s, f in zip(MSLOTS, ma) if f]
            act2[:len(on)] = on
            cx2[:] = mctx[t]
            cx2[COLS] = lm.value
            rc |= L.gmx_chain_forward(ih, gh, 0, rows_i[t], bcs[t], a_pr2, a_act2, len(on), a_cx2, pp, a_out, a_ip, a_ia)
        else:
            rc = L.gmx_chain_forward_match(ih, gh, 0, rows_i[t], rows_m[t], bcs[t], a_pred, a_act, 2, rows_x[t], pp,
                                           a_out, a_ip, a_ia, a_mp, a_ma, plm)
        rc |= L.gmx_indirect_learn(ih, 0, bs[t])
        rc |= L.gmx_bank_learn(gh, 0, bs[t])
        if route != "a":
            rc |= L.gmx_match_learn(mh, 0, bs[t])
        if rc:
            raise RuntimeError("bit %d: status %d" % (t, rc))

    t = START
    for _ in range(WARMUP):
        bit(t)
        t += 1
    us = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(BITS):
            bit(t)
            t += 1
        ig.sync()
        mg.sync()
        mt.sync()
        us.append((time.perf_counter() - t0) * 1e6 / BITS)
    med = sorted(us)[len(us) // 2]
    print(json.dumps(dict(route=route, us_per_bit=us, median_us=med, spread=(max(us) - min(us)) / med,
                          p_last=float(p.value), build=gmix_amd.build_info() if hasattr(gmix_amd, "build_info") else "")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_match_latency.json"))
    ap.add_argument("--label", default="new")
    ap.add_argument("--routes", default="a,b,c")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose gmix_amd package (and built library) is measured")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.tree)
        return
    res = {}
    for route in a.routes.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", route, "--tree", a.tree],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("route %s failed (status %d): nothing more is started" % (route, r.returncode))
        res[route] = json.loads(r.stdout.strip().splitlines()[-1])
        print(route, "%.2f us/bit (spread %.1f%%)" % (res[route]["median_us"], 100 * res[route]["spread"]), flush=True)
    doc = {}
    if os.path.exists(a.out):
        doc = json.load(open(a.out))
    doc.setdefault("setup", dict(shape="stock: 6 Match, 41 Indirect, 33 mixers of 90 inputs", streams=1, start_bit=START,
                                 warmup_bits=WARMUP, bits_per_repeat=BITS, repeats=REPEATS,
                                 clock="host, around each repeat; us per bit; median and (max-min)/median"))
    doc[a.label] = res
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
