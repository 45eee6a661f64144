#!/usr/bin/env python3
"""Per-bit latency of the stock chain with the Match models riding in the session wave, one stream, by where the
context variables come from:

  a  gmx_chain_forward_match on context words computed beforehand            (the floor: the host's contexts cost nothing)
  b  the same, tests/helpers/ctx_ref.c computing the 52 variables of every bit inside the loop and the host filling
     the three record sets from them                                          (what a caller without the bank does)
  c  gmx_chain_forward_ctx: the variables step in the session wave, the host sends the coded bit alone

    python scripts/bench_chain_ctx.py --out profiles/chain_ctx_latency.json

One process, one set of banks (52 stock context variables, 6 stock Match models, 41 stock Indirect models, stock
mixers).  The legs alternate: ROUNDS rounds of a, b, c, each leg WARMUP untimed bits and then BITS bits with the host's
clock around them (a synchronise of all banks inside the clock); the stream goes on from leg to leg, the context bank
and ctx_ref.c being brought to a leg's first bit outside the clock (gmx_ctx_run / cref_run).  For a and b the context
bank is detached, so their waves are the build without the context phase.  The calls are made through ctypes on arrays
prepared beforehand; the interpreter's own cost per call is in every figure.  Reported per leg: the median over the
rounds and (max - min) / median, in microseconds per bit."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WARMUP, BITS, ROUNDS = 1000, 4000, 3
MSLOTS = [2, 3, 4, 5, 6, 7]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_ctx_latency.json"))
    a = ap.parse_args()
    import numpy as np
    import ctx_common as cc
    import gmix_amd
    from gmix_amd import topology
    from gmix_amd.ctx import desc_array
    from gmix_amd.match import match_stream

    named, mroute, iroute, xroute = topology.stock_contexts()
    arr = desc_array(named)
    descs = [arr[i] for i in range(len(named))]
    V, bcv = len(descs), [n for n, _, _ in named].index("bit_context")
    T = ROUNDS * 3 * (WARMUP + BITS)
    data = match_stream(9, T // 8 + 1)
    bits = np.ascontiguousarray(np.unpackbits(data)[:T])
    vals = cc.Ref(descs).run(bits)          # leg a's words, and the check of leg c's
    zi = np.load(os.path.join(ROOT, "tests", "golden", "ind_stock41.npz"))
    imodels = topology.stock_indirect()
    KI, KM, N, M = len(imodels), len(MSLOTS), 90, 33
    cols = topology.stock_longest_match_columns()
    ig = gmix_amd.IndirectGroup(imodels, zi["ns_next"], zi["rm_next"], 1, slots=[(8 + 2 * i, 9 + 2 * i) for i in range(KI)])
    mg = gmix_amd.MixerGroup(topology.stock(90), 1)
    mt = gmix_amd.MatchGroup([(t, topology.STOCK_MATCH_LIMIT, s) for (_, t), s in zip(topology.STOCK_MATCH, MSLOTS)],
                             len(data) + 64, 1)
    cg = gmix_amd.CtxGroup(named, 1)
    cb = gmix_amd.CtxBatch(cg, 3 * (WARMUP + BITS), values=False)
    ig.attach_match(mt, cols)
    ref = cc.Ref(descs)                     # leg b's
    ir, xr, mr = np.array(iroute), np.array(xroute), np.array(mroute)

    def merged(route, base):
        out = np.ascontiguousarray(np.broadcast_to(base, (T, len(route))), np.uint32).copy()
        on = route >= 0
        out[:, on] = vals[:, route[on]]
        return out

    ictx, xctx, mctx = merged(ir, np.uint32(7)), merged(xr, np.uint32(0)), merged(mr, np.uint32(0))
    rng = np.random.default_rng(5)
    pred = np.ascontiguousarray(rng.normal(0, 2, N), np.float32)
    host_active = np.array([0, 1], np.int32)
    L, vp = ig.L, C.c_void_p
    p, lm, bc_out = C.c_float(), C.c_uint32(), C.c_uint32()
    out, ip, ia = np.zeros(M, np.float32), np.zeros(2 * KI, np.float32), np.zeros(2 * KI, np.uint8)
    mp, ma = np.zeros(KM, np.float32), np.zeros(KM, np.uint8)
    ic_b, xc_b, mc_b = np.full(KI, 7, np.uint32), np.zeros(KM, np.uint32), np.zeros(M, np.uint32)
    v1, b1 = np.zeros((1, V), np.uint32), np.zeros(1, np.uint8)
    A = lambda x: x.ctypes.data_as(vp)
    a_pred, a_act, a_out, a_ip, a_ia, a_mp, a_ma = A(pred), A(host_active), A(out), A(ip), A(ia), A(mp), A(ma)
    a_icb, a_xcb, a_mcb, a_v1, a_b1 = A(ic_b), A(xc_b), A(mc_b), A(v1), A(b1)
    rows_i = [ictx[t].ctypes.data_as(vp) for t in range(T)]
    rows_x = [xctx[t].ctypes.data_as(vp) for t in range(T)]
    rows_m = [mctx[t].ctypes.data_as(vp) for t in range(T)]
    bcs, bs = [int(v) for v in vals[:, bcv]], [int(v) for v in bits]
    ih, gh, mh, ch, rh = ig.h, mg.h, mt.h, cg.h, ref.h
    pp, plm, pbc = C.byref(p), C.byref(lm), C.byref(bc_out)
    ion, xon, mon = ir >= 0, xr >= 0, mr >= 0
    irv, xrv, mrv = ir[ion], xr[xon], mr[mon]
    cref_run = ref.L.cref_run

    def bit(leg, t):
        if leg == "a":
            rc = L.gmx_chain_forward_match(ih, gh, 0, rows_i[t], rows_x[t], bcs[t], a_pred, a_act, 2, rows_m[t], pp,
                                           a_out, a_ip, a_ia, a_mp, a_ma, plm)
        elif leg == "b":
            b1[0] = bs[t]
            cref_run(rh, 1, a_b1, a_v1)    # (ctx_ref.c codes the bit as it computes the values of its Predict)
            row = v1[0]
            ic_b[ion], xc_b[xon], mc_b[mon] = row[irv], row[xrv], row[mrv]
            rc = L.gmx_chain_forward_match(ih, gh, 0, a_icb, a_xcb, int(row[bcv]), a_pred, a_act, 2, a_mcb, pp, a_out,
                                           a_ip, a_ia, a_mp, a_ma, plm)
        else:
            rc = L.gmx_chain_forward_ctx(ih, gh, 0, a_icb, None, a_pred, a_act, 2, a_mcb, pp, a_out, a_ip, a_ia, a_mp,
                                         a_ma, plm, None, pbc)
            rc |= L.gmx_ctx_learn(ch, 0, bs[t])
        rc |= L.gmx_indirect_learn(ih, 0, bs[t])
        rc |= L.gmx_bank_learn(gh, 0, bs[t])
        rc |= L.gmx_match_learn(mh, 0, bs[t])
        if rc:
            raise RuntimeError("leg %s bit %d: status %d" % (leg, t, rc))

    us = dict(a=[], b=[], c=[])
    t, at_dev, at_ref = 0, 0, 0
    for _ in range(ROUNDS):
        for leg in "abc":
            if leg == "c":                  # the bank to the leg's first bit, and into the waves
                if t > at_dev:
                    cb.bits[0, :t - at_dev] = bits[at_dev:t]
                    cb.upload(t - at_dev)
                    cg.run(cb, t - at_dev)
                    cg.sync()
                ig.attach_ctx(cg, mroute, iroute, xroute)
            elif leg == "b" and t > at_ref:
                ref.run(bits[at_ref:t], values=False)
            for _ in range(WARMUP):
                bit(leg, t)
                t += 1
            t0 = time.perf_counter()
            for _ in range(BITS):
                bit(leg, t)
                t += 1
            for x in (ig, mg, mt, cg):
                x.sync()
            us[leg].append((time.perf_counter() - t0) * 1e6 / BITS)
            if leg == "c":
                assert bc_out.value == bcs[t - 1], "the bank is not where ctx_ref.c is"
                ig.attach_ctx(None)
                at_dev = t
            elif leg == "b":
                at_ref = t
    res = {}
    for leg, v in us.items():
        med = sorted(v)[len(v) // 2]
        res[leg] = dict(us_per_bit=v, median_us=med, spread=(max(v) - min(v)) / med)
        print(leg, "%.2f us/bit (spread %.1f%%)" % (med, 100 * res[leg]["spread"]), flush=True)
    doc = dict(setup=dict(shape="stock: 52 context variables, 6 Match, 41 Indirect, 33 mixers of 90 inputs", streams=1,
                          warmup_bits=WARMUP, bits_per_leg=BITS, rounds=ROUNDS,
                          legs=dict(a="gmx_chain_forward_match, contexts precomputed",
                                    b="gmx_chain_forward_match, ctx_ref.c inside the loop",
                                    c="gmx_chain_forward_ctx"),
                          clock="host, around each leg of a round; us per bit; median and (max-min)/median"),
               result=res, build=gmix_amd.build_info() if hasattr(gmix_amd, "build_info") else "")
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
