#!/usr/bin/env python3
"""What stepping the context variables on the device does to one lock-step step of the stock chain (gmx_chainstep: LSTM
byte model, 41 Indirect models, six Match models attached, 33 mixers): once with the HOST filling every context column,
the Match models' context words and the bit context -- the step as it was, through the same binary without attach --
and once with a stock context bank ATTACHED (gmx_chainstep_attach_ctx: gmx_ctx_step_kernel at the head of every step,
0xFFFFFFFF in every routed place).  Per configuration and stream count:

  wall_us_per_step     gmx_chainstep_step by the host's clock (the posted writes of the records are inside it: nobody
                       commits beforehand); what the host spends on COMPUTING the contexts is outside it in both modes
  device_us_per_step   HIP events around the step's graph (gmx_chainstep_timed_step), in passes of their own
  commit_bytes         bytes of records per stream a commit moves (gmx_chainstep_commit_bytes)

The two configurations run in the same process, in alternation, `--rounds` times each on fresh banks; a round's figure is
the median over its steps after `--warmup` of them, the reported figure the median of the rounds, with their range.  The
Indirect and the Match bank use 256-entry tables so that 256 streams of them fit beside 256 x 201 MB of hash tables
(scripts/bench_ctx.py does the same).  No threshold is attached to these numbers.  Writes
profiles/chainstep_ctx_bench.json.

    python scripts/bench_chainstep_ctx.py [--streams 64 256] [--steps 2000] [--warmup 400] [--rounds 3]
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

K = 41
IND_SLOTS = [(8 + 2 * i, 9 + 2 * i) for i in range(K)]
MATCH_SLOTS = [2, 3, 4, 5, 6, 7]
LSTM_SLOT, MIX_LSTM_COL, IND_LSTM_COL = 1, 22, 16
FILL = 0xFFFFFFFF


def one_run(S, steps, warmup, attached, timed, recs, z, w0, seed):
    """steps + 1 lock-step steps on fresh banks -> microseconds of every step after the warm-up (wall, or device when
    `timed`), and the bytes a commit moves."""
    descs, mixer_route, ind_route, match_route = topology.stock_contexts()
    cols = topology.stock_longest_match_columns()
    lg = gmix_amd.LstmGroup(S)
    ig = gmix_amd.IndirectGroup([(256, lr) for _, lr in topology.stock_indirect()], z["ns_next"], z["rm_next"], S,
                                slots=IND_SLOTS)
    mg = gmix_amd.MixerGroup(topology.stock(90), S)
    xg = gmix_amd.MatchGroup([(256, lim, sl) for (_, lim, _), sl in zip(topology.stock_match(), MATCH_SLOTS)],
                             steps // 8 + 64, S)
    for s in range(S):
        lg.set_weights(w0, stream=s)
    cs = gmix_amd.ChainStep(mg, ig, lg, lstm_slot=LSTM_SLOT, mixer_ctx_col=MIX_LSTM_COL, ind_ctx_col=IND_LSTM_COL)
    cs.attach_match(xg, cols)
    cg = None
    if attached:
        cg = gmix_amd.CtxGroup(descs, S)
        cs.attach_ctx(cg, mixer_route, ind_route, match_route)
    commit_bytes = cs.commit_bytes
    rng = np.random.default_rng(seed)
    cs.predictions[:, :90] = rng.standard_normal((S, 90)).astype(np.float32)
    cs.active_mask[:] = 0
    cs.active_mask[:, 0] = 0x01   # the host-side model's slot; the device-side models set their own
    ppm = rng.random((S, 256), dtype=np.float32)
    ppm /= ppm.sum(axis=1, keepdims=True)
    bits, mctx, ictx, xctx, bc = recs   # [S][T], [S][T][33], [S][T][41], [S][T][6], [S][T]
    if attached:
        cs.contexts[:] = FILL
        cs.ind_contexts[:] = FILL
        cs.match_contexts[:] = FILL
        cs.bit_contexts[:] = FILL
    us = []
    for t in range(steps + 1):
        i = min(t, steps - 1)
        if t % 8 == 0:
            cs.ppm[:] = ppm
        if not attached:
            cs.contexts[:] = mctx[:, i]
            cs.ind_contexts[:] = ictx[:, i]
            cs.match_contexts[:] = xctx[:, i]
            cs.bit_contexts[:] = bc[:, i]
        if t > 0:
            cs.bits[:] = bits[:, t - 1]
        cs.what[:] = (1 if t > 0 else 0) | (2 if t < steps else 0)
        if timed:
            v = cs.timed_step() * 1e3
        else:
            t0 = time.perf_counter()
            cs.step()
            v = (time.perf_counter() - t0) * 1e6
        if t >= warmup:
            us.append(v)
    cs.close()
    for h in (cg, xg, lg, ig, mg):
        if h:
            h.close()
    return np.asarray(us), commit_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chainstep_ctx_bench.json"))
    a = ap.parse_args()
    import ctx_common as cc
    z = np.load(os.path.join(ROOT, "tests", "golden", "ind_stock41.npz"))
    w0 = ((np.random.default_rng(1).random((3, 50, 563), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
    descs, mixer_route, ind_route, match_route = topology.stock_contexts()
    f = cc.fixture("ctx_stock")
    assert [d[0] for d in descs] == f.names
    bcv = f.names.index("bit_context")

    def cols(route, v):   # the columns other banks write hold 0 in the host's records
        r = np.asarray(route)
        return np.where(r[None, :] >= 0, v[:, np.maximum(r, 0)], 0).astype(np.uint32)
    distinct, per = 16, []
    for i in range(distinct):
        b = np.unpackbits(match_stream(3000 + i, a.steps // 8 + 1))[:a.steps]
        v = cc.Ref(f.descs).run(b)   # what the host computes per stream-bit today (tests/helpers/ctx_ref.c)
        per.append((b, cols(mixer_route, v), cols(ind_route, v), cols(match_route, v), v[:, bcv].copy()))
    res = {"build": gmix_amd._lib.lib().gmx_build_info().decode(), "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "runs": []}
    for S in a.streams:
        recs = tuple(np.stack([per[s % distinct][j] for s in range(S)]) for j in range(5))
        row = {"streams": S}
        got = {(m, k): [] for m in ("host", "attached") for k in ("wall", "device")}
        for r in range(a.rounds):
            for attached in ((False, True) if r % 2 == 0 else (True, False)):   # alternated, the order too
                for timed in (False, True):
                    us, cb = one_run(S, a.steps, a.warmup, attached, timed, recs, z, w0, 10 + r)
                    got[("attached" if attached else "host", "device" if timed else "wall")].append(float(np.median(us)))
                    row[("attached" if attached else "host") + "_commit_bytes_per_stream"] = cb
        for (m, k), v in got.items():
            row[f"{m}_{k}_us_per_step"] = float(np.median(v))
            row[f"{m}_{k}_us_rounds"] = v
        row["wall_delta_us"] = row["attached_wall_us_per_step"] - row["host_wall_us_per_step"]
        row["device_delta_us"] = row["attached_device_us_per_step"] - row["host_device_us_per_step"]
        res["runs"].append(row)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
