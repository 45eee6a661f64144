#!/usr/bin/env python3
"""What the Match lanes add to one lock-step step of the stock chain (gmx_chainstep: LSTM byte model, 41 Indirect
models, 33 mixers; scripts/bench_chainstep.py's records over the Match fixtures' stream generator): gmx_chainstep_step
by the host's clock at 64 and 256 streams, WITHOUT a Match bank (the step as it was: the six Match slots come in the
caller's records) and WITH one attached (gmx_chainstep_attach_match: lanes 56..63 of the Indirect models' launch).
The two are measured in the same process, in alternation, `--rounds` times each on fresh banks; a round's figure is
the median over its steps after `--warmup` of them, the reported delta the median of the rounds' differences, its
spread their range.  A separate launch is known to cost a step 4.5 us: `fused_pays_off` says
whether the delta, less the spread, stays below that.  Writes profiles/chainstep_match.json.

The device-side timeline of either configuration: run one of them alone under the profiler, as
scripts/trace_chainstep.sh does for scripts/bench_chainstep.py --
    rocprofv3 --kernel-trace --output-format csv -d out -- python3 scripts/bench_chainstep_match.py --only attached \\
        --streams 64 --rounds 1 --steps 1000

    python scripts/bench_chainstep_match.py [--streams 64 256] [--steps 3000] [--warmup 500] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gmix_amd  # noqa: E402
from gmix_amd import topology  # noqa: E402
from gmix_amd.match import match_stream, stream_bits  # noqa: E402
from bench_match import stock_contexts  # noqa: E402

SEPARATE_LAUNCH_US = 4.5
MATCH_SLOTS = [2, 3, 4, 5, 6, 7]   # the host-side models' slots of bench_chainstep.py that are the Match models'
MATCH_COLS = [6, 30]               # the gate contexts that are longest_match (predictor.cpp)


def one_run(S, steps, warmup, attached, streams, z, w0, seed):
    """steps + 1 lock-step steps on fresh banks -> microseconds of every gmx_chainstep_step after the warm-up."""
    K = 41
    slots = [(8 + 2 * i, 9 + 2 * i) for i in range(K)]
    lg = gmix_amd.LstmGroup(S)
    ig = gmix_amd.IndirectGroup(topology.stock_indirect(), z["ns_next"], z["rm_next"], S, slots=slots)
    mg = gmix_amd.MixerGroup(topology.stock(90), S)
    for s in range(S):
        lg.set_weights(w0, stream=s)
    cs = gmix_amd.ChainStep(mg, ig, lg, lstm_slot=1, mixer_ctx_col=22, ind_ctx_col=16)
    mt = None
    if attached:
        mt = gmix_amd.MatchGroup([(t, l, sl) for (t, l, _), sl in zip(topology.stock_match(), MATCH_SLOTS)],
                                 steps // 8 + 64, S)
        cs.attach_match(mt, MATCH_COLS)
    rng = np.random.default_rng(seed)
    cs.predictions[:, :90] = rng.standard_normal((S, 90)).astype(np.float32)
    cs.active_mask[:] = 0
    cs.active_mask[:, 0] = 0x01 if attached else 0xfd  # the host-side models' slots; the device-side models set their own
    ppm = rng.random((S, 256), dtype=np.float32)
    ppm /= ppm.sum(axis=1, keepdims=True)
    mctx, bc, bits = streams  # [S][T][6], [S][T], [S][T]
    us = []
    for t in range(steps + 1):
        i = min(t, steps - 1)
        if t % 8 == 0:
            byte_ctx = rng.integers(0, 1 << 16, (S, 33), dtype=np.uint32)
            ind_ctx = rng.integers(0, 1 << 24, (S, K), dtype=np.uint32)
            cs.ppm[:] = ppm
            if attached:
                cs.match_contexts[:] = mctx[:, i]
        ctx = byte_ctx.copy()
        ctx[:, (2, 11, 26, 29)] = (byte_ctx[:, (2, 11, 26, 29)] << 8) | (bc[:, i, None] + 1)  # the bit-level gate contexts
        cs.contexts[:] = ctx
        cs.ind_contexts[:] = ind_ctx
        cs.bit_contexts[:] = bc[:, i]
        if t > 0:
            cs.bits[:] = bits[:, t - 1]
        cs.what[:] = (1 if t > 0 else 0) | (2 if t < steps else 0)
        t0 = time.perf_counter()
        cs.step()
        if t >= warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    cs.close()
    for h in (mt, lg, ig, mg):
        if h:
            h.close()
    return np.asarray(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["base", "attached"], default=None, help="one configuration (for a profiler)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chainstep_match.json"))
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "ind_stock41.npz"))
    w0 = ((np.random.default_rng(1).random((3, 50, 563), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
    distinct = 16
    recs = []
    for i in range(distinct):
        d = match_stream(2000 + i, a.steps // 8 + 1)
        b, bc = stream_bits(d)
        recs.append((np.repeat(stock_contexts(d), 8, axis=0), bc, b))
    res = {"build": gmix_amd._lib.lib().gmx_build_info().decode(), "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "separate_launch_us": SEPARATE_LAUNCH_US, "runs": []}
    for S in a.streams:
        streams = tuple(np.stack([recs[s % distinct][j][:a.steps] for s in range(S)]) for j in range(3))
        base, att = [], []
        for r in range(a.rounds):
            for attached in ((False, True) if r % 2 == 0 else (True, False)):  # alternated, the order too
                if a.only and (a.only == "attached") != attached:
                    continue
                us = one_run(S, a.steps, a.warmup, attached, streams, z, w0, 10 + r)
                (att if attached else base).append(float(np.median(us)))
        row = {"streams": S, "base_us_per_step": base, "attached_us_per_step": att}
        if base and att:
            d = np.asarray(att) - np.asarray(base)
            row.update(delta_us=float(np.median(d)), delta_spread_us=float(d.max() - d.min()),
                       base_spread_us=float(max(base) - min(base)),
                       fused_pays_off=bool(np.median(d) - (d.max() - d.min()) <= SEPARATE_LAUNCH_US))
        res["runs"].append(row)
    if not a.only:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
