#!/usr/bin/env python3
"""Times gmx_group_run on shapes outside the three literal ones, through the default route and -- where the
library has gmx_group_set_register_rows -- through the register-resident kernel for any three-layer bank
(gmix_amd/csrc/gmx_pair.hip).  HIP events around the kernel (kernel_ms), records generated on the device
(gmx_batch_fill_synthetic), warm-up launches first, the median of the timed launches.

    python scripts/bench_pair.py --out profiles/pair_bench.json            # this tree
    python scripts/bench_pair.py --tree <checkout of the parent commit> --label parent --out ...   # a baseline

A tree without the switch times its default route only.  --out merges into an existing file under --label, so that
both builds of one session end up side by side; every launch's time is kept."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (inputs, l0, l1, layer-0 table rows, [(streams, bits)], [ctx_mode])
SHAPES = {
    "128x24/8/1": (128, 24, 8, 1 << 10, [(1024, 512), (2048, 512)], [0, 3]),
    "91x24/8/1": (91, 24, 8, 1 << 10, [(1024, 1024)], [4]),
    "40x5/3/1": (40, 5, 3, 1 << 10, [(1024, 1024)], [0]),
    "256x24/8/1": (256, 24, 8, 1 << 12, [(2048, 512)], [0]),      # bench.py's also.synth3
    "stock90": (90, 24, 8, 0, [(1024, 1024)], [4]),               # bench.py's also.stock_real
}


def topo_of(topology, name):
    n, l0, l1, t0, _, _ = SHAPES[name]
    if name == "stock90":
        return topology.stock(90)
    return topology.synth3(n, l0=l0, l1=l1, table0=t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="checkout whose gmix_amd package (and built library) is timed")
    ap.add_argument("--label", default="this")
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--commit", default=None, help="what the tree is (a checkout without .git cannot say)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import gmix_amd
    from gmix_amd import topology
    has_switch = hasattr(gmix_amd.MixerGroup, "set_register_rows")
    commit = a.commit
    if not commit and os.path.exists(os.path.join(a.tree, ".git")):
        commit = subprocess.run(["git", "-C", a.tree, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    res = {"tree": os.path.relpath(os.path.abspath(a.tree), ROOT), "commit": commit or None,
           "build": gmix_amd._lib.lib().gmx_build_info().decode(), "has_register_rows": has_switch, "runs": []}
    for name in a.shapes.split(","):
        n, l0, l1, _, sizes, modes = SHAPES[name]
        topo = topo_of(topology, name)
        for S, T in sizes:
            for mode in modes:
                for route in (["default", "register_rows"] if has_switch else ["default"]):
                    g = gmix_amd.MixerGroup(topo, S)
                    if route == "register_rows":
                        g.set_register_rows(True)
                    b = gmix_amd.Batch(g, T, outputs=False, mask=False)
                    ms = []
                    for k in range(a.warmup + a.launches):
                        b.fill_synthetic(T, seed=11, restart=(k == 0), ctx_mode=mode, ctx_mod=70001 if mode == 3 else 1)
                        t = g.run(b, T, learn=True, timed=True)
                        if k >= a.warmup:
                            ms.append(t)
                    b.close()
                    g.close()
                    med = sorted(ms)[len(ms) // 2]
                    bpb = topo.bytes_per_bit()
                    r = {"shape": name, "streams": S, "bits": T, "ctx_mode": mode, "ctx_mod": 70001 if mode == 3 else 1, "route": route,
                         "kernel_ms": [round(x, 4) for x in ms], "kernel_ms_median": round(med, 4),
                         "spread": round((max(ms) - min(ms)) / med, 4), "bits_per_s": S * T / (med * 1e-3),
                         "algorithmic_bytes_per_bit": bpb, "frac_of_8TBs": S * T * bpb / (med * 1e-3) / 8e12}
                    res["runs"].append(r)
                    print(json.dumps(r), flush=True)
    if a.out:
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres[a.label] = res
        json.dump(allres, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
