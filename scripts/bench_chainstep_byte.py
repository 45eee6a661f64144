#!/usr/bin/env python3
"""What a whole byte per call is worth in the lock-step chain (gmx_chainstep_byte, include/gmxmix_decoder.h): the stock
chain with every bank attached -- LSTM byte model, 41 Indirect models, six Match models, the 52 context variables, 33
mixers -- decoding random input, per stream count:

  leg A  eight gmx_chainstep_step calls per byte, the host's turn between them in C (scripts/chainstep_byte_host.cpp:
         Decoder::Decode of every stream's bit, ModPPMD's range walk, the record's slot and mask bit)
  leg B  one gmx_chainstep_byte call per byte

  wall_us_per_byte     by the host's clock around a leg of `--bytes` bytes; legs alternate within a round; the figure
                       is the median of the rounds, `spread` their (max - min) / median
  device_us_per_byte   HIP events around the graphs (gmx_chainstep_timed_step x 8, gmx_chainstep_timed_byte), in a
                       pass of its own

Every process is a fresh child.  With --parent-lib (a libgmxmix.so built from the parent commit) leg A is measured on
that library too, in processes alternating with the new library's: the per-bit route's graphs and kernels are unchanged,
so the two should agree within the spread of repeated runs.  The Indirect and the Match bank use 256-entry tables so
that 256 streams fit beside the hash tables (scripts/bench_chainstep_ctx.py does the same).  No threshold is attached to
these numbers.  Writes profiles/chainstep_byte_bench.json.

    python scripts/bench_chainstep_byte.py [--streams 64 256] [--bytes 300] [--warmup 60] [--rounds 3]
                                           [--parent-lib build_tmp/libgmxmix_parent.so] [--processes 2]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 41
IND_SLOTS = [(8 + 2 * i, 9 + 2 * i) for i in range(K)]
MATCH_SLOTS = [2, 3, 4, 5, 6, 7]
PPMD_SLOT, LSTM_SLOT, MIX_LSTM_COL, IND_LSTM_COL = 0, 1, 22, 16
FILL = 0xFFFFFFFF
IN_LEN = 4096


def host_lib():
    """scripts/chainstep_byte_host.cpp as a shared library under build_tmp/ (built once, strict floats)."""
    out = os.path.join(ROOT, "build_tmp", "chainstep_byte_host.so")
    src = os.path.join(ROOT, "scripts", "chainstep_byte_host.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", out, src])
    H = C.CDLL(out)
    vp, i32, u32 = C.c_void_p, C.c_int, C.c_uint32
    H.gmxb_init.argtypes = [i32, vp, vp, u32]
    H.gmxb_init.restype = None
    H.gmxb_host_bit.argtypes = [i32, i32, i32, vp, vp, vp, u32, vp, vp, vp, i32, vp, i32, i32, vp, vp]
    H.gmxb_host_bit.restype = None
    return H


class Chain:
    def __init__(self, gmix_amd, S, n_bytes, decoder, inputs, seed=1):
        from gmix_amd import topology
        z = np.load(os.path.join(ROOT, "tests", "golden", "ind_stock41.npz"))
        w0 = ((np.random.default_rng(seed).random((3, 50, 563), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
        descs, mixer_route, ind_route, match_route = topology.stock_contexts()
        self.S = S
        self.lg = gmix_amd.LstmGroup(S)
        self.ig = gmix_amd.IndirectGroup([(256, lr) for _, lr in topology.stock_indirect()], z["ns_next"], z["rm_next"], S,
                                         slots=IND_SLOTS)
        self.mg = gmix_amd.MixerGroup(topology.stock(90), S)
        self.xg = gmix_amd.MatchGroup([(256, lim, sl) for (_, lim, _), sl in zip(topology.stock_match(), MATCH_SLOTS)],
                                      n_bytes + 64, S)
        self.cg = gmix_amd.CtxGroup(descs, S)
        for s in range(S):
            self.lg.set_weights(w0, stream=s)
        cs = gmix_amd.ChainStep(self.mg, self.ig, self.lg, lstm_slot=LSTM_SLOT, mixer_ctx_col=MIX_LSTM_COL,
                                ind_ctx_col=IND_LSTM_COL)
        cs.attach_match(self.xg, topology.stock_longest_match_columns())
        cs.attach_ctx(self.cg, mixer_route, ind_route, match_route)
        for v in (cs.contexts, cs.ind_contexts, cs.match_contexts, cs.bit_contexts):
            v[:] = FILL
        cs.predictions[:] = 0
        cs.active_mask[:] = 0
        if decoder:
            cs.attach_decoder(PPMD_SLOT)
            for s in range(S):
                cs.set_input(s, inputs[s].tobytes())
            cs.take[:] = 1
        self.cs = cs

    def close(self):
        self.cs.close()
        for h in (self.cg, self.xg, self.lg, self.ig, self.mg):
            h.close()


def child(a):
    import gmix_amd
    L = gmix_amd._lib.lib()
    S = a.streams[0]
    legs = a.legs
    total = (a.warmup + a.bytes) * (a.rounds + 1) + 16
    rng = np.random.default_rng(3)
    inputs = rng.integers(0, 256, (S, IN_LEN), dtype=np.uint8)
    ppms = rng.random((8, S, 256), dtype=np.float32) + np.float32(1e-3)
    ppms /= ppms.sum(axis=2, keepdims=True)
    out = {"lib": a.tag, "build": L.gmx_build_info().decode(), "streams": S}
    run = {}
    if "A" in legs:
        H = host_lib()
        ca = Chain(gmix_amd, S, total, False, inputs)
        cs = ca.cs
        st = np.zeros((S, 4), np.uint32)
        walk = np.zeros((S, 2), np.int32)
        H.gmxb_init(S, st.ctypes.data, inputs.ctypes.data, IN_LEN)
        n_pad = cs.predictions.shape[1]
        ptr = dict(st=st.ctypes.data, walk=walk.ctypes.data, buf=inputs.ctypes.data, p=cs.p.ctypes.data,
                   ppm=cs.ppm.ctypes.data, pred=cs.predictions.ctypes.data, mask=cs.active_mask.ctypes.data,
                   bits=cs.bits.ctypes.data, what=cs.what.ctypes.data)
        state = {"n": 0}
        step, timed_step, h = L.gmx_chainstep_step, L.gmx_chainstep_timed_step, cs.h
        ms = C.c_float(0)

        def leg_a(n, timed=False):
            dev = 0.0
            for _ in range(n):
                cs.ppm[:] = ppms[state["n"] & 7]
                for j in range(8):
                    H.gmxb_host_bit(S, j, 1 if (state["n"] or j) else 0, ptr["st"], ptr["walk"], ptr["buf"], IN_LEN,
                                    ptr["p"], ptr["ppm"], ptr["pred"], n_pad, ptr["mask"], cs.mask_words, PPMD_SLOT,
                                    ptr["bits"], ptr["what"])
                    if timed:
                        rc = timed_step(h, C.byref(ms))
                        dev += ms.value
                    else:
                        rc = step(h)
                    assert rc == 0, rc
                state["n"] += 1
            return dev
        run["A"] = leg_a
    if "B" in legs:
        cb = Chain(gmix_amd, S, total, True, inputs)
        csb = cb.cs
        byte, timed_byte, hb = L.gmx_chainstep_byte, L.gmx_chainstep_timed_byte, csb.h
        nb = {"n": 0}
        msb = C.c_float(0)

        def leg_b(n, timed=False):
            dev = 0.0
            for _ in range(n):
                csb.decoder_ppm[:] = ppms[nb["n"] & 7]
                if timed:
                    rc = timed_byte(hb, C.byref(msb))
                    dev += msb.value
                else:
                    rc = byte(hb)
                assert rc == 0, rc
                nb["n"] += 1
            return dev
        run["B"] = leg_b
    wall = {k: [] for k in run}
    for r in range(a.rounds):
        order = sorted(run) if r % 2 == 0 else sorted(run, reverse=True)
        for k in order:
            run[k](a.warmup)
            t0 = time.perf_counter()
            run[k](a.bytes)
            wall[k].append((time.perf_counter() - t0) * 1e6 / a.bytes)
    for k in run:
        run[k](a.warmup // 2)
        dev = run[k](a.bytes // 2, timed=True) * 1e3 / (a.bytes // 2)
        med = float(np.median(wall[k]))
        out[k] = {"wall_us_per_byte": med, "spread": (max(wall[k]) - min(wall[k])) / med, "rounds_us": wall[k],
                  "device_us_per_byte": dev}
    if "A" in legs and "B" in legs:
        # both legs decode the same input under the same distributions: after as many bytes they have the same state
        assert state["n"] == nb["n"]
        # (leg A's last bit is decoded by the NEXT step's host turn: done here on copies)
        st2, walk2 = st.copy(), walk.copy()
        pred2, mask2 = np.zeros_like(cs.predictions), np.zeros_like(cs.active_mask)
        b2, w2 = np.zeros(S, np.uint8), np.zeros(S, np.uint8)
        H.gmxb_host_bit(S, 1, 1, st2.ctypes.data, walk2.ctypes.data, ptr["buf"], IN_LEN, ptr["p"], ptr["ppm"],
                        pred2.ctypes.data, n_pad, mask2.ctypes.data, cs.mask_words, PPMD_SLOT, b2.ctypes.data,
                        w2.ctypes.data)
        sb = np.array([csb.decoder_state(s) for s in range(S)], np.uint32)
        out["same_coder_state"] = bool(np.array_equal(sb, st2))
    if "A" in legs:
        ca.close()
    if "B" in legs:
        cb.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--bytes", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--processes", type=int, default=2, help="fresh processes per library and stream count")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chainstep_byte_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--legs", default="AB")
    ap.add_argument("--tag", default="new")
    a = ap.parse_args()
    if a.child:
        return child(a)
    host_lib()
    res = {"setup": {"bytes_per_leg": a.bytes, "warmup_bytes": a.warmup, "rounds": a.rounds,
                     "clock": "host, around each leg of a round; us per byte; median and (max-min)/median of the rounds",
                     "legs": {"A": "8 x gmx_chainstep_step per byte, the host's decode and range walk in C between them",
                              "B": "1 x gmx_chainstep_byte per byte"},
                     "shape": "stock: LSTM, 52 context variables, 6 Match, 41 Indirect (256-entry tables), 33 mixers of 90"},
           "runs": []}
    for S in a.streams:
        for i in range(a.processes):
            for tag, lib, legs in (("new", None, "AB"), ("parent", a.parent_lib, "A")):
                if tag == "parent" and not lib:
                    continue
                env = dict(os.environ)
                if lib:
                    env["GMX_LIB"] = os.path.abspath(lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--streams", str(S), "--bytes", str(a.bytes),
                       "--warmup", str(a.warmup), "--rounds", str(a.rounds), "--legs", legs, "--tag", tag]
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:   # (nothing more is started on the device after a process that failed)
                    sys.stderr.write(r.stdout + r.stderr)
                    raise SystemExit(r.returncode)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
                row = json.loads(line[7:])
                row["process"] = i
                res["runs"].append(row)
                print(json.dumps(row), flush=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
