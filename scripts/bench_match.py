"""Match banks on the device: the six stock models over the Match fixtures' stream generator, 64 and 256 streams x
2 048 bits per launch -- warm-up launches, then timed ones by HIP events (gmx_match_run's kernel_ms) -- beside
tests/helpers/match_ref.c (OUR plain-C restatement, not the reference's binary) on one host core over the same
records.  Reported, not gated.  Writes profiles/match_bench.json.

    python scripts/bench_match.py [--streams 64 256] [--launches 10] [--warmup 3]
"""
import argparse
import ctypes as C
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
from gmix_amd.match import match_stream, stream_bits  # noqa: E402


def murmur3_u64(key, seed=0xDEADBEEF):
    """MurmurHash3_x86_32 of the 8 bytes of `key` (uint64 array), as SkipContext::Predict calls it
    (skip-context.cpp:12-17)."""
    M = np.uint64(0xffffffff)

    def rotl(x, r):
        return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & M

    h = np.full(key.shape, seed, np.uint64)
    for k in (key & M, key >> np.uint64(32)):
        k = (k * np.uint64(0xcc9e2d51)) & M
        k = rotl(k, 15)
        k = (k * np.uint64(0x1b873593)) & M
        h = rotl(h ^ k, 13)
        h = (h * np.uint64(5) + np.uint64(0xe6546b64)) & M
    h ^= np.uint64(8)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & M
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & M
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def stock_contexts(data):
    """[n][6]: last_byte and the hashes of the last 2..6 bytes at every byte boundary (predictor.cpp:84-108)."""
    n = len(data)
    prev = [np.concatenate((np.zeros(j + 1, np.uint64), data[:n - j - 1].astype(np.uint64)))[:n] for j in range(6)]
    out = np.zeros((n, 6), np.uint32)
    out[:, 0] = prev[0]
    for m in range(2, 7):
        key = np.zeros(n, np.uint64)
        for j in range(m):
            key = (key << np.uint64(8)) + prev[j]
        out[:, m - 1] = murmur3_u64(key)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--bits", type=int, default=2048)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.json"))
    a = ap.parse_args()
    rounds = a.warmup + a.launches
    nb = a.bits * rounds // 8
    distinct = 16
    recs = []
    for i in range(distinct):
        d = match_stream(1000 + i, nb)
        bits, bc = stream_bits(d)
        recs.append((np.repeat(stock_contexts(d), 8, axis=0), bc, bits))
    # the numpy hashes above are the reference's: the match_stock fixture recorded SkipContext's own values
    import match_common as mc
    fx = mc.fixture("match_stock")
    assert np.array_equal(stock_contexts(fx.data), fx.ctx[::8]), "stock_contexts != the reference's recorded contexts"
    models = topology.stock_match()
    res = {"build": gmix_amd._lib.lib().gmx_build_info().decode(), "bits_per_launch": a.bits,
           "launches": a.launches, "warmup": a.warmup, "device": []}
    for S in a.streams:
        g = gmix_amd.MatchGroup(models, nb + 64, S)
        b = gmix_amd.MatchBatch(g, a.bits)
        ms = []
        for r in range(rounds):
            t0 = r * a.bits
            for s in range(S):
                c, bc, bits = recs[s % distinct]
                b.set_records(s, c[t0:t0 + a.bits], bc[t0:t0 + a.bits], bits[t0:t0 + a.bits])
            b.upload(a.bits)
            b.wait()
            t = g.run(b, a.bits, timed=True)
            if r >= a.warmup:
                ms.append(t)
        sec = g.export(0)  # (sizes the buffers, then exports: the second time, with buffers in hand, is one export)
        nl, ns = C.c_size_t(len(sec[0])), C.c_size_t(len(sec[1]))
        lb, sb = np.zeros(nl.value, np.uint8), np.zeros(ns.value, np.uint8)
        t0 = time.perf_counter()
        rc = g.L.gmx_match_export(g.h, 0, lb.ctypes.data_as(C.c_void_p), C.byref(nl), sb.ctypes.data_as(C.c_void_p),
                                  C.byref(ns))
        export_ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and lb.tobytes() == sec[0]
        med = float(np.median(ms))
        res["device"].append({
            "streams": S, "kernel_ms_median": med, "kernel_ms_min": float(min(ms)), "kernel_ms_max": float(max(ms)),
            "stream_bits_per_s": S * a.bits / (med * 1e-3), "us_per_stream_bit": med * 1e3 / (S * a.bits),
            "device_bytes_per_stream": int(g.bank_bytes), "export_ms": export_ms, "export_long_bytes": len(sec[0])})
        b.close()
        g.close()
    # our restatement on one host core over the records of one stream
    ref = mc.Ref([(t, l) for t, l, _ in models])
    c, bc, bits = recs[0]
    t0 = time.perf_counter()
    ref.run(c, bc, bits)
    dt = time.perf_counter() - t0
    res["host_restatement_one_core"] = {"what": "tests/helpers/match_ref.c (gcc -O2), not the reference's binary",
                                        "bits": len(bits), "us_per_stream_bit": dt * 1e6 / len(bits)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
