"""Regenerates tests/golden/match_*.npz from the reference itself (build container only: it needs the reference's
sources and g++).  ref_match_harness.cpp is compiled against them where they lie, into oracle/_ref/; the fixtures
hold inputs, the reference's recorded results and its own coverage counters, nothing of its program text.

    python tests/golden/make_match_golden.py [--ref /path/to/reference]
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from gmix_amd.match import match_stream  # noqa: E402
from gmix_amd.topology import STOCK_MATCH, STOCK_MATCH_LIMIT  # noqa: E402

TUS = ["models/match.cpp", "contexts/basic-contexts.cpp", "contexts/skip-context.cpp", "contexts/murmur-hash.cpp",
       "contexts/nonstationary.cpp", "contexts/run-map.cpp", "memory/short-term-memory.cpp",
       "memory/long-term-memory.cpp", "mixer/sigmoid.cpp"]

# name -> (seed, bytes, table sizes or None for the stock six, limit, context ranges)
FIXTURES = {
    "match_stock": dict(seed=11, n=12000, tables=None, limit=STOCK_MATCH_LIMIT),
    "match_tiny": dict(seed=5, n=6000, tables=[16, 7, 1], limit=5, ranges=[40, 23, 9]),
    "match_k8": dict(seed=23, n=6000, tables=[64, 100, 256, 1000, 4096, 5000, 33, 1 << 14], limit=60,
                     ranges=[256, 1 << 12, 1 << 16, 1 << 20, 1 << 24, 1 << 16, 97, 1 << 30]),
}
# what every fixture has to cover, by the reference's own counters
NEED = dict(not_pushed=200, eoh_resets=1, bits_at_255=400, same_entry=20)
# match_tiny does not reach match_length_ 255 with this stream generator, for any seed tried.  A match of L bits
# needs its pointer at least (L - 64) / 8 history bytes behind the end when it begins (bytes are no longer pushed from
# 64 bits on, and the pointer then runs into the end: match.cpp:40-42): 24 bytes for 255.  A table entry can survive
# that long only while no later byte's context falls on the same entry, and with 16, 7 and 1 entries and contexts that
# follow the data, the copies this generator makes (their sources drawn from the whole history) begin at entries that
# have been overwritten since.  A stream built by hand around one surviving entry could reach it; this generator's
# streams do not, so the counter is recorded (0) and asserted in the two other fixtures only.
EXEMPT = {("match_tiny", "bits_at_255")}


def slot_hash(u):
    """FNV-1a over the K 32-bit patterns of every bit's slots: u [T][K] uint32 -> [T] uint32."""
    h = np.full(len(u), 2166136261, np.uint64)
    for k in range(u.shape[1]):
        h = ((h ^ u[:, k].astype(np.uint64)) * np.uint64(16777619)) & np.uint64(0xffffffff)
    return h.astype(np.uint32)


def build(ref):
    out = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "ref_match_harness")
    src = os.path.join(ref, "src")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-include", "cstring", "-I", src,
                           os.path.join(HERE, "ref_match_harness.cpp")] + [os.path.join(src, t) for t in TUS] +
                          ["-o", exe])
    return exe


def contexts_for(data, ranges):
    """Contexts of ours for the non-stock fixtures: model k hashes the last (k % 4) + 1 bytes into [0, ranges[k]) --
    tied to the data, so that matches are found, and small enough for the tables to fill."""
    n, K = len(data), len(ranges)
    ctx = np.zeros((n, K), np.uint64)
    prev = np.zeros(4, np.uint64)
    for i in range(n):
        for k in range(K):
            h = np.uint64(0)
            for j in range(k % 4 + 1):
                h = (h * np.uint64(40503) + prev[j] + np.uint64(k)) & np.uint64(0xffffffff)
            ctx[i, k] = (h & np.uint64(0xffffffff)) % np.uint64(ranges[k])
        prev[1:] = prev[:-1]
        prev[0] = data[i]
    return ctx.astype(np.uint32)


def run(exe, name, spec):
    data = match_stream(spec["seed"], spec["n"])
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        data.tofile(fin)
        if spec["tables"] is None:
            tables = [t for _, t in STOCK_MATCH]
            cmd = [exe, fin, fout, "stock"]
            ctx_bytes = None
        else:
            tables = spec["tables"]
            ctx_bytes = contexts_for(data, spec["ranges"])
            fctx = os.path.join(td, "ctx.bin")
            ctx_bytes.tofile(fctx)
            cmd = [exe, fin, fout, "ctx", fctx, str(spec["limit"])] + [str(t) for t in tables]
        subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
        raw = open(fout, "rb").read()
    K, T = struct.unpack_from("<IQ", raw, 0)
    assert K == len(tables) and T == 8 * len(data)
    rec = np.dtype([("ctx", "<u4", (K,)), ("bc", "<u4"), ("bit", "u1"), ("slot", "<f4", (K,)), ("act", "u1", (K,)),
                    ("lm", "<u4")])
    r = np.frombuffer(raw, rec, T, 12)
    off = 12 + T * rec.itemsize
    (nl,) = struct.unpack_from("<Q", raw, off)
    long_sec = raw[off + 8:off + 8 + nl]
    off += 8 + nl
    (ns,) = struct.unpack_from("<Q", raw, off)
    short_sec = raw[off + 8:off + 8 + ns]
    off += 8 + ns
    usage = struct.unpack_from("<%dQ" % K, raw, off)
    off += 8 * K
    not_pushed, eoh, at255, max_count, same_entry = struct.unpack_from("<5Q", raw, off)
    assert off + 40 == len(raw) and ns == 11 * K
    # the aliased variables do not move within a byte: one row per byte is all a test needs
    ctx = r["ctx"].reshape(-1, 8, K)
    assert (ctx == ctx[:, :1]).all()
    assert (r["bit"] == np.unpackbits(data)).all()
    if ctx_bytes is not None:
        assert (ctx[:, 0] == ctx_bytes).all()
    # which checkpoint branch every model took
    dense, p = [], 8 + struct.unpack_from("<Q", long_sec, 0)[0]
    for t in tables:
        (cnt,) = struct.unpack_from("<I", long_sec, p)
        d = not (cnt < (5.0 / 9.0) * t)
        dense.append(int(d))
        p += 4 + (5 * t if d else 9 * cnt) + 2048
    assert p == len(long_sec)
    meta = dict(not_pushed=not_pushed, eoh_resets=eoh, bits_at_255=at255, max_count=max_count,
                same_entry=same_entry)
    print(name, meta, "dense:", dense, "long bytes:", nl)
    for key, least in NEED.items():
        assert (name, key) in EXEMPT or meta[key] >= least, (name, key, meta[key], least)
    if name in ("match_stock", "match_tiny"):
        assert max_count == spec["limit"], (name, max_count)
    np.savez_compressed(
        os.path.join(HERE, name + ".npz"), seed=spec["seed"], n_bytes=spec["n"], data=data,
        tables=np.array(tables, np.uint32), limit=spec["limit"], ctx_bytes=ctx[:, 0].astype(np.uint32),
        # 2.3 MB of slot values would not fit a fixture: per bit one FNV-1a word over the K bit patterns.  A test
        # that needs the floats themselves takes them from tests/helpers/match_ref.c, once its hashes equal these.
        slot_hash=slot_hash(r["slot"].view(np.uint32)),
        act=np.packbits(r["act"], axis=None), lm=r["lm"].astype(np.uint8),
        long=np.frombuffer(long_sec, np.uint8), short=np.frombuffer(short_sec, np.uint8),
        usage=np.array(usage, np.uint64), dense=np.array(dense, np.uint8),
        meta_keys=np.array(sorted(meta)), meta_vals=np.array([meta[k] for k in sorted(meta)], np.uint64))
    return dense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("GMX_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    exe = build(a.ref)
    dense = []
    for name, spec in FIXTURES.items():
        dense += run(exe, name, spec)
    assert 0 in dense and 1 in dense, "both checkpoint branches across the set"


if __name__ == "__main__":
    main()
