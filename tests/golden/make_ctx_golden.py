"""Regenerates tests/golden/ctx_*.npz from the reference itself (build container only: it needs the reference's
sources and g++).  ref_ctx_harness.cpp is compiled against them where they lie, into oracle/_ref/, by the recipe of
oracle/ref_build/Makefile (tests/ctx_harness.py calls it and reads the harness's output); the fixtures hold
inputs, settings, the reference's recorded results and its own coverage counters, nothing of its program text.

    python tests/golden/make_ctx_golden.py [--ref /path/to/reference]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctx_common  # noqa: E402
import ctx_harness  # noqa: E402
from gmix_amd.ctx import desc_array  # noqa: E402
from gmix_amd.match import match_stream  # noqa: E402
from gmix_amd.topology import stock_context_descs  # noqa: E402


def popcount(i):
    return bin(i).count("1")


# A bank the reference's Predictor does not build: hash tables of 1, 3, 7 and 100 entries (no power of two among the
# last three), every order 1..4, a skip over eight bytes up to position 15, interval maps that are no division.
TINY = [
    ("hash_1", "indirect_hash", dict(outer_order=1, table_size=1, inner_order=1)),
    ("hash_3", "indirect_hash", dict(outer_order=2, table_size=3, inner_order=3)),
    ("hash_7", "indirect_hash", dict(outer_order=4, table_size=7, inner_order=4)),
    ("hash_100", "indirect_hash", dict(outer_order=3, table_size=100, inner_order=2)),
    ("skip_8", "skip", dict(bytes_to_use=[0, 1, 2, 3, 5, 8, 13, 15])),
    ("skip_15", "skip", dict(bytes_to_use=[15])),
    ("skip_0", "skip", dict(bytes_to_use=[0])),
    ("interval_odd_31", "interval", dict(map=[(7 * i + i // 3) % 11 for i in range(256)], num_bits=31)),
    ("interval_pop_5", "interval", dict(map=[popcount(i) for i in range(256)], num_bits=5)),
    ("interval_xor_20", "interval", dict(map=[i ^ 0x5a for i in range(256)], num_bits=20)),
    ("interval_zero_1", "interval", dict(map=[0] * 256, num_bits=1)),
    ("last_byte", "recent_byte", dict(index=0)),
    ("recent_bytes[9]", "recent_byte", dict(index=9)),
    ("bit_context", "bit_context", {}),
    ("last_byte_plus_recent", "byte_plus_recent", dict(index=0)),
    ("second_last_plus_recent", "byte_plus_recent", dict(index=1)),
    ("always_zero", "zero", {}),
]
# name -> (stream seed, bytes, variables, the hash table whose count is to equal table_size / 2 at a recorded position)
FIXTURES = {
    "ctx_stock": dict(seed=11, n=3000, descs=stock_context_descs(), boundary=None),
    "ctx_tiny": dict(seed=5, n=2500, descs=TINY, boundary="hash_100"),
}
NEED = dict(same_entry=20, wraps=1)


def find_boundary(descs, h, size, bits):
    """The first bit count at which hash variable h holds exactly size / 2 non-zero entries, by tests/helpers/ctx_ref.c
    -- the position is then recorded by the reference itself, and its own count is what run() asserts."""
    ref = ctx_common.Ref(descs)
    for t in range(0, len(bits), 8):
        ref.run(bits[t:t + 8], values=False)
        data, off = ref.export()
        if ctx_harness.section_count(data[off[h]:off[h + 1]]) == size // 2:
            return t + 8
    raise AssertionError("no position with count == table_size / 2")


def run(exe, name, spec, out_dir=HERE):
    data = match_stream(spec["seed"], spec["n"])
    bits = np.unpackbits(data)
    T = len(bits)
    names = [d[0] for d in spec["descs"]]
    arr = desc_array(spec["descs"])
    descs = [arr[i] for i in range(len(names))]
    V = len(descs)
    hash_vars = [i for i, d in enumerate(descs) if d.kind == 6]
    H = len(hash_vars)
    # never run, 3 bits in, 1 001 bytes + 5 bits (the ring has wrapped), the end
    positions = [0, 3, 8 * 1001 + 5, T]
    boundary = {}
    if spec["boundary"]:
        h = [names[v] for v in hash_vars].index(spec["boundary"])
        size = descs[hash_vars[h]].table_size
        positions.append(find_boundary(descs, h, size, bits))
        boundary = dict(position_index=len(positions) - 1, hash=h, table_size=size)
    rec = ctx_harness.record(data, arr, V, positions, exe)
    assert rec["T"] == T
    vals, same_entry, wraps, n_pos = rec["values"], rec["same_entry"], rec["wraps"], len(positions)
    sections, section_off = b"", []
    for row in rec["sections"]:
        section_off.append([])
        for sec in row:
            section_off[-1].append(len(sections))
            sections += sec
        section_off[-1].append(len(sections))
    boards = rec["boards"]
    dense = sum(rec["dense"], [])
    # the harness records positions in ascending order
    order = np.argsort(positions, kind="stable")
    positions = [positions[i] for i in order]
    if boundary:
        boundary["position_index"] = int(np.nonzero(order == boundary["position_index"])[0][0])
        sec = sections[section_off[boundary["position_index"]][boundary["hash"]]:]
        assert ctx_harness.section_count(sec) == boundary["table_size"] // 2, "the reference's own count at the boundary"
    # byte-level variables do not move within a byte; the two per-bit kinds are their first value + bit_context
    bc = ctx_common.bit_contexts(data)
    by = vals.reshape(-1, 8, V)
    for v, d in enumerate(descs):
        if d.kind in ctx_common.PER_BIT_KINDS:
            assert (by[:, :, v] == by[:, :1, v] + bc.reshape(-1, 8)).all(), names[v]
        else:
            assert (by[:, :, v] == by[:, :1, v]).all(), names[v]
    skips = [v for v, d in enumerate(descs) if d.kind == 5]
    assert all(vals[0, v] != 0 for v in skips), "a SkipContext fires at the very first Predict"
    meta = dict(same_entry=same_entry, wraps=wraps)
    print(name, meta, "dense per position and table:", dense, "section bytes:", len(sections))
    for key, least in NEED.items():
        assert meta[key] >= least, (name, key, meta[key], least)
    np.savez_compressed(
        os.path.join(out_dir, name + ".npz"), seed=spec["seed"], n_bytes=spec["n"], data=data,
        descs=np.frombuffer(bytes(arr)[:V * C.sizeof(arr[0])], np.uint8), names=np.array(names),
        byte_vals=by[:, 0, :].astype(np.uint32), positions=np.array(positions, np.uint64),
        sections=np.frombuffer(sections, np.uint8), section_off=np.array(section_off, np.uint64),
        boards=np.stack(boards), dense=np.array(dense, np.uint8).reshape(n_pos, H),
        boundary_keys=np.array(sorted(boundary)), boundary_vals=np.array([boundary[k] for k in sorted(boundary)], np.int64),
        meta_keys=np.array(sorted(meta)), meta_vals=np.array([meta[k] for k in sorted(meta)], np.uint64))
    return dense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("GMX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=HERE, help="directory the fixtures are written to")
    a = ap.parse_args()
    exe = ctx_harness.build(a.ref)
    dense = {}
    for name, spec in FIXTURES.items():
        dense[name] = run(exe, name, spec, a.out)
    # The 2^8-entry tables of the stock bank need 128 non-zero entries for the dense branch: with this stream generator
    # the three of them are dense at the end of ctx_stock's 3 000 bytes and sparse at the three positions before, so
    # ctx_stock alone has both branches; ctx_tiny takes the dense branch from the start (a table of 1 entry is dense by
    # definition: count < 0 never holds) and the sparse one in its first bytes.
    both = sum(dense.values(), [])
    assert 0 in both and 1 in both, "both WriteToDisk branches across the set"
    assert 1 in dense["ctx_tiny"] and 0 in dense["ctx_stock"] and 1 in dense["ctx_stock"]


if __name__ == "__main__":
    main()
