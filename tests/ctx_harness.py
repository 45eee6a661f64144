"""The reference's own context objects behind tests/golden/ref_ctx_harness.cpp (oracle/_ref/ref_ctx_harness, present
where the reference was built): the one recipe that builds the binary, the call, and the reader of its output file.
Shared by tests/golden/make_ctx_golden.py, which records fixtures with it, and tests/test_oracle_ctx_shapes.py, which
compares tests/helpers/ctx_ref.c with it live."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np

from gmix_amd._lib import CtxBlackboard, CtxDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_ctx_harness")
BOARD_BYTES = C.sizeof(CtxBlackboard)
INDIRECT_HASH = 6


def have_harness():
    return os.path.exists(HARNESS)


def build(ref):
    """oracle/ref_build/Makefile's ref_ctx_harness target against the reference's sources under `ref`."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref_build"), "REF=" + os.path.abspath(ref),
                           "../_ref/ref_ctx_harness"])
    return HARNESS


def section_count(sec):
    """The count a WriteToDisk section begins with: the table's non-zero entries."""
    return struct.unpack_from("<I", sec, 0)[0]


def is_dense(sec, table_size):
    """WriteToDisk's branch (indirect-hash.cpp:42), from the section's own count."""
    return not section_count(sec) < table_size // 2


def parse(raw, descs, positions):
    """ref_ctx_harness's out.bin (the layout is in the head of ref_ctx_harness.cpp) for the variables `descs` and the
    requested `positions`, which the harness records in ascending order:
      values [T][V] uint32 at Predict of every bit; positions sorted; sections [P][H] bytes; dense [P][H] 0 / 1;
      boards [P] uint8 arrays of gmx_ctx_blackboard; same_entry, wraps: the harness's coverage counters."""
    V = len(descs)
    sizes = [d.table_size for d in descs if d.kind == INDIRECT_HASH]
    H = len(sizes)
    V2, T = struct.unpack_from("<IQ", raw, 0)
    assert V2 == V
    vals = np.frombuffer(raw, "<u4", T * V, 12).reshape(T, V)
    off = 12 + 4 * T * V
    (n_pos,) = struct.unpack_from("<I", raw, off)
    off += 4
    assert n_pos == len(positions)
    positions = sorted(positions)
    sections, dense, boards = [], [], []
    for p in range(n_pos):
        pos_bits, h2 = struct.unpack_from("<QI", raw, off)
        off += 12
        assert pos_bits == positions[p] and h2 == H
        row, drow = [], []
        for h in range(H):
            (n,) = struct.unpack_from("<Q", raw, off)
            off += 8
            sec = raw[off:off + n]
            off += n
            d = is_dense(sec, sizes[h])
            assert n == 4 + (4 * sizes[h] if d else 8 * section_count(sec)) + 12
            row.append(sec)
            drow.append(int(d))
        sections.append(row)
        dense.append(drow)
        boards.append(np.frombuffer(raw, np.uint8, BOARD_BYTES, off))
        off += BOARD_BYTES
    same_entry, wraps = struct.unpack_from("<2Q", raw, off)
    assert off + 16 == len(raw)
    return dict(T=T, values=vals, positions=positions, sections=sections, dense=dense, boards=boards,
                same_entry=same_entry, wraps=wraps)


def record(data, arr, V, positions, exe=HARNESS):
    """Runs the harness over the bytes `data` for the first V descriptors of the ctypes array `arr` (gmix_amd.ctx.
    desc_array) and returns parse()'s dict.  The recording lives in a temporary directory."""
    descs = [arr[i] for i in range(V)]
    with tempfile.TemporaryDirectory() as td:
        fin, fd, fout = os.path.join(td, "in.bin"), os.path.join(td, "descs.bin"), os.path.join(td, "out.bin")
        np.ascontiguousarray(data, np.uint8).tofile(fin)
        with open(fd, "wb") as f:
            f.write(bytes(arr)[:V * C.sizeof(CtxDesc)])
        subprocess.check_call([exe, fin, fd, fout] + [str(p) for p in positions], stdout=subprocess.DEVNULL)
        with open(fout, "rb") as f:
            raw = f.read()
    out = parse(raw, descs, positions)
    assert out["T"] == 8 * len(data)
    return out
