"""Shared helpers for the tests that take the context banks (gmix_amd/csrc/gmx_ctx.hip) away from the two recorded
descriptor lists: a seeded generator of descriptor lists over everything ctx_describe() admits, a routing helper, the
input streams, and the named cases -- the ones tests/test_oracle_ctx_shapes.py pins tests/helpers/ctx_ref.c to the
reference on, and tests/test_gpu_ctx_shapes.py runs through the kernels."""
from collections import namedtuple

import numpy as np

from gmix_amd.ctx import desc_array
from gmix_amd.match import match_stream

MAX_VARS, MAX_HASH, CKPT_CHUNK, RING = 64, 16, 16384, 1000   # GMX_CTX_MAX_VARS / _MAX_HASH / _CKPT_CHUNK / _RING
# small tables, and tables around one and two chunks of the checkpoint kernels
TABLE_SIZES = [1, 2, 3, 5, 255, 256, 257, 1000, 4096, 16383, 16384, 16385, 32769, 40000, 49999, 65536]
# largest map value -> shift_ (interval-context.cpp:12-13) 1, 1, 2, 2, 3, 4, 7, 8; 31 and 63 add shift_ 5 and 6
INTERVAL_MAX = [0, 1, 2, 3, 7, 8, 100, 255, 31, 63]
STATELESS = ["skip", "interval", "recent_byte", "byte_plus_recent", "bit_context", "zero"]


def _params(rng, kind, reference_only, table_size=None):
    if kind == "indirect_hash":
        return dict(outer_order=int(rng.integers(1, 5)), inner_order=int(rng.integers(1, 5)),
                    table_size=int(rng.choice(TABLE_SIZES) if table_size is None else table_size))
    if kind == "skip":   # any order, with repeats
        return dict(bytes_to_use=[int(b) for b in rng.integers(0, 16, int(rng.integers(1, 9)))])
    if kind == "interval":
        mx = int(rng.choice(INTERVAL_MAX))
        return dict(map=[int(m) for m in rng.integers(0, mx + 1, 256)], num_bits=int(rng.integers(1, 32)))
    if kind == "recent_byte":
        return dict(index=int(rng.integers(0, 10)))
    if kind == "byte_plus_recent":
        # the reference has last_byte_plus_recent and second_last_plus_recent alone
        return dict(index=int(rng.integers(0, 2 if reference_only else 10)))
    return {}


def random_descs(seed, V, H, reference_only=False, table_sizes=None, hash_orders=None):
    """[(name, kind, params)] of V variables, H of them IndirectHash, in an order drawn with the rest; the other V - H
    are one of each stateless kind first (as far as they go) and drawn after that.  table_sizes: the H table sizes
    instead of drawn ones; hash_orders: outer_order is drawn from this list instead of 1..4.  reference_only keeps
    byte_plus_recent to index 0 / 1.  The draw of everything else does not depend on reference_only."""
    assert 1 <= V <= MAX_VARS and 0 <= H <= min(V, MAX_HASH)
    assert table_sizes is None or len(table_sizes) == H
    rng = np.random.default_rng(seed)
    rest = V - H
    kinds = [STATELESS[i] for i in rng.permutation(len(STATELESS))][:rest]
    kinds += [STATELESS[i] for i in rng.integers(0, len(STATELESS), rest - len(kinds))]
    kinds += ["indirect_hash"] * H
    kinds = [kinds[i] for i in rng.permutation(V)]
    out, h = [], 0
    for i, kind in enumerate(kinds):
        # (a generator of its own per variable: reference_only changes one draw of one variable, nothing after it)
        vr = np.random.default_rng([seed, i])
        p = _params(vr, kind, reference_only, table_sizes[h] if kind == "indirect_hash" and table_sizes else None)
        if kind == "indirect_hash":
            if hash_orders:
                p["outer_order"] = int(vr.choice(hash_orders))
            h += 1
        out.append((f"{kind}_{i}", kind, p))
    return out


def interval_grid(part):
    """Every shift_ 1..8 against every num_bits 1..31, 248 interval variables in four lists of 62 (part 0..3), each
    list with bit_context and the byte_plus_recent index the drawn lists happen to miss: the unrolled sum of the expand
    kernel, its `i * shift < 32` cut and the carry from the board at every pair.  A map's largest value is
    (1 << shift_) - 1, at byte 255; the others are drawn."""
    pairs = [(sh, nb) for sh in range(1, 9) for nb in range(1, 32)]
    out = []
    for sh, nb in pairs[part::4]:
        m = [int(x) for x in np.random.default_rng([77, sh, nb]).integers(0, 1 << sh, 256)]
        m[255] = (1 << sh) - 1
        out.append((f"interval_s{sh}_b{nb}", "interval", dict(map=m, num_bits=nb)))
    index = 3 if part else 1
    return out + [("bit_context", "bit_context", {}), (f"byte_plus_recent_{index}", "byte_plus_recent", dict(index=index))]


def as_descs(named):
    """The CtxDesc objects of a [(name, kind, params)] list (what ctx_common.Ref and CtxGroup take)."""
    arr = desc_array(named)
    return [arr[i] for i in range(len(named))]


def route(named, n_cols, seed, unrouted=2, repeats=3):
    """A route of n_cols columns over the variables of `named`: every kind there is comes first (as far as the columns
    go), `repeats` variables take a second and some a third column, `unrouted` columns are -1, the rest is drawn; the
    columns are then shuffled."""
    rng = np.random.default_rng([seed, n_cols])
    V = len(named)
    first = {}
    for v, (_, kind, _) in enumerate(named):
        first.setdefault(kind, v)
    cols = list(first.values())[:max(0, n_cols - unrouted)]
    for v in list(cols[:repeats]):
        cols += [v] * int(rng.integers(1, 3))
    cols = cols[:max(0, n_cols - unrouted)]
    cols += [int(v) for v in rng.integers(0, V, max(0, n_cols - unrouted - len(cols)))]
    cols += [-1] * (n_cols - len(cols))
    return [int(cols[i]) for i in rng.permutation(n_cols)]


# (seed, V, H, S, n_bytes, chunking).  chunking = (batch capacity, bits per launch) of the GPU test: launches that begin
# and end inside bytes (7, 333: neither is a multiple of 8), and launches at the batch's full capacity, which is no
# multiple of 8 either (1003).  Every stream is longer than the 1 000-byte history ring, for the reference's recorded
# position 8 * 1001 + 5; the GPU test codes GPU_BITS bits of it per stream.
Case = namedtuple("Case", "seed V H S n_bytes chunking")
INSIDE, FULL, SHORT = (1000, 333), (1003, 1003), (64, 7)
GPU_BITS = 2600
CASES = {
    # the corners of the lane geometry: no hash variable (no chain launch, no scratch array, the early returns of
    # export and import), one, all sixteen lanes of a stream; one variable, all 64
    "v1_h0": Case(101, 1, 0, 2, 1100, SHORT),
    "v1_h1": Case(107, 1, 1, 5, 1100, INSIDE),     # (outer_order 1: a repeated byte stays on one table entry)
    "v16_h16": Case(103, 16, 16, 5, 1200, FULL),
    "v64_h16": Case(104, 64, 16, 9, 1300, INSIDE),
    "v64_h0": Case(105, 64, 0, 3, 1100, FULL),
    "v63_h15": Case(106, 63, 15, 4, 1250, INSIDE),
}
_r = np.random.default_rng(20240)
for _i in range(8):
    _V = int(_r.integers(2, MAX_VARS + 1))
    CASES[f"random{_i}"] = Case(200 + _i, _V, int(_r.integers(0, min(_V, MAX_HASH) + 1)), int(_r.integers(1, 10)),
                                int(_r.integers(1050, 1500)), [INSIDE, FULL, SHORT][_i % 3])
for _i in range(4):   # interval_grid(_i)
    CASES[f"intervals{_i}"] = Case(300 + _i, 64, 0, 2, 1100, [INSIDE, FULL, SHORT, INSIDE][_i])
# the streams of these cases are gmix_amd.match.match_stream's (long runs of one byte, copies, a small alphabet: byte
# openings that stay on one table entry); every other stream is uniformly random bytes
MATCH_STREAM_CASES = ("random6", "random7")
# Tables of more than one checkpoint chunk that fill up: 40 000 random bytes; outer_order 3 / 4, so that nearly every
# byte opening is a context of its own (with order 1 a table never holds more than 256 entries)
BIG_TABLE_SIZES = [16385, 40000, 65536, 16384, 32769, 1, 2, 255, 256, 257, 16383, 5, 1000, 4096, 3, 49999]
BIG = Case(1, 64, 16, 1, 40000, (8192, 8192))
BIG_MID_BYTES = 25000
LONG_RUN_CASE = "v64_h16"   # the descriptors of the launch longer than the ring, of the ragged run with targets and of
#                             the lock-step case


def descs(name, reference_only=False):
    if name == "big_tables":
        return random_descs(BIG.seed, BIG.V, BIG.H, reference_only, table_sizes=BIG_TABLE_SIZES, hash_orders=[3, 4])
    if name.startswith("intervals"):
        named = interval_grid(int(name[len("intervals"):]))
        # (the reference has byte_plus_recent 0 / 1 alone)
        return [(n, k, dict(index=min(p["index"], 1)) if reference_only and k == "byte_plus_recent" else p)
                for n, k, p in named]
    c = CASES[name]
    return random_descs(c.seed, c.V, c.H, reference_only)


def case(name):
    return BIG if name == "big_tables" else CASES[name]


def stream(name):
    """The case's bytes (read-only)."""
    c = case(name)
    if name in MATCH_STREAM_CASES:
        data = match_stream(c.seed, c.n_bytes)
    else:
        data = np.random.default_rng(c.seed).integers(0, 256, c.n_bytes, dtype=np.uint8)
    data.setflags(write=False)
    return data


def offsets(S):
    """Stream s of a GPU case begins this many bytes into the case's data (tests/test_gpu_ctx.py's offsets)."""
    return [37 * s + s % 3 for s in range(S)]


def positions(name):
    """Bit counts the reference's state is recorded at: never run, 3 bits in, 1 001 bytes + 5 bits (the ring has
    wrapped), the end -- and for big_tables the position of the first export of the GPU test."""
    T = 8 * case(name).n_bytes
    return [0, 3, 8 * 1001 + 5, T] + ([8 * BIG_MID_BYTES] if name == "big_tables" else [])
