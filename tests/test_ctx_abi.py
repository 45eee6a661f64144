"""The gmx_ctx_* entry points: declared in include/gmxmix.h, exported by libgmxmix.so, and their behaviour where no
device is needed (argument checks; GMX_ERR_NO_DEVICE without a GPU: there is no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

import gmix_amd
from gmix_amd import _lib, topology
from gmix_amd.ctx import desc_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gmx_ctx_" + n for n in (
    "create destroy n_streams n_vars bank_bytes reset sync set_cu_mask batch_create batch_destroy batch_max_bits "
    "batch_bits batch_values batch_upload batch_download batch_wait run run_ragged blackboard_get blackboard_set "
    "export import copy memory_usage last_kernel_ms").split()]
GMX_ERR_INVALID, GMX_ERR_NO_DEVICE = -1, -4

ZERO = ("z", "zero", {})
HASH = ("h", "indirect_hash", dict(outer_order=1, table_size=16, inner_order=1))
IDENT = list(range(256))


def test_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gmxmix.h")).read()
    for t in ("gmx_ctx_desc", "gmx_ctx_targets", "gmx_ctx_blackboard"):
        assert "typedef struct %s" % t in header
    L = C.CDLL(gmix_amd.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in gmix_amd.ABI_SYMBOLS, n
        getattr(L, n)


def _create(descs, n_vars=None, S=1):
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.gmx_ctx_create(C.byref(h), desc_array(descs), len(descs) if n_vars is None else n_vars, S, 0)
    if rc == 0:
        L.gmx_ctx_destroy(h)
    return rc


@pytest.mark.parametrize("descs,n_vars,S", [
    ([ZERO], 0, 1),                                                                       # V = 0
    ([ZERO] * 65, 65, 1),                                                                 # V = 65
    ([HASH] * 17, 17, 1),                                                                 # 17 hash variables
    ([("h", "indirect_hash", dict(outer_order=0, table_size=16, inner_order=1))], 1, 1),  # order 0
    ([("h", "indirect_hash", dict(outer_order=1, table_size=16, inner_order=5))], 1, 1),  # order 5
    ([("h", "indirect_hash", dict(outer_order=5, table_size=16, inner_order=1))], 1, 1),
    ([("h", "indirect_hash", dict(outer_order=1, table_size=0, inner_order=1))], 1, 1),   # table_size 0
    ([("i", "interval", dict(map=IDENT, num_bits=0))], 1, 1),                             # num_bits 0
    ([("i", "interval", dict(map=IDENT, num_bits=32))], 1, 1),                            # num_bits 32
    ([("s", "skip", dict(bytes_to_use=[0, 1, 16]))], 1, 1),                               # an entry of 16
    ([("s", "skip", dict(bytes_to_use=[]))], 1, 1),                                       # no entry
    ([("r", "recent_byte", dict(index=10))], 1, 1),
    ([("k", 7, {})], 1, 1),                                                               # no such kind
    ([ZERO], 1, 0), ([ZERO], 1, -3),                                                      # S <= 0
])
def test_bad_arguments(descs, n_vars, S):
    assert _create(descs, n_vars, S) == GMX_ERR_INVALID


def test_nine_skip_entries():
    d = desc_array([("s", "skip", dict(bytes_to_use=list(range(8))))])
    d[0].n_bytes = 9
    L = _lib.lib()
    h = C.c_void_p()
    assert L.gmx_ctx_create(C.byref(h), d, 1, 1, 0) == GMX_ERR_INVALID


def test_no_device_is_an_error_not_a_fallback():
    want = 0 if gmix_amd.device_count() > 0 else GMX_ERR_NO_DEVICE
    assert _create([ZERO, HASH]) == want
    assert _create([("s", "skip", dict(bytes_to_use=list(range(8)))), ("i", "interval", dict(map=IDENT, num_bits=31)),
                    ("h", "indirect_hash", dict(outer_order=4, table_size=7, inner_order=4))]) == want


def test_null_handles():
    L = _lib.lib()
    assert L.gmx_ctx_n_streams(None) == GMX_ERR_INVALID
    assert L.gmx_ctx_n_vars(None) == GMX_ERR_INVALID
    assert L.gmx_ctx_reset(None) == GMX_ERR_INVALID
    assert L.gmx_ctx_sync(None) == GMX_ERR_INVALID
    assert L.gmx_ctx_bank_bytes(None) == 0
    assert L.gmx_ctx_batch_max_bits(None) == 0
    assert L.gmx_ctx_batch_bits(None) is None and L.gmx_ctx_batch_values(None) is None
    h = C.c_void_p()
    assert L.gmx_ctx_create(None, desc_array([ZERO]), 1, 1, 0) == GMX_ERR_INVALID
    assert L.gmx_ctx_create(C.byref(h), None, 1, 1, 0) == GMX_ERR_INVALID
    assert L.gmx_ctx_batch_create(C.byref(h), None, 8, 0) == GMX_ERR_INVALID
    assert L.gmx_ctx_run(None, None, 8, None, None) == GMX_ERR_INVALID
    assert L.gmx_ctx_run_ragged(None, None, None, None) == GMX_ERR_INVALID
    assert L.gmx_ctx_blackboard_get(None, 0, None) == GMX_ERR_INVALID
    assert L.gmx_ctx_export(None, 0, None, None, None) == GMX_ERR_INVALID
    assert L.gmx_ctx_import(None, 0, None, 0) == GMX_ERR_INVALID
    assert L.gmx_ctx_copy(None, 0, None, 0) == GMX_ERR_INVALID
    assert L.gmx_ctx_memory_usage(None, 0, None) == GMX_ERR_INVALID
    assert L.gmx_ctx_last_kernel_ms(None, None) == GMX_ERR_INVALID
    L.gmx_ctx_destroy(None)
    L.gmx_ctx_batch_destroy(None)


def test_stock_contexts_routes_by_name():
    descs, mixer_route, ind_route, match_route = topology.stock_contexts()
    names = [d[0] for d in descs]
    assert len(descs) == 52 and len(set(names)) == 52
    kinds = [d[1] for d in descs]
    assert kinds.count("interval") == 9 and kinds.count("indirect_hash") == 9 and kinds.count("skip") == 20
    assert len(mixer_route) == 33 and len(ind_route) == 41 and len(match_route) == 6
    ctx = topology.stock_context_names()
    assert [i for i, r in enumerate(mixer_route) if r < 0] == [6, 22, 30]
    assert [ctx[i] for i in (6, 22, 30)] == ["longest_match", "lstm_prediction_context", "longest_match"]
    assert [i for i, r in enumerate(ind_route) if r < 0] == [16]
    assert all(r >= 0 for r in match_route)
    for route, cols in ((mixer_route, ctx), (ind_route, [c for c, _, _ in topology.STOCK_INDIRECT]),
                        (match_route, [c for c, _ in topology.STOCK_MATCH])):
        assert all(r < 0 or names[r] == c for r, c in zip(route, cols))
    # 3 (2^8 + 2^16 + 2^24) u32 entries per stream
    assert sum(4 * d[2]["table_size"] for d in descs if d[1] == "indirect_hash") == 3 * 4 * (2**8 + 2**16 + 2**24)
