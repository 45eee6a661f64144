"""The gmx_match_* entry points: declared in include/gmxmix.h, exported by libgmxmix.so, and their behaviour where
no device is needed (argument checks; GMX_ERR_NO_DEVICE without a GPU: there is no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

import gmix_amd
from gmix_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gmx_match_" + n for n in (
    "create destroy n_streams n_models bank_bytes reset sync set_cu_mask batch_create batch_destroy batch_max_bits "
    "batch_contexts batch_bit_contexts batch_bits batch_predictions batch_active batch_longest batch_upload "
    "batch_download batch_wait run run_ragged forward learn slots_get slots_set history_size export import copy "
    "memory_usage").split()]
GMX_ERR_INVALID, GMX_ERR_NO_DEVICE = -1, -4


def test_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gmxmix.h")).read()
    assert "typedef struct gmx_match_desc" in header
    L = C.CDLL(gmix_amd.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in gmix_amd.ABI_SYMBOLS, n
        getattr(L, n)


def _create(models, n_models, cap, S):
    L = _lib.lib()
    descs = (_lib.MatchDesc * max(1, len(models)))(*[_lib.MatchDesc(*m) for m in models])
    h = C.c_void_p()
    rc = L.gmx_match_create(C.byref(h), descs, n_models, cap, S, 0)
    if rc == 0:
        L.gmx_match_destroy(h)
    return rc


@pytest.mark.parametrize("models,n,cap,S", [
    ([(16, 5, 0)], 0, 1024, 1),                              # K = 0
    ([(16, 5, i) for i in range(9)], 9, 1024, 1),            # K = 9
    ([(0, 5, 0)], 1, 1024, 1),                               # table_size 0
    ([(16, 5, 0)], 1, 1024, 0), ([(16, 5, 0)], 1, 1024, -3),  # S <= 0
    ([(16, 5, 0), (16, 5, 0)], 2, 1024, 1),                  # two models on one slot
    ([(16, 5, 0)], 1, 1 << 32, 1),                           # a history that u32 pointers cannot address
])
def test_bad_arguments(models, n, cap, S):
    assert _create(models, n, cap, S) == GMX_ERR_INVALID


def test_no_device_is_an_error_not_a_fallback():
    want = 0 if gmix_amd.device_count() > 0 else GMX_ERR_NO_DEVICE
    assert _create([(16, 5, 0)], 1, 1024, 1) == want


def test_null_handles():
    L = _lib.lib()
    assert L.gmx_match_n_streams(None) == GMX_ERR_INVALID
    assert L.gmx_match_reset(None) == GMX_ERR_INVALID
    assert L.gmx_match_bank_bytes(None) == 0
    assert L.gmx_match_batch_max_bits(None) == 0
    h = C.c_void_p()
    assert L.gmx_match_batch_create(C.byref(h), None, 8) == GMX_ERR_INVALID
    L.gmx_match_destroy(None)
    L.gmx_match_batch_destroy(None)
