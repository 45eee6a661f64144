"""The PPMd bank (include/gmxmix_ppmd.h, gmx_ppmd.hip) as far as a machine without a GPU can check it: the header
declares exactly ABI_SYMBOLS_PPMD, every name is exported and bound and absent from gmxmix.h; the pinned lists are as
they were; NULL handles and out-of-range parameters give the documented answers before any device is looked for; the
header compiles as C and as C++; the Python surface exists; the state block fits the kernel's LDS budget; and
`make report-ppmd` shows every kernel of gmx_ppmd.hip without scratch and without spills."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib
from gmix_amd.bank import PpmdBatch, PpmdGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GMX_ERR_INVALID = -1


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gmxmix_ppmd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmxmix.h")).read(), flags=re.S)
    raw = C.CDLL(gmix_amd.LIB_PATH)
    L = _lib.lib()
    assert len(_lib.ABI_SYMBOLS_PPMD) == len(set(_lib.ABI_SYMBOLS_PPMD)) == 27
    for name in _lib.ABI_SYMBOLS_PPMD:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/gmxmix_ppmd.h"
        assert not re.search(r"\b" + name + r"\s*\(", base), f"{name} is declared in include/gmxmix.h"
        assert hasattr(raw, name), f"{name} is not exported by libgmxmix.so"
        assert name not in gmix_amd.ABI_SYMBOLS
        assert getattr(L, name).argtypes, f"{name} has no argtypes in gmix_amd/_lib.py"
    declared = set(re.findall(r"\b(gmx_\w+)\s*\(", header))
    assert declared == set(_lib.ABI_SYMBOLS_PPMD), declared ^ set(_lib.ABI_SYMBOLS_PPMD)
    # the pinned lists are as they were
    assert len(gmix_amd.ABI_SYMBOLS) == len(set(gmix_amd.ABI_SYMBOLS)) == 203
    assert len(_lib.ABI_SYMBOLS_DECODER) == 12 and len(_lib.ABI_SYMBOLS_LSTM_SHAPE) == 4
    assert len(_lib.ABI_SYMBOLS_ENCODER) == 15 and len(_lib.ABI_SYMBOLS_ANALYSIS) == 15
    assert _lib.ABI_SYMBOLS_LSTM_GROUP == ["gmx_lstm_group_export", "gmx_lstm_group_import"]
    for m in ("reset", "sync", "run", "feed", "step", "step_launch", "step_wait", "memory_usage", "restores", "launches",
              "close"):
        assert callable(getattr(PpmdGroup, m)), m
    for m in ("upload", "download", "wait", "close"):
        assert callable(getattr(PpmdBatch, m)), m
    assert gmix_amd.PpmdGroup is PpmdGroup and "PpmdGroup" in gmix_amd.__all__ and "PpmdBatch" in gmix_amd.__all__


def test_null_handles_and_refusals_need_no_device():
    L = _lib.lib()
    h = C.c_void_p()
    n = (C.c_uint64 * 1)(1)
    one = (C.c_uint8 * 1)(0)
    assert L.gmx_ppmd_create(None, 1, 20, 1, 0) == GMX_ERR_INVALID
    # out of range: refused before a device is looked for
    for S, order, mb, dev in ((0, 20, 1, 0), (1, 1, 1, 0), (1, 0, 1, 0), (1, 65, 1, 0), (1, 20, 0, 0), (1, 20, 4096, 0),
                              (1, 20, 1, -1)):
        assert L.gmx_ppmd_create(C.byref(h), S, order, mb, dev) == GMX_ERR_INVALID, (S, order, mb, dev)
        assert not h.value
    L.gmx_ppmd_destroy(None)
    L.gmx_ppmd_batch_destroy(None)
    assert L.gmx_ppmd_n_streams(None) == GMX_ERR_INVALID
    assert L.gmx_ppmd_bank_bytes(None) == 0 and L.gmx_ppmd_batch_max_bytes(None) == 0
    assert L.gmx_ppmd_reset(None, -1) == GMX_ERR_INVALID and L.gmx_ppmd_sync(None) == GMX_ERR_INVALID
    assert L.gmx_ppmd_batch_create(C.byref(h), None, 8) == GMX_ERR_INVALID and not h.value
    assert L.gmx_ppmd_batch_create(None, None, 8) == GMX_ERR_INVALID
    for name in ("bytes", "ppm", "predictions", "active", "used"):
        assert getattr(L, "gmx_ppmd_batch_" + name)(None) is None, name
    assert L.gmx_ppmd_batch_upload(None, 1) == GMX_ERR_INVALID
    assert L.gmx_ppmd_batch_download(None, 1, 7) == GMX_ERR_INVALID
    assert L.gmx_ppmd_batch_wait(None) == GMX_ERR_INVALID
    assert L.gmx_ppmd_run(None, None, 1, None) == GMX_ERR_INVALID
    assert L.gmx_ppmd_run_ragged(None, None, n) == GMX_ERR_INVALID
    assert L.gmx_ppmd_feed(None, None, 1, None, None, 0) == GMX_ERR_INVALID
    assert L.gmx_ppmd_step_launch(None, one, one) == GMX_ERR_INVALID
    assert L.gmx_ppmd_step_wait(None) == GMX_ERR_INVALID and L.gmx_ppmd_step(None, one, one) == GMX_ERR_INVALID
    assert L.gmx_ppmd_step_ppm(None) is None
    assert L.gmx_ppmd_memory_usage(None, 0) == 0 and L.gmx_ppmd_restores(None, 0) == -1
    assert L.gmx_debug_ppmd_launches(None) == GMX_ERR_INVALID


def test_extension_header_compiles_as_c_and_cxx(tmp_path):
    for compiler, ext in (("gcc", "c"), ("g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "gmxmix_ppmd.h"\n'
                       'unsigned what = GMX_PPMD_PPM | GMX_PPMD_PREDICTIONS | GMX_PPMD_USED;\n'
                       'int (*p_create)(gmx_ppmd**, int, int, int, int) = gmx_ppmd_create;\n'
                       'int (*p_run)(gmx_ppmd*, gmx_ppmd_batch*, uint64_t, float*) = gmx_ppmd_run;\n'
                       'int (*p_ragged)(gmx_ppmd*, gmx_ppmd_batch*, const uint64_t*) = gmx_ppmd_run_ragged;\n'
                       'int (*p_feed)(gmx_ppmd*, gmx_ppmd_batch*, uint64_t, gmx_lstm_batch*, gmx_batch*, int) = '
                       'gmx_ppmd_feed;\n'
                       'int (*p_step)(gmx_ppmd*, const uint8_t*, const uint8_t*) = gmx_ppmd_step;\n'
                       'const float* (*p_ppm)(gmx_ppmd*) = gmx_ppmd_step_ppm;\n'
                       'int64_t (*p_restores)(gmx_ppmd*, int) = gmx_ppmd_restores;\n')
        subprocess.check_call([compiler, "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / ("inc_" + ext + ".o"))])


def test_ppmd_kernels_have_no_scratch_and_no_spills():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gmix_amd", "csrc"), "report-ppmd"],
                         check=True, capture_output=True, text=True).stdout
    kernels, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        m = re.search(r"(ScratchSize|VGPRs Spill|SGPRs Spill|LDS Size)[^:]*: (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    src = open(os.path.join(ROOT, "gmix_amd", "csrc", "gmx_ppmd.hip")).read()
    defined = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\(\d+\)\s+)?(\w+)\s*\(", src))
    assert defined == {"gmx_ppmd_kernel", "gmx_ppmd_init_kernel", "gmx_ppmd_feed_kernel"}, defined
    for k in defined:
        got = [v for n, v in kernels.items() if re.search(r"\d" + k + r"(?!_)\d*[A-Z0-9]", n) or n == k]
        assert len(got) == 1, (k, kernels)
        assert {x: got[0][x] for x in ("ScratchSize", "VGPRs Spill", "SGPRs Spill")} == \
            {"ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0}, (k, got)
        assert got[0]["LDS Size"] <= 16384, (k, got)      # the state block and the distribution: ten blocks a CU
