"""The device analysis averages (include/gmxmix_analysis.h, gmx_analysis.hip) as far as a machine without a GPU can check
them: the header declares exactly ABI_SYMBOLS_ANALYSIS, every name is exported and bound and absent from gmxmix.h; the
pinned lists are as they were; NULL handles give the documented answers; the header compiles as C and as C++; the Python
surface exists; and `make report-analysis` shows every kernel of gmx_analysis.hip without scratch and without spills."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib
from gmix_amd.bank import Analysis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GMX_ERR_INVALID = -1


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gmxmix_analysis.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmxmix.h")).read(), flags=re.S)
    raw = C.CDLL(gmix_amd.LIB_PATH)
    L = _lib.lib()
    assert len(_lib.ABI_SYMBOLS_ANALYSIS) == len(set(_lib.ABI_SYMBOLS_ANALYSIS)) == 15
    for name in _lib.ABI_SYMBOLS_ANALYSIS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/gmxmix_analysis.h"
        assert not re.search(r"\b" + name + r"\s*\(", base), f"{name} is declared in include/gmxmix.h"
        assert hasattr(raw, name), f"{name} is not exported by libgmxmix.so"
        assert name not in gmix_amd.ABI_SYMBOLS
        assert getattr(L, name).argtypes, f"{name} has no argtypes in gmix_amd/_lib.py"
    declared = set(re.findall(r"\b(gmx_\w+)\s*\(", header))
    assert declared == set(_lib.ABI_SYMBOLS_ANALYSIS), declared ^ set(_lib.ABI_SYMBOLS_ANALYSIS)
    # the pinned lists are as they were
    assert len(gmix_amd.ABI_SYMBOLS) == len(set(gmix_amd.ABI_SYMBOLS)) == 203
    assert len(_lib.ABI_SYMBOLS_DECODER) == 12 and len(_lib.ABI_SYMBOLS_LSTM_SHAPE) == 4
    assert len(_lib.ABI_SYMBOLS_ENCODER) == 15
    assert _lib.ABI_SYMBOLS_LSTM_GROUP == ["gmx_lstm_group_export", "gmx_lstm_group_import"]
    for m in ("reset", "set_frequency", "update_batch", "update", "take", "take_launch", "take_wait", "d2h_bytes", "close"):
        assert callable(getattr(Analysis, m)), m
    assert gmix_amd.Analysis is Analysis and "Analysis" in gmix_amd.__all__


def test_null_handles():
    L = _lib.lib()
    n = (C.c_uint64 * 1)(1)
    cols = (C.c_uint32 * 2)(0, 0)
    assert L.gmx_analysis_create(None, 1, cols, 1, 8, 0) == GMX_ERR_INVALID
    L.gmx_analysis_destroy(None)
    assert L.gmx_analysis_reset(None, -1, None, 0) == GMX_ERR_INVALID
    assert L.gmx_analysis_set_frequency(None, -1, 1) == GMX_ERR_INVALID
    assert L.gmx_analysis_update_batch(None, None, n, None) == GMX_ERR_INVALID
    assert L.gmx_analysis_update(None, None, None, 0, n) == GMX_ERR_INVALID
    for name in ("take", "take_launch", "take_wait"):
        assert getattr(L, "gmx_analysis_" + name)(None) == GMX_ERR_INVALID, name
    for name in ("ema", "samples", "sample_bits"):
        assert getattr(L, "gmx_analysis_" + name)(None, 0) is None, name
    assert L.gmx_analysis_bits_seen(None, 0) == 0 and L.gmx_analysis_n_samples(None, 0) == 0
    assert L.gmx_debug_analysis_d2h_bytes(None) == GMX_ERR_INVALID


def test_extension_header_compiles_as_c_and_cxx(tmp_path):
    for compiler, ext in (("gcc", "c"), ("g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "gmxmix_analysis.h"\n'
                       'gmx_analysis_column col = {GMX_AN_FINAL_P, 0};\n'
                       'int (*p_create)(gmx_analysis**, int, const gmx_analysis_column*, int, uint64_t, int) = '
                       'gmx_analysis_create;\n'
                       'int (*p_reset)(gmx_analysis*, int, const double*, uint64_t) = gmx_analysis_reset;\n'
                       'int (*p_batch)(gmx_analysis*, gmx_batch*, const uint64_t*, float*) = gmx_analysis_update_batch;\n'
                       'int (*p_update)(gmx_analysis*, const float*, const uint8_t*, uint64_t, const uint64_t*) = '
                       'gmx_analysis_update;\n'
                       'const double* (*p_ema)(gmx_analysis*, int) = gmx_analysis_ema;\n'
                       'const uint64_t* (*p_bits)(gmx_analysis*, int) = gmx_analysis_sample_bits;\n')
        subprocess.check_call([compiler, "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / ("inc_" + ext + ".o"))])


def test_analysis_kernels_have_no_scratch_and_no_spills():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gmix_amd", "csrc"), "report-analysis"],
                         check=True, capture_output=True, text=True).stdout
    kernels, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        m = re.search(r"(ScratchSize|VGPRs Spill|SGPRs Spill)[^:]*: (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    src = open(os.path.join(ROOT, "gmix_amd", "csrc", "gmx_analysis.hip")).read()
    defined = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src))
    assert len(defined) == 3 and "gmx_analysis_kernel" in defined, defined
    for k in defined:
        got = [v for n, v in kernels.items() if re.search(r"\d" + k + r"(?!_)\d*[A-Z0-9]", n) or n == k]
        assert got == [{"ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0}], (k, kernels)
