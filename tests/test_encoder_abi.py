"""The device arithmetic encoder (include/gmxmix_encoder.h, gmx_encoder.hip) as far as a machine without a GPU can check
it: the header declares exactly ABI_SYMBOLS_ENCODER, every name is exported and bound and absent from gmxmix.h; the three
pinned lists are as they were; NULL handles give the documented answers; the header compiles as C and as C++; the Python
surface exists; and `make report-encoder` shows every kernel of gmx_encoder.hip without scratch and without spills."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib
from gmix_amd.bank import Encoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GMX_ERR_INVALID = -1


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gmxmix_encoder.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmxmix.h")).read(), flags=re.S)
    raw = C.CDLL(gmix_amd.LIB_PATH)
    L = _lib.lib()
    assert len(_lib.ABI_SYMBOLS_ENCODER) == len(set(_lib.ABI_SYMBOLS_ENCODER)) == 15
    for name in _lib.ABI_SYMBOLS_ENCODER:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/gmxmix_encoder.h"
        assert not re.search(r"\b" + name + r"\s*\(", base), f"{name} is declared in include/gmxmix.h"
        assert hasattr(raw, name), f"{name} is not exported by libgmxmix.so"
        assert name not in gmix_amd.ABI_SYMBOLS
        assert getattr(L, name).argtypes, f"{name} has no argtypes in gmix_amd/_lib.py"
    declared = set(re.findall(r"\b(gmx_\w+)\s*\(", header))
    assert declared == set(_lib.ABI_SYMBOLS_ENCODER), declared ^ set(_lib.ABI_SYMBOLS_ENCODER)
    # the pinned lists are as they were
    assert len(gmix_amd.ABI_SYMBOLS) == len(set(gmix_amd.ABI_SYMBOLS)) == 203
    assert len(_lib.ABI_SYMBOLS_DECODER) == 12 and len(_lib.ABI_SYMBOLS_LSTM_SHAPE) == 4
    for m in ("reset", "state", "encode_batch", "encode", "flush", "take", "total_bytes", "bad_bit", "d2h_bytes", "close"):
        assert callable(getattr(Encoder, m)), m


def test_null_handles():
    L = _lib.lib()
    out = (C.c_uint32 * 2)()
    n = (C.c_uint64 * 1)(1)
    assert L.gmx_encoder_create(None, 1, 8, 0) == GMX_ERR_INVALID
    L.gmx_encoder_destroy(None)
    assert L.gmx_encoder_reset(None, -1, None) == GMX_ERR_INVALID
    assert L.gmx_encoder_state(None, 0, out) == GMX_ERR_INVALID
    assert L.gmx_encoder_encode_batch(None, None, n, None) == GMX_ERR_INVALID
    assert L.gmx_encoder_encode(None, None, None, 0, n) == GMX_ERR_INVALID
    assert L.gmx_encoder_flush(None, None) == GMX_ERR_INVALID
    for name in ("take", "take_launch", "take_wait"):
        assert getattr(L, "gmx_encoder_" + name)(None) == GMX_ERR_INVALID, name
    assert L.gmx_encoder_bytes(None, 0) is None
    assert L.gmx_encoder_n_bytes(None, 0) == 0 and L.gmx_encoder_total_bytes(None, 0) == 0
    assert L.gmx_encoder_bad_bit(None, 0) == GMX_ERR_INVALID
    assert L.gmx_debug_encoder_d2h_bytes(None) == GMX_ERR_INVALID


def test_extension_header_compiles_as_c_and_cxx(tmp_path):
    for compiler, ext in (("gcc", "c"), ("g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "gmxmix_encoder.h"\n'
                       'int (*p_create)(gmx_encoder**, int, uint64_t, int) = gmx_encoder_create;\n'
                       'int (*p_batch)(gmx_encoder*, gmx_batch*, const uint64_t*, float*) = gmx_encoder_encode_batch;\n'
                       'int (*p_encode)(gmx_encoder*, const float*, const uint8_t*, uint64_t, const uint64_t*) = '
                       'gmx_encoder_encode;\n'
                       'const uint8_t* (*p_bytes)(gmx_encoder*, int) = gmx_encoder_bytes;\n'
                       'int64_t (*p_bad)(gmx_encoder*, int) = gmx_encoder_bad_bit;\n')
        subprocess.check_call([compiler, "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / ("inc_" + ext + ".o"))])


def test_encoder_kernels_have_no_scratch_and_no_spills():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gmix_amd", "csrc"), "report-encoder"],
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
    src = open(os.path.join(ROOT, "gmix_amd", "csrc", "gmx_encoder.hip")).read()
    defined = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src))
    assert len(defined) == 5 and "gmx_encoder_kernel" in defined, defined
    for k in defined:
        got = [v for n, v in kernels.items() if re.search(r"\d" + k + r"(?!_)\d*[A-Z0-9]", n) or n == k]
        assert got == [{"ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0}], (k, kernels)
