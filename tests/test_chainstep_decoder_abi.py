"""The device arithmetic decoder of the lock-step chain (include/gmxmix_decoder.h, gmx_coder.hip) as far as a machine
without a GPU can check it: every name of ABI_SYMBOLS_DECODER is declared in the extension header, exported and bound;
include/gmxmix.h's pinned list is as it was; NULL handles are refused; the header compiles as C and as C++; the Python
surface exists; and `make report-coder` shows the two kernels of a byte graph without scratch and without spills."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib
from gmix_amd.bank import ChainStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GMX_ERR_INVALID = -1


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gmxmix_decoder.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    base = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmxmix.h")).read(), flags=re.S)
    raw = C.CDLL(gmix_amd.LIB_PATH)
    L = _lib.lib()
    assert len(_lib.ABI_SYMBOLS_DECODER) == len(set(_lib.ABI_SYMBOLS_DECODER)) == 12
    for name in _lib.ABI_SYMBOLS_DECODER:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/gmxmix_decoder.h"
        assert not re.search(r"\b" + name + r"\s*\(", base), f"{name} is declared in include/gmxmix.h"
        assert hasattr(raw, name), f"{name} is not exported by libgmxmix.so"
        assert name not in gmix_amd.ABI_SYMBOLS
        assert getattr(L, name).argtypes, f"{name} has no argtypes in gmix_amd/_lib.py"
    declared = set(re.findall(r"\b(gmx_\w+)\s*\(", header))
    assert declared == set(_lib.ABI_SYMBOLS_DECODER), declared ^ set(_lib.ABI_SYMBOLS_DECODER)
    assert len(gmix_amd.ABI_SYMBOLS) == len(set(gmix_amd.ABI_SYMBOLS)) == 203   # gmxmix.h's list is as it was
    for m in ("attach_decoder", "set_input", "byte", "decoder_state"):
        assert callable(getattr(ChainStep, m)), m


def test_null_handles():
    L = _lib.lib()
    out = (C.c_uint32 * 4)()
    ms = C.c_float(1.0)
    assert L.gmx_chainstep_attach_decoder(None, 0) == GMX_ERR_INVALID
    assert L.gmx_chainstep_decoder_set_input(None, 0, None, 0, None) == GMX_ERR_INVALID
    assert L.gmx_chainstep_decoder_state(None, 0, out) == GMX_ERR_INVALID
    for name in ("byte", "byte_launch", "byte_wait"):
        assert getattr(L, "gmx_chainstep_" + name)(None) == GMX_ERR_INVALID, name
    assert L.gmx_chainstep_timed_byte(None, C.byref(ms)) == GMX_ERR_INVALID
    for name in ("decoder_ppm", "take", "decoded", "byte_p"):
        assert getattr(L, "gmx_chainstep_" + name)(None) is None, name
    assert L.gmx_debug_chainstep_bit_launches(None) == GMX_ERR_INVALID


def test_extension_header_compiles_as_c_and_cxx(tmp_path):
    for compiler, ext in (("gcc", "c"), ("g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "gmxmix_decoder.h"\n'
                       'int (*p_attach)(gmx_chainstep*, int) = gmx_chainstep_attach_decoder;\n'
                       'int (*p_input)(gmx_chainstep*, int, const void*, size_t, const uint32_t*) = '
                       'gmx_chainstep_decoder_set_input;\n'
                       'int (*p_byte)(gmx_chainstep*) = gmx_chainstep_byte;\n'
                       'const float* (*p_p)(gmx_chainstep*) = gmx_chainstep_byte_p;\n')
        subprocess.check_call([compiler, "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / ("inc_" + ext + ".o"))])


def test_byte_graph_kernels_have_no_scratch_and_no_spills():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gmix_amd", "csrc"), "report-coder"],
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
    for k in ("gmx_coder_step_kernel", "gmx_coder_tail_kernel"):
        got = [v for n, v in kernels.items() if k in n]
        assert got == [{"ScratchSize": 0, "VGPRs Spill": 0, "SGPRs Spill": 0}], (k, kernels)
