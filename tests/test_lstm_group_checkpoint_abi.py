"""The LSTM group checkpoint (gmx_lstm_group_export / gmx_lstm_group_import, gmx_lstm_ckpt.hip) as far as a machine
without a GPU can check it: the two symbols are declared (in the extension header include/gmxmix_lstm_group.h, which
leaves the pinned list of include/gmxmix.h as it is), exported and bound, a null handle is refused, the Python surface
exists, the header compiles as C and as C++, and neither kernel uses scratch memory or spills."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib, lstm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gmx_lstm_group_export", "gmx_lstm_group_import")


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gmxmix_lstm_group.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(gmix_amd.LIB_PATH)
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/gmxmix_lstm_group.h"
        assert hasattr(raw, name), f"{name} is not exported by libgmxmix.so"
        assert name in _lib.ABI_SYMBOLS_LSTM_GROUP and name not in gmix_amd.ABI_SYMBOLS
        assert getattr(L, name).argtypes, f"{name} has no argtypes in gmix_amd/_lib.py"
    assert len(L.gmx_lstm_group_export.argtypes) == 9 and len(L.gmx_lstm_group_import.argtypes) == 7
    assert callable(lstm.LstmGroup.export_all) and callable(lstm.LstmGroup.import_all)
    # a null handle is an argument error in both calls; the strides are filled all the same
    nl, ns = C.c_size_t(0), C.c_size_t(0)
    assert L.gmx_lstm_group_export(None, 0, 1, None, 0, None, 0, C.byref(nl), C.byref(ns)) == -1
    assert (nl.value, ns.value) == (5560200, 1458256)
    assert L.gmx_lstm_group_export(None, 0, 1, None, 0, None, 0, None, None) == -1
    assert L.gmx_lstm_group_import(None, 0, 1, None, 0, None, 0) == -1


def test_extension_header_compiles_as_c_and_cxx(tmp_path):
    for compiler, ext in (("gcc", "c"), ("g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "gmxmix_lstm_group.h"\n'
                       'int (*p_export)(gmx_lstm*, int, int, void*, size_t, void*, size_t, size_t*, size_t*) = '
                       'gmx_lstm_group_export;\n'
                       'int (*p_import)(gmx_lstm*, int, int, const void*, size_t, const void*, size_t) = '
                       'gmx_lstm_group_import;\n')
        subprocess.check_call([compiler, "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / ("inc_" + ext + ".o"))])


def test_checkpoint_kernels_use_no_scratch():
    src = os.path.join(ROOT, "gmix_amd", "csrc")
    out = subprocess.run(
        ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
         "-fno-gpu-flush-denormals-to-zero", "--cuda-device-only", "-c", os.path.join(src, "gmx_lstm_ckpt.hip"),
         "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=src)
    report = out.stderr + out.stdout
    kernels = {}
    for blk in re.split(r"Function Name: ", report)[1:]:
        name = re.search(r"gmx_lstm_ckpt_(\w+?)_kernel", blk)
        if not name:
            continue
        kernels[name.group(1)] = tuple(int(re.search(pat + r": (\d+)", blk).group(1))
                                       for pat in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill", r"SGPRs Spill"))
    assert sorted(kernels) == ["pack", "scatter"], (sorted(kernels), report[-2000:])
    for k, (scratch, vspill, sspill) in kernels.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, kernels
