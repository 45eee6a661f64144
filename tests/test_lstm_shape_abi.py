"""The shaped LSTM banks (include/gmxmix_lstm_shape.h, gmx_lstm_any.hip) as far as a machine without a GPU can check
them: the new symbols are declared in the extension header -- which leaves the pinned list of include/gmxmix.h as it
is --, exported and bound with the header's signatures, gmx_lstm_shape_supported (host code) accepts exactly the
documented range, the header compiles as C and as C++, and the general kernel uses no scratch memory."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

import gmix_amd
from gmix_amd import _lib, lstm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (return type, number of parameters) as include/gmxmix_lstm_shape.h declares them
DECLARED = {
    "gmx_lstm_shape_supported": ("int", 1),
    "gmx_lstm_create_shaped": ("int", 4),
    "gmx_lstm_get_shape": ("int", 2),
    "gmx_debug_lstm_any_launches": ("int64_t", 1),
}


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gmxmix_lstm_shape.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(gmix_amd.LIB_PATH)
    L = _lib.lib()
    assert sorted(_lib.ABI_SYMBOLS_LSTM_SHAPE) == sorted(DECLARED)
    declared = set(re.findall(r"\b(gmx_\w+)\s*\(", header))
    assert declared == set(DECLARED), declared ^ set(DECLARED)
    for name, (ret, n_args) in DECLARED.items():
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared as {ret} in include/gmxmix_lstm_shape.h"
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert hasattr(raw, name), f"{name} is not exported by libgmxmix.so"
        assert name not in gmix_amd.ABI_SYMBOLS
        assert len(getattr(L, name).argtypes) == n_args, f"{name}: argtypes in gmix_amd/_lib.py"
    assert L.gmx_debug_lstm_any_launches.restype is C.c_int64
    # the struct: two int32 and two floats, in the header's order
    m = re.search(r"typedef\s+struct\s+gmx_lstm_shape\s*\{(.*?)\}\s*gmx_lstm_shape\s*;", header, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == \
        "int32_t num_cells, horizon; float learning_rate, gradient_clip;"
    assert [(n, t) for n, t in _lib.LstmShapeC._fields_] == [
        ("num_cells", C.c_int32), ("horizon", C.c_int32), ("learning_rate", C.c_float), ("gradient_clip", C.c_float)]
    assert C.sizeof(_lib.LstmShapeC) == 16
    # the Python surface
    assert lstm.LstmShape._fields == ("num_cells", "horizon", "learning_rate", "gradient_clip")
    assert isinstance(lstm.LstmGroup.shape, property)
    # null arguments are argument errors, nothing is dereferenced
    h = C.c_void_p()
    assert L.gmx_lstm_create_shaped(C.byref(h), None, 1, 0) == -1 and not h.value
    assert L.gmx_lstm_get_shape(None, C.byref(_lib.LstmShapeC())) == -1
    assert L.gmx_debug_lstm_any_launches(None) == -1
    # an unsupported shape is refused before a device is looked for
    bad = _lib.LstmShapeC(257, 100, 0.03, 10.0)
    assert L.gmx_lstm_create_shaped(C.byref(h), C.byref(bad), 1, 0) == -1 and not h.value


def test_gmxmix_h_pinned_list_is_unchanged():
    assert len(gmix_amd.ABI_SYMBOLS) == len(set(gmix_amd.ABI_SYMBOLS)) == 203
    main = open(os.path.join(ROOT, "include", "gmxmix.h")).read()
    for name in DECLARED:
        assert name not in main
    assert "gmx_lstm_shape" not in main


nan, inf = math.nan, math.inf
SUPPORTED = [
    # cells, horizon, lr, clip, accepted
    (50, 100, 0.03, 10.0, True),       # the stock shape
    (0, 100, 0.03, 10.0, False), (1, 100, 0.03, 10.0, True), (256, 100, 0.03, 10.0, True), (257, 100, 0.03, 10.0, False),
    (-1, 100, 0.03, 10.0, False),
    (50, 1, 0.03, 10.0, False), (50, 2, 0.03, 10.0, True), (50, 256, 0.03, 10.0, True), (50, 257, 0.03, 10.0, False),
    (50, 0, 0.03, 10.0, False),
    (50, 100, 0.0, 10.0, False), (50, 100, -0.03, 10.0, False), (50, 100, nan, 10.0, False), (50, 100, inf, 10.0, False),
    (50, 100, -inf, 10.0, False),
    (50, 100, 0.03, 0.0, False), (50, 100, 0.03, -10.0, False), (50, 100, 0.03, nan, False), (50, 100, 0.03, inf, False),
    (1, 2, 1e-30, 1e-30, True), (256, 256, 5.0, 1e30, True),
]


@pytest.mark.parametrize("cells,horizon,lr,clip,ok", SUPPORTED)
def test_shape_supported(cells, horizon, lr, clip, ok):
    L = _lib.lib()
    s = _lib.LstmShapeC(cells, horizon, lr, clip)
    assert L.gmx_lstm_shape_supported(C.byref(s)) == (1 if ok else 0)
    assert lstm.shape_supported((cells, horizon, lr, clip)) is ok
    assert L.gmx_lstm_shape_supported(None) == 0


def test_extension_header_compiles_as_c_and_cxx(tmp_path):
    for compiler, ext in (("gcc", "c"), ("g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "gmxmix_lstm_shape.h"\n'
                       'int (*p_sup)(const gmx_lstm_shape*) = gmx_lstm_shape_supported;\n'
                       'int (*p_new)(gmx_lstm**, const gmx_lstm_shape*, int, int) = gmx_lstm_create_shaped;\n'
                       'int (*p_get)(const gmx_lstm*, gmx_lstm_shape*) = gmx_lstm_get_shape;\n'
                       'int64_t (*p_cnt)(const gmx_lstm*) = gmx_debug_lstm_any_launches;\n'
                       'gmx_lstm_shape stock = {50, 100, 0.03f, 10.0f};\n')
        subprocess.check_call([compiler, "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                               "-o", str(tmp_path / ("inc_" + ext + ".o"))])


def test_general_kernel_uses_no_scratch():
    src = os.path.join(ROOT, "gmix_amd", "csrc")
    out = subprocess.run(
        ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
         "-fno-gpu-flush-denormals-to-zero", "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-c",
         os.path.join(src, "gmx_lstm_any.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, cwd=src)
    report = out.stderr + out.stdout
    blk = [b for b in re.split(r"Function Name: ", report)[1:] if "gmx_lstm_any_kernel" in b]
    assert len(blk) == 1, report[-2000:]
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk[0]).group(1))
    vspill = int(re.search(r"VGPRs Spill: (\d+)", blk[0]).group(1))
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk[0]).group(1))
    assert scratch == 0 and vspill == 0 and lds <= 65536, blk[0]
