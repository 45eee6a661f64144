"""The Match group checkpoint (gmx_match_group_export / gmx_match_group_import, gmx_match_ckpt.hip) as far as a machine
without a GPU can check it: the two symbols are declared, exported and bound, a null handle is refused, the Python
surface exists and knows the kernels' chunk length, and none of the kernels uses scratch memory."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib, match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gmx_match_group_export", "gmx_match_group_import")
KERNELS = ["count", "history", "pack", "restore", "scatter", "zero"]


def test_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gmxmix.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(gmix_amd.LIB_PATH)
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/gmxmix.h"
        assert hasattr(raw, name), f"{name} is not exported by libgmxmix.so"
        assert name in gmix_amd.ABI_SYMBOLS
        assert getattr(L, name).argtypes, f"{name} has no argtypes in gmix_amd/_lib.py"
    assert len(L.gmx_match_group_export.argtypes) == 7 and len(L.gmx_match_group_import.argtypes) == 6
    assert callable(match.MatchGroup.export_all) and callable(match.MatchGroup.import_all)
    # a null handle is an argument error in both calls
    off = (C.c_size_t * 2)()
    buf = (C.c_uint8 * 16)()
    assert L.gmx_match_group_export(None, 0, 1, None, 0, off, None) == -1
    assert L.gmx_match_group_import(None, 0, 1, buf, off, buf) == -1
    # the launch counter of the GPU tests is an exported debug hook, not part of the header
    assert hasattr(raw, "gmx_debug_match_group_ops") and "gmx_debug_match_group_ops" not in header
    # the chunk length the tests aim their keys at is the kernels'
    h = open(os.path.join(ROOT, "gmix_amd", "csrc", "gmx_match.h")).read()
    assert int(re.search(r"#define\s+GMX_MATCH_CKPT_CHUNK\s+(\d+)", h).group(1)) == match.CKPT_CHUNK == 16384


def test_checkpoint_kernels_use_no_scratch():
    src = os.path.join(ROOT, "gmix_amd", "csrc")
    out = subprocess.run(
        ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
         "-fno-gpu-flush-denormals-to-zero", "-c", os.path.join(src, "gmx_match_ckpt.hip"), "-o", "/dev/null",
         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=src)
    report = out.stderr + out.stdout
    kernels = {}
    for blk in re.split(r"Function Name: ", report)[1:]:
        name = re.search(r"gmx_match_gck_(\w+?)_kernel", blk)
        if not name:
            continue
        kernels[name.group(1)] = tuple(int(re.search(pat + r": (\d+)", blk).group(1))
                                       for pat in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill"))
    assert sorted(kernels) == KERNELS, (sorted(kernels), report[-2000:])
    for k, (scratch, spill) in kernels.items():
        assert scratch == 0 and spill == 0, kernels
