"""The context group checkpoint (gmx_ctx_group_export / _import / _blackboard_get / _blackboard_set and
gmx_debug_ctx_group_ops, gmx_ctx_ckpt.hip) as far as a machine without a GPU can check it: the five symbols are
declared, exported and bound, null handles and empty windows are refused, the Python surface exists and knows the
kernels' chunk length, and none of the kernels uses scratch memory."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib, ctx
from gmix_amd._lib import CtxBlackboard
from gmix_amd.ctx import desc_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gmx_ctx_group_export", "gmx_ctx_group_import", "gmx_ctx_group_blackboard_get",
           "gmx_ctx_group_blackboard_set", "gmx_debug_ctx_group_ops")
KERNELS = ["board_gather", "board_scatter", "count", "pack", "scatter", "zero"]
GMX_ERR_INVALID, GMX_ERR_NO_DEVICE = -1, -4


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
    assert [len(getattr(L, n).argtypes) for n in SYMBOLS] == [7, 5, 4, 4, 1]
    for m in ("group_export", "group_sizes", "group_import", "group_blackboards", "set_group_blackboards", "group_ops"):
        assert callable(getattr(ctx.CtxGroup, m)), m
    # the record the board kernels write is the header's struct
    assert C.sizeof(CtxBlackboard) == 1316
    # the chunk length the tests aim their keys at is the kernels'
    h = open(os.path.join(ROOT, "gmix_amd", "csrc", "gmx_ctx.h")).read()
    assert int(re.search(r"#define\s+GMX_CTX_CKPT_CHUNK\s+(\d+)", h).group(1)) == ctx.CKPT_CHUNK == 16384


def test_null_handles_and_empty_windows():
    L = _lib.lib()
    off = (C.c_size_t * 4)()
    buf = (C.c_uint8 * 16)()
    bb = (CtxBlackboard * 1)()
    for count in (1, 0, -1):
        assert L.gmx_ctx_group_export(None, 0, count, None, 0, off, None) == GMX_ERR_INVALID
        assert L.gmx_ctx_group_import(None, 0, count, buf, off) == GMX_ERR_INVALID
        assert L.gmx_ctx_group_blackboard_get(None, 0, count, bb) == GMX_ERR_INVALID
        assert L.gmx_ctx_group_blackboard_set(None, 0, count, bb) == GMX_ERR_INVALID
    assert L.gmx_debug_ctx_group_ops(None) == GMX_ERR_INVALID
    # without a device there is still no bank to call them on: no CPU fallback
    h = C.c_void_p()
    rc = L.gmx_ctx_create(C.byref(h), desc_array([("h", "indirect_hash", dict(outer_order=1, table_size=16,
                                                                              inner_order=1))]), 1, 2, 0)
    if gmix_amd.device_count() == 0:
        assert rc == GMX_ERR_NO_DEVICE and not h.value
        return
    assert rc == 0
    try:
        for count in (0, -1, 3):   # count < 1, and a window that leaves the bank
            assert L.gmx_ctx_group_export(h, 0, count, None, 0, off, None) == GMX_ERR_INVALID
            assert L.gmx_ctx_group_import(h, 0, count, buf, off) == GMX_ERR_INVALID
            assert L.gmx_ctx_group_blackboard_get(h, 0, count, bb) == GMX_ERR_INVALID
            assert L.gmx_ctx_group_blackboard_set(h, 0, count, bb) == GMX_ERR_INVALID
        assert L.gmx_ctx_group_export(h, 2, 1, None, 0, off, None) == GMX_ERR_INVALID
        assert L.gmx_ctx_group_export(h, -1, 1, None, 0, off, None) == GMX_ERR_INVALID
        assert L.gmx_ctx_group_export(h, 0, 1, None, 0, None, None) == GMX_ERR_INVALID
    finally:
        L.gmx_ctx_destroy(h)


def test_checkpoint_kernels_use_no_scratch():
    src = os.path.join(ROOT, "gmix_amd", "csrc")
    out = subprocess.run(
        ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
         "-fno-gpu-flush-denormals-to-zero", "-c", os.path.join(src, "gmx_ctx_ckpt.hip"), "-o", "/dev/null",
         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=src)
    report = out.stderr + out.stdout
    kernels = {}
    for blk in re.split(r"Function Name: ", report)[1:]:
        name = re.search(r"gmx_ctx_gck_(\w+?)_kernel", blk)
        if not name:
            continue
        kernels[name.group(1)] = tuple(int(re.search(pat + r": (\d+)", blk).group(1))
                                       for pat in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill", r"SGPRs Spill"))
    assert sorted(kernels) == KERNELS, (sorted(kernels), report[-2000:])
    for k, v in kernels.items():
        assert v == (0, 0, 0), kernels
