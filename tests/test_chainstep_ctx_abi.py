"""gmx_chainstep_attach_ctx / gmx_chainstep_commit_bytes / gmx_chainstep_timed_step: declared in include/gmxmix.h, listed in ABI_SYMBOLS and
exported by libgmxmix.so; NULL arguments are refused without a device; and the resource report of the kernel that
hosts the context banks' lock step (gmx_ctx_step.h) shows no scratch."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gmx_chainstep_attach_ctx", "gmx_chainstep_commit_bytes", "gmx_chainstep_timed_step"]
GMX_ERR_INVALID = -1


def test_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gmxmix.h")).read()
    L = C.CDLL(gmix_amd.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in gmix_amd.ABI_SYMBOLS, n
        getattr(L, n)
    assert "gmx_ctx_step_routes" in header


def test_null_arguments():
    L = _lib.lib()
    routes = _lib.CtxStepRoutes()
    assert L.gmx_chainstep_attach_ctx(None, None, None) == GMX_ERR_INVALID
    assert L.gmx_chainstep_attach_ctx(None, None, C.byref(routes)) == GMX_ERR_INVALID
    assert L.gmx_chainstep_commit_bytes(None) == 0
    assert L.gmx_chainstep_timed_step(None, None) == GMX_ERR_INVALID


def test_routes_struct_matches_the_header():
    """Three (pointer, int32) pairs, each padded to 16 bytes."""
    assert C.sizeof(_lib.CtxStepRoutes) == 48
    assert _lib.CtxStepRoutes.n_match_route.offset == 40


def test_step_kernel_has_no_scratch():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gmix_amd", "csrc"), "report-ctx"],
                         check=True, capture_output=True, text=True).stdout
    kernels, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        m = re.search(r"(ScratchSize|LDS Size|VGPRs Spill|SGPRs Spill)[^:]*: (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    step = [v for k, v in kernels.items() if "gmx_ctx_step_kernel" in k]
    assert step == [{"ScratchSize": 0, "LDS Size": 256, "VGPRs Spill": 0, "SGPRs Spill": 0}], kernels
