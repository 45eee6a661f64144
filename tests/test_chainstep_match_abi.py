"""gmx_chainstep_attach_match / gmx_chainstep_match_contexts: declared in include/gmxmix.h and exported by
libgmxmix.so; and the resource report of the kernels that host the Match models' lock step (gmx_match_step.h): no
scratch, and no LDS beyond what the Indirect models' step kernel has without them."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gmx_chainstep_attach_match", "gmx_chainstep_match_contexts"]
GMX_ERR_INVALID = -1


def test_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gmxmix.h")).read()
    L = C.CDLL(gmix_amd.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in gmix_amd.ABI_SYMBOLS, n
        getattr(L, n)


def test_null_handles():
    L = _lib.lib()
    assert L.gmx_chainstep_match_contexts(None) is None
    assert L.gmx_chainstep_attach_match(None, None, None, 0) == GMX_ERR_INVALID


def test_no_scratch_and_no_lds_growth():
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gmix_amd", "csrc"), "report-match-step"],
                         check=True, capture_output=True, text=True).stdout
    kernels = {}
    name = None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        m = re.search(r"(ScratchSize|LDS Size|VGPRs)[^:]*: (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    alone = [v for k, v in kernels.items() if "gmx_match_step_kernel" in k]
    assert len(alone) == 1 and alone[0] == {"VGPRs": alone[0]["VGPRs"], "ScratchSize": 0, "LDS Size": 0}, kernels
    # gmx_indirect_step_kernel<WITH_LSTM, WITH_MATCH>: ILb<lstm>ELb<match>E in the mangled name
    fused = {}
    for k, v in kernels.items():
        m = re.search(r"gmx_indirect_step_kernelILb([01])ELb([01])E", k)
        if m:
            fused[(int(m.group(1)), int(m.group(2)))] = v
    assert sorted(fused) == [(0, 0), (0, 1), (1, 0), (1, 1)], kernels
    for lstm in (0, 1):
        assert fused[(lstm, 1)]["ScratchSize"] == 0 and fused[(lstm, 0)]["ScratchSize"] == 0
        assert fused[(lstm, 1)]["LDS Size"] == fused[(lstm, 0)]["LDS Size"], fused
