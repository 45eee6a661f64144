"""gmx_indirect_attach_match / gmx_chain_forward_match: declared in include/gmxmix.h, listed in ABI_SYMBOLS and
exported by libgmxmix.so; NULL handles are refused; and the resource report of the per-bit session kernel of the
Indirect models, which hosts the Match models in lanes 56..63 (gmx_indirect_session_kernel<WITH_MATCH>): no scratch in
either build, and no LDS beyond what the build without them has.  The report of the Match lock step's other two hosts
(make report-match-step) must still say what tests/test_chainstep_match_abi.py asserts of it."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gmx_indirect_attach_match", "gmx_chain_forward_match"]
GMX_ERR_INVALID = -1


def report(target):
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "gmix_amd", "csrc"), target], check=True,
                         capture_output=True, text=True).stdout
    kernels, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        m = re.search(r"(ScratchSize|LDS Size|VGPRs)[^:]*: (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    return kernels


def test_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "gmxmix.h")).read()
    L = C.CDLL(gmix_amd.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in gmix_amd.ABI_SYMBOLS, n
        getattr(L, n)


def test_null_handles():
    L = _lib.lib()
    assert L.gmx_indirect_attach_match(None, None, None, 0) == GMX_ERR_INVALID
    assert L.gmx_chain_forward_match(None, None, 0, None, None, 0, None, None, 0, None, None, None, None, None, None,
                                     None, None) == GMX_ERR_INVALID


def test_session_kernel_no_scratch_and_no_lds_growth():
    kernels = report("report-ind-session")
    # gmx_indirect_session_kernel<WITH_MATCH>: ILb<match>E in the mangled name
    built = {}
    for k, v in kernels.items():
        m = re.search(r"gmx_indirect_session_kernelILb([01])E", k)
        if m:
            built[int(m.group(1))] = v
    assert sorted(built) == [0, 1], kernels
    assert built[0]["ScratchSize"] == 0 and built[1]["ScratchSize"] == 0, built
    assert built[0]["LDS Size"] == built[1]["LDS Size"], built


def test_the_other_hosts_of_the_match_step_are_as_before():
    kernels = report("report-match-step")
    alone = [v for k, v in kernels.items() if "gmx_match_step_kernel" in k]
    assert len(alone) == 1 and alone[0] == {"VGPRs": alone[0]["VGPRs"], "ScratchSize": 0, "LDS Size": 0}, kernels
    fused = {}
    for k, v in kernels.items():
        m = re.search(r"gmx_indirect_step_kernelILb([01])ELb([01])E", k)
        if m:
            fused[(int(m.group(1)), int(m.group(2)))] = v
    assert sorted(fused) == [(0, 0), (0, 1), (1, 0), (1, 1)], kernels
    for lstm in (0, 1):
        assert fused[(lstm, 1)]["ScratchSize"] == 0 and fused[(lstm, 0)]["ScratchSize"] == 0
        assert fused[(lstm, 1)]["LDS Size"] == fused[(lstm, 0)]["LDS Size"], fused
