"""gmx_ctx_forward / gmx_ctx_learn / gmx_indirect_attach_ctx / gmx_chain_forward_ctx: declared in include/gmxmix.h,
listed in ABI_SYMBOLS and exported by libgmxmix.so; NULL handles are refused; the command block of the Indirect models'
per-bit session keeps its size with the ctx_what words in it; and the resource report of the session kernel's four
builds and of the one-block per-bit kernel: no scratch, no VGPR spill, scalar registers kept in vector lanes bounded,
no static LDS in the session kernel."""
import ctypes as C
import os
import re
import subprocess

import gmix_amd
from gmix_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gmix_amd", "csrc")
NAMES = ["gmx_ctx_forward", "gmx_ctx_learn", "gmx_indirect_attach_ctx", "gmx_chain_forward_ctx"]
GMX_ERR_INVALID = -1
MB_CMD_BYTES = 672   # sizeof(GmxIndMbCmd) before ctx_what[2] was taken out of its padding


def test_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "gmxmix.h")).read()
    L = C.CDLL(gmix_amd.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in gmix_amd.ABI_SYMBOLS, n
        getattr(L, n)
    assert len(gmix_amd.ABI_SYMBOLS) == len(set(gmix_amd.ABI_SYMBOLS)) == 203
    assert "do not use these banks yet" not in header


def test_null_handles():
    L = _lib.lib()
    assert L.gmx_ctx_forward(None, 0, None, None) == GMX_ERR_INVALID
    assert L.gmx_ctx_learn(None, 0, 0) == GMX_ERR_INVALID
    assert L.gmx_indirect_attach_ctx(None, None, None) == GMX_ERR_INVALID
    assert L.gmx_chain_forward_ctx(None, None, 0, None, None, None, None, 0, None, None, None, None, None, None, None,
                                   None, None, None) == GMX_ERR_INVALID


def test_command_block_keeps_its_size(tmp_path):
    src = tmp_path / "size.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmx_internal.h"\n'
                   'int main() { printf("%zu %zu %zu\\n", sizeof(GmxIndMbCmd), offsetof(GmxIndMbCmd, ctx_what),\n'
                   '                    offsetof(GmxIndMbCmd, match_what)); return 0; }\n')
    exe = tmp_path / "size"
    # (the header's few __host__ __device__ helpers compile as plain functions here)
    subprocess.check_call(["g++", "-std=c++17", "-D__host__=", "-D__device__=", "-I", CSRC, str(src), "-o", str(exe)])
    size, ctx_what, match_what = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert size == MB_CMD_BYTES
    assert ctx_what == match_what + 8 and ctx_what + 8 <= size
    assert re.search(r"static_assert\(sizeof\(GmxIndMbCmd\) == %d" % MB_CMD_BYTES,
                     open(os.path.join(CSRC, "gmx_internal.h")).read())


def test_session_kernel_builds_no_scratch_no_spill_to_memory():
    """All four builds: no scratch, no VGPR spill, no static LDS (the 256-byte stage is dynamic LDS).  The compiler may
    keep scalar registers in the lanes of a vector register (`SGPRs Spill`: the parent's Match build keeps 7 there): that
    costs no memory, and it is held to the 64 lanes of ONE vector register."""
    out = subprocess.run(["make", "-s", "-C", CSRC, "report-ind-session"], check=True, capture_output=True,
                         text=True).stdout
    built = {}
    for block in re.split(r"Function Name: ", out)[1:]:
        m = re.match(r"\S*gmx_indirect_session_kernelILb([01])ELb([01])E", block)
        if not m:
            continue
        fig = {k: int(v) for k, v in re.findall(r"(ScratchSize|LDS Size|VGPRs Spill|SGPRs Spill|VGPRs)[^:\n]*: (\d+)",
                                                 block)}
        built[(int(m.group(1)), int(m.group(2)))] = fig
    assert sorted(built) == [(0, 0), (0, 1), (1, 0), (1, 1)], out
    for key, v in built.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["LDS Size"] == 0, (key, v)
        assert v["SGPRs Spill"] <= 64, (key, v)
        assert v["VGPRs"] <= 256, (key, v)   # (one wave a SIMD at most is ever resident: far inside the 512 of a lone wave)


def test_per_bit_kernel_no_scratch():
    out = subprocess.run(["make", "-s", "-C", CSRC, "report-ctx"], check=True, capture_output=True, text=True).stdout
    blocks = re.split(r"Function Name: ", out)
    mine = [b for b in blocks if b.startswith("_Z18gmx_ctx_bit_kernel")]
    step = [b for b in blocks if b.startswith("_Z19gmx_ctx_step_kernel")]
    assert len(mine) == 1 and len(step) == 1, out
    for b in mine + step:
        assert re.search(r"ScratchSize[^:]*: 0\b", b) and re.search(r"VGPRs Spill: 0\b", b), b
        assert re.search(r"SGPRs Spill: 0\b", b) and re.search(r"LDS Size[^:]*: 256\b", b), b
