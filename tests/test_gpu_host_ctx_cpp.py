"""gmx::CtxBank (gmix_amd/host/gmx_models.h), the C++ owner of a context bank: compiled with g++ against libgmxmix.so
and run on the GPU box over sections and boards the Python CtxGroup wrote (the owner has no run surface)."""
import ctypes as C
import os
import subprocess

import pytest

import ctx_common as cc
from gmix_amd._lib import CtxDesc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 4                                             # kS of tests/cpp/test_host_ctx.cpp


def test_cpp_ctx_bank_group_checkpoint(gpu, tmp_path):
    f = cc.fixture("ctx_tiny")
    bits = [0, 300, 605, 800]                     # never run; a few hundred bits, one position inside a byte
    g = gpu.CtxGroup(f.descs, S)
    b = gpu.CtxBatch(g, max(bits), values=False)
    for s in range(S):
        o = 8 * 400 * s
        b.bits[s, :bits[s]] = f.bits[o:o + bits[s]]
    b.upload(max(bits))
    g.run_ragged(b, bits)
    b.wait()
    b.close()
    (tmp_path / "descs.bin").write_bytes(bytes((CtxDesc * f.V)(*f.descs)))
    for s in range(S):
        r = cc.Ref(f.descs)
        r.run(f.bits[8 * 400 * s:8 * 400 * s + bits[s]], values=False)
        sec, _ = g.export(s)
        assert sec == r.export()[0] and cc.board_bytes(g.blackboard(s)) == cc.board_bytes(r.board()), s
        (tmp_path / f"sec{s}.bin").write_bytes(sec)
        (tmp_path / f"board{s}.bin").write_bytes(cc.board_bytes(g.blackboard(s)))
    g.close()
    assert C.sizeof(CtxDesc) * f.V == (tmp_path / "descs.bin").stat().st_size
    exe = str(tmp_path / "test_host_ctx")
    subprocess.check_call([
        "g++", "-std=c++17", "-Wall", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_host_ctx.cpp"),
        "-L" + os.path.join(ROOT, "gmix_amd"), "-lgmxmix", "-Wl,-rpath," + os.path.join(ROOT, "gmix_amd"),
        "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "Tests passed." in out.stdout, out.stdout + out.stderr
