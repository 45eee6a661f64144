"""gmx::MatchBank (gmix_amd/host/gmx_models.h), the C++ owner of a Match bank: compiled with g++ against libgmxmix.so
and run on the GPU box over sections the Python MatchGroup wrote (the owner has no run surface yet)."""
import os
import subprocess

import numpy as np
import pytest

import match_common as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES, LIMIT, S = [4096, 100, 40000], 60, 4      # kTables, kLimit, kS of tests/cpp/test_host_match.cpp


def test_cpp_match_bank_group_checkpoint(gpu, tmp_path):
    f = mc.fixture("match_k8")
    bits = [0, 300, 605, 800]                     # never run; a few hundred bits, one position inside a byte
    g = gpu.MatchGroup([(t, LIMIT) for t in TABLES], 1024, S)
    b = gpu.MatchBatch(g, max(bits))
    for s in range(S):
        o = 8 * 400 * s
        b.set_records(s, f.ctx[o:o + bits[s], [4, 1, 7]], f.bc[o:o + bits[s]], f.bits[o:o + bits[s]])
    b.upload(max(bits))
    g.run_ragged(b, np.array(bits, np.uint64))
    b.close()
    for s in range(S):
        l, sh = g.export(stream=s)
        (tmp_path / f"long{s}.bin").write_bytes(l)
        (tmp_path / f"short{s}.bin").write_bytes(sh)
    g.close()
    exe = str(tmp_path / "test_host_match")
    subprocess.check_call([
        "g++", "-std=c++17", "-Wall", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_host_match.cpp"),
        "-L" + os.path.join(ROOT, "gmix_amd"), "-lgmxmix", "-Wl,-rpath," + os.path.join(ROOT, "gmix_amd"),
        "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "Tests passed." in out.stdout, out.stdout + out.stderr
