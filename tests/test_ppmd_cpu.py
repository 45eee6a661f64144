"""gmix_amd/csrc/gmx_ppmd.h off the GPU: tests/cpp/test_ppmd.cpp builds the header for the host (strict floats:
-ffp-contract=off) and replays every case of tests/golden/ppmd_trace.npz, recorded from the reference's own ModPPMD
(tests/golden/make_ppmd_golden.py).  Exact everywhere: every recorded float and slot, `used` after every byte, every
running hash, the number of model flushes.  The same program built with -fsanitize=address,undefined runs stand-alone
across the flushes of sym3 and rand256."""
import os
import subprocess

import numpy as np
import pytest

import ppmd_common as pc


@pytest.fixture(scope="module")
def golden():
    return np.load(pc.GOLDEN)


def test_fixture_names_the_cases_and_their_flushes(golden):
    assert [str(n) for n in golden["names"]] == list(pc.CASES)
    for name, (_, n, _, must_flush) in pc.CASES.items():
        assert len(golden[name + "_used"]) == n
        fl = golden[name + "_flushes"].tolist()
        assert fl == pc.flushes(golden[name + "_used"])
        assert bool(fl) == must_flush, name
        assert golden[name + "_rows"].tolist() == pc.full_rows(n, fl).tolist()
        assert len(golden[name + "_hash"]) == n // pc.HASH_EVERY
    assert golden["sym3_flushes"].tolist() == [43747] and golden["rand256_flushes"].tolist() == [47480]
    assert golden["abcd_flushes"].tolist() == [51830]
    u = golden["sym3_used"]
    assert (int(u[43746]), int(u[43747])) == (1048571, 515344)
    u = golden["rand256_used"]
    assert (int(u[47479]), int(u[47480])) == (547920, 89032)      # the allocator gave up with the arena half used


@pytest.mark.parametrize("name", list(pc.CASES))
def test_restatement_replays_the_reference(golden, name):
    _, n, order, _ = pc.CASES[name]
    m = pc.HostModel(order, pc.ARENA_MB)
    r = m.run(pc.case_bytes(name))
    rows = golden[name + "_rows"]
    assert np.array_equal(r["used"], golden[name + "_used"])
    assert np.array_equal(r["ppm"][rows], golden[name + "_ppm"])
    assert np.array_equal(r["pred"][rows, 0], golden[name + "_slot"])
    assert np.array_equal(r["hash"][pc.HASH_EVERY - 1::pc.HASH_EVERY], golden[name + "_hash"])
    assert m.restores == len(golden[name + "_flushes"])
    assert m.memory_usage == int(golden[name + "_used"][-1])
    m.close()


@pytest.mark.parametrize("name,n", [("noisy500", None), ("rand256", 40000)])
def test_arena_size_matters_only_after_a_flush(name, n):
    d = pc.case_bytes(name, n)
    got = []
    for mb in (1, 2, 64):
        m = pc.HostModel(pc.ORDER, mb)
        r = m.run(d, want_ppm=False)
        assert m.restores == 0
        got.append((r["hash"], r["used"], r["pred"]))
        m.close()
    for other in got[1:]:
        for x, y in zip(got[0], other):
            assert np.array_equal(x, y)


def test_refused_parameters():
    L = pc.host_lib()
    for order, mb in ((1, 1), (65, 1), (20, 0), (20, 4096)):
        assert not L.ppmd_host_create(order, mb)


def test_sanitized_program_across_the_flushes(tmp_path, golden):
    exe = str(tmp_path / "test_ppmd_san")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
        "-static-libasan", "-static-libubsan",      # the runtime inside the program: it needs no place in a preload list
        "-Wall", "-I" + os.path.join(pc.ROOT, "gmix_amd", "csrc"), "-o", exe,
        os.path.join(pc.ROOT, "tests", "cpp", "test_ppmd.cpp")])
    for name in ("sym3", "rand256"):
        m = pc.HostModel()
        r = m.run(pc.case_bytes(name), want_ppm=False)
        m.close()
        assert np.array_equal(r["used"], golden[name + "_used"])
        fin, fex = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".expect"))
        pc.case_bytes(name).tofile(fin)
        np.stack([r["used"], r["hash"]], axis=1).astype("<u8").tofile(fex)
        p = subprocess.run([exe, fin, str(pc.ORDER), str(pc.ARENA_MB), fex], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "ok: %d bytes, 1 restores" % len(pc.case_bytes(name)) in p.stdout, p.stdout
        assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr
