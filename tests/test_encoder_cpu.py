"""gmix_amd/csrc/gmx_encoder.h off the GPU: tests/cpp/test_encoder.cpp builds the header for the host (strict floats:
-ffp-contract=off) and replays tests/golden/encoder_trace.npz, recorded from the reference's own Encoder
(tests/golden/make_encoder_golden.py), state by state and byte by byte: trace_english's 2 400 bits, 2 000 bits of the
operand mixture, and a run resumed from a state whose first bit emits four bytes.  It decodes its own output back to the
bits with gmx_coder_decode, and checks 10^6 random tuples of state, p and bit against the reference's loop spelled out.
PyEncoder (tests/encoder_common.py), which the GPU tests take their expected values from, replays the same fixture, and
equals oracle.encode on whole outputs.  Exact everywhere."""
import os
import subprocess

import numpy as np

import encoder_common as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ["english", "mixture", "resumed"]


def fixture():
    t = np.load(os.path.join(GOLDEN, "encoder_trace.npz"))
    assert [str(n) for n in t["names"]] == NAMES
    return t


def test_fixture_cases():
    t = fixture()
    assert len(t["english_bits"]) == 2400 and len(t["mixture_bits"]) == 2000
    assert tuple(t["resumed_start"]) == ec.FOUR and t["resumed_count"][0] == 4 and t["resumed_bits"][0] == 1
    pv = set(t["mixture_p"].tolist())
    for v in (0.0, 1.0, 0.5, ec.LO, ec.HI):
        assert int(np.float32(v).view(np.uint32)) in pv, v


def test_header_on_the_host(tmp_path):
    t = fixture()
    d = str(tmp_path)
    for n in NAMES:
        for key, ext, dt in (("bits", "bits", np.uint8), ("p", "p", "<u4"), ("state", "state", "<u4"),
                             ("count", "count", "<u4"), ("output", "out", np.uint8), ("start", "start", "<u4")):
            np.ascontiguousarray(t[n + "_" + key], dt).tofile(os.path.join(d, n + "." + ext))
    exe = str(tmp_path / "test_encoder")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_encoder.cpp")])
    r = subprocess.run([exe, d] + NAMES, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok:") == 4, r.stdout
    lines = {ln.split()[1]: ln for ln in r.stdout.splitlines() if ln.startswith("ok:")}
    assert "2400 bits decoded back" in lines["english"] and "2000 bits decoded back" in lines["mixture"], r.stdout


def test_pyencoder_replays_the_fixture_and_equals_the_oracle(oracle):
    t = fixture()
    for n in NAMES:
        e = ec.PyEncoder(t[n + "_start"])
        bits, p = t[n + "_bits"], t[n + "_p"].view(np.float32)
        for i in range(len(bits)):
            k = e.encode(int(bits[i]), p[i])
            assert 0 <= k <= 4
            assert e.state == tuple(int(v) for v in t[n + "_state"][i]) and len(e.out) == t[n + "_count"][i], (n, i)
        assert 1 <= e.flush() <= 5
        assert bytes(e.out) == t[n + "_output"].tobytes(), n
        if n != "resumed":
            assert oracle.encode(bits, p) == t[n + "_output"].tobytes(), n


def test_densest_sustained_output_is_two_bytes_per_bit():
    for bit, p in ((1, 0.0), (0, 1.0)):
        assert set(ec.emit_counts([bit] * 400, [np.float32(p)] * 400)[2:].tolist()) == {2}
