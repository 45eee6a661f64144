"""gmix_amd/csrc/gmx_coder.h off the GPU: tests/cpp/test_coder.cpp builds the header for the host (strict floats:
-ffp-contract=off) and
  - decodes oracle.encode(bits, p) of tests/golden/trace_english.npz -- 2 400 bits under the real reference's p -- back
    to those bits;
  - replays tests/golden/decoder_trace.npz, recorded from the reference's own Decoder over a stub Predictor
    (tests/golden/make_decoder_golden.py): x1_, x2_, x_ and the bit after every Decode of an encoded payload, of 64
    random bytes and of a 3-byte input whose reads pass the end; the p hold both clamps and 0.5;
  - checks the PPMd range walk against a plain std::accumulate loop, with denom == 0 and p == 0.5 among the cases.
Exact everywhere."""
import os
import subprocess

import numpy as np

import goldenlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EPS = np.float32(0.0001)


def write_case(d, name, payload, p_u32, bits, state=None):
    np.ascontiguousarray(payload, np.uint8).tofile(os.path.join(d, name + ".in"))
    np.ascontiguousarray(p_u32, "<u4").tofile(os.path.join(d, name + ".p"))
    np.ascontiguousarray(bits, np.uint8).tofile(os.path.join(d, name + ".bits"))
    if state is not None:
        np.ascontiguousarray(state, "<u4").tofile(os.path.join(d, name + ".state"))


def test_decoder_and_range_walk_on_the_host(tmp_path, oracle):
    d = str(tmp_path)
    _, z = goldenlib.load("trace_english")
    bits = np.unpackbits(z["bits"])
    p = z["p"].view(np.float32)
    assert len(bits) == len(p) == 2400
    write_case(d, "english", np.frombuffer(oracle.encode(bits, p), np.uint8), z["p"], bits)
    t = np.load(os.path.join(GOLDEN, "decoder_trace.npz"))
    names = [str(n) for n in t["names"]]
    assert names == ["encoded", "random64", "dry3"]
    assert len(t["random64_input"]) == 64 and len(t["dry3_input"]) == 3
    for n in names:
        pv = set(t[n + "_p"].tolist())
        for v in (EPS, np.float32(1.0) - EPS, np.float32(0.5)):
            assert int(v.view(np.uint32)) in pv, (n, v)
        write_case(d, n, t[n + "_input"], t[n + "_p"], t[n + "_bits"], t[n + "_state"])
    exe = str(tmp_path / "test_coder")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_coder.cpp")])
    r = subprocess.run([exe, d, "english"] + names, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok:") == 6, r.stdout
    lines = {ln.split()[1]: ln for ln in r.stdout.splitlines() if ln.startswith("ok:")}
    assert " 0 shifts past the end" not in lines["dry3"], lines["dry3"]          # the short input does run dry
    assert "64 of 64 input bytes read" in lines["random64"], lines["random64"]
