"""The `.long` section codec off the GPU: tests/cpp/test_sections.cpp drives gmix_amd/host/gmx_sections.h -- the
Indirect, Match and mixer sections encoded and decoded against the expressions the adapters carried by hand (the
sparse / dense rules at both sides of their thresholds), every proper prefix and out-of-range keys refused."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_long_section_codec(tmp_path):
    exe = str(tmp_path / "test_sections")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "gmix_amd", "host"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_sections.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok:") == 4, r.stdout
