"""The LSTM group checkpoint's layout description off the GPU: tests/cpp/test_lstm_ckpt_layout.cpp builds the segment
tables of gmix_amd/csrc/gmx_lstm_ckpt.h (which the kernels of gmx_lstm_ckpt.hip walk) over a fabricated bank layout with
a plain C++ compiler and checks them against the two file layouts restated there: exact tiling in order, an injective
map into the bank that never lands on padding, and the offsets the reference's files have."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lstm_ckpt_segment_tables(tmp_path):
    exe = str(tmp_path / "test_lstm_ckpt_layout")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_lstm_ckpt_layout.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok:") == 4, r.stdout
