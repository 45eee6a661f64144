"""The session mailbox protocol off the GPU: tests/cpp/test_mailbox.cpp drives gmix_amd/csrc/gmx_mailbox.h (the
host's half, which the mixers', the Indirect models' and the LSTM's sessions share) against a thread that plays the
wave -- the time-out and dead-session paths included, which no GPU test may reach."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mailbox_protocol_against_a_thread(tmp_path):
    exe = str(tmp_path / "test_mailbox")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_mailbox.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok:") == 5, r.stdout
