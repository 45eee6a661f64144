"""The group checkpoints' staging off the GPU: tests/cpp/test_ckpt_stage.cpp drives gmix_amd/csrc/gmx_ckpt_stage.h (the
slice plan, the staging buffers and the export / import pipelines that the mixers', the Indirect models' and the
context banks' group checkpoints share) against a fake link whose device runs what was queued only at a wait, or at
once -- so a host buffer read too early or reused too soon shows as wrong bytes, which no GPU test can provoke."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ckpt_staging_against_a_fake_link(tmp_path):
    exe = str(tmp_path / "test_ckpt_stage")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_ckpt_stage.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok:") == 9, r.stdout
