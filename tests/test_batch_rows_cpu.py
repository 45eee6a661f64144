"""The record batches off the GPU: tests/cpp/test_batch_rows.cpp drives gmix_amd/csrc/gmx_batch_rows.h (the geometry
of a transfer of the first records of every stream, and the column tables of the five batch types) -- the copy plan
replayed with memcpy over every small shape, and the tables' byte sums and allocation sizes against the expressions
the per-bank copies of the batch code carried, which is what keeps the own-stream threshold where it was."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_rows_and_column_tables(tmp_path):
    exe = str(tmp_path / "test_batch_rows")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "gmix_amd", "csrc"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_batch_rows.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok:") == 6, r.stdout
