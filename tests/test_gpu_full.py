"""The full drop-in on an MI355X: the reference's Predictor with its six Match models behind gmx::GpuMatch as well
(dropin/Makefile: `new Match(` -> `new gmx::GpuMatch(`), so that LSTM, Indirect models, Match models and mixers all
live on the device and the host keeps PPMd, the context hashes and the coder.  Every compressed file, restored file,
checkpoint section and analysis table must equal the stock strict build's byte for byte.  The inputs make the Match
models work (tests/full_common.py) and the tests that read analysis tables prove it from the stock build's own table.
Every subprocess has a time limit of its own; a crash, an abort or a timeout fails the test at once, and nothing more is
started on the device by it."""
import os
import subprocess

import pytest

from batched_common import compress_pair, gmix, need, run_many, same_outputs
from dropin_common import compare, exe as exe_path, run_pair
from full_common import corpus_exercises_match, match_corpus

pytestmark = pytest.mark.gpu


def _tester_history(stock_data, n):
    rows = [r.split("\t") for r in open(os.path.join(stock_data, "memory.tsv")).read().splitlines() if r.strip()]
    assert rows[0][-1].strip() == "match history" and 0 < int(rows[-1][-1]) < n, rows[-1][-1]


def test_reference_tester_full_per_bit_equals_stock(gpu, tmp_path):
    """2 000 bytes / 200 generated through the per-bit surface: gmx_match_forward / _learn for every bit, Copy,
    restart from a checkpoint, generation (Predict after Perceive without Learn: gmx_match_slots_set hands the bit
    over), and the history and match section of every .long written by the reference's own serialiser from the
    staged bank."""
    need("ref_tester_strict", "ref_tester_full")
    da, db = run_pair("ref_tester_strict", "ref_tester_full", 2000, 200, tmp_path, timeout=600)
    _tester_history(da, 2000)
    compare(da, db)


def test_reference_tester_full_run_ahead_equals_stock(gpu, tmp_path):
    """The same with RunCompression running ahead (the Match bank in the ring) and the decode tests on the bank the
    batches left behind."""
    need("ref_tester_strict", "ref_tester_full_batched")
    da, db = run_pair("ref_tester_strict", "ref_tester_full_batched", 2000, 200, tmp_path, timeout=600)
    _tester_history(da, 2000)
    compare(da, db)


def test_gmix_full_cli_compress_and_cross_decompress(gpu, tmp_path):
    """`gmix_full -c` == `gmix_strict -c` on 3 000 bytes, and each build decompresses the OTHER's file."""
    need("gmix_strict", "gmix_full")
    src = tmp_path / "input"
    src.write_bytes(match_corpus(3000, 5))
    out = {}
    for exe in ("gmix_strict", "gmix_full"):
        wd = tmp_path / exe
        wd.mkdir()
        r = subprocess.run([exe_path(exe), "-c", str(src), str(wd / "c")], cwd=wd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
        out[exe] = (wd / "c").read_bytes()
    assert len(out["gmix_strict"]) > 5 and out["gmix_strict"] == out["gmix_full"]
    corpus_exercises_match(tmp_path / "gmix_strict", 3000)
    for exe, other in (("gmix_strict", "gmix_full"), ("gmix_full", "gmix_strict")):
        wd = tmp_path / exe
        r = subprocess.run([exe_path(exe), "-d", str(tmp_path / other / "c"), str(wd / "d")], cwd=wd, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
        assert (wd / "d").read_bytes() == src.read_bytes(), f"{exe} did not restore {other}'s file"


def test_full_run_ahead_and_lock_step(gpu, tmp_path):
    """6 000 bytes: 23 chunks of 2 048 bits and a ragged end through the ring with four banks.  The output and both
    analysis tables equal the stock build's; `gmix_full_batched -d` restores the file through the lock step at S = 1
    (gmx_chainstep with the Match bank attached)."""
    need("gmix_strict", "gmix_full_batched")
    n = 6000
    src, stock, full = compress_pair("gmix_strict", "gmix_full_batched", match_corpus(n, 1), tmp_path)
    col = corpus_exercises_match(stock, n)
    assert len(set(col)) > 10
    same_outputs(stock, full)
    gmix("gmix_full_batched", "-d", full / "c", full / "back", full, timeout=300)
    assert (full / "back").read_bytes() == src.read_bytes()


def test_full_many_files_both_ways(gpu, tmp_path):
    """Four files of 1 / 613 / 1 500 / 3 000 bytes in one pool: compressed side by side (they end in different
    rounds), then restored in lock step.  Outputs equal gmix_strict's, restored files equal the inputs."""
    need("gmix_strict", "gmix_full_many")
    files = []
    for k, n in enumerate((1, 613, 1500, 3000)):
        f = tmp_path / f"f{k}"
        f.write_bytes(match_corpus(n, 2 + k))
        files.append(f)
    st = run_many("gmix_full_many", files, tmp_path / "out", 2048, timeout=300)
    assert st["failed"] == 0 and st["device_bits"] == 8 * (1 + 613 + 1500 + 3000)
    for k, f in enumerate(files):
        gmix("gmix_strict", "-c", f, tmp_path / f"ref{k}", tmp_path)
        assert (tmp_path / f"ref{k}").read_bytes() == (tmp_path / "out" / f"{k}.gmix").read_bytes(), f"file {k}"
    st = run_many("gmix_full_many", [tmp_path / "out" / f"{k}.gmix" for k in range(4)], tmp_path / "back", 2048,
                  timeout=300, extra=("-d",))
    assert st["mode"] == "decompress" and st["failed"] == 0 and st["launches"] >= 8 * 3000 + 1
    for k, f in enumerate(files):
        assert (tmp_path / "back" / f"{k}.out").read_bytes() == f.read_bytes(), f"file {k}"


@pytest.mark.parametrize("mode", ["compress", "decompress"])
def test_history_capacity_is_an_error_status_not_a_fault(gpu, tmp_path, mode):
    """A capacity below what the file needs (100 bytes for 1 500 bytes of text): gmx_match_run / the step refuse on the
    HOST, before anything is queued, with GMX_ERR_INVALID; the shared pool reports it, the job fails and the driver
    exits non-zero -- no signal, no hang.  Nothing is provoked on the device."""
    need("gmix_strict", "gmix_full_many")
    f = tmp_path / "f0"
    f.write_bytes(match_corpus(1500, 3))
    files = [f]
    extra = ("--match-history", "100")
    if mode == "decompress":
        gmix("gmix_strict", "-c", f, tmp_path / "c0", tmp_path)
        files = [tmp_path / "c0"]
        extra = ("-d",) + extra
    r = subprocess.run([exe_path("gmix_full_many"), "-T", "2048", *extra, str(tmp_path / "out")] + [str(x) for x in files],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stdout[-500:], r.stderr[-2000:])   # (an exit status, not a signal)
    assert '"failed": 1' in r.stdout and "invalid" in r.stderr.lower(), (r.stdout[-500:], r.stderr[-1000:])
