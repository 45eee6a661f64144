"""The *_dev drop-in on an MI355X: the reference's Predictor with its 38 context objects behind gmx::GpuCtxBank as well
(dropin/Makefile: `new IntervalContext(` / `new SkipContext(` / `new IndirectHash(` / `new BasicContexts(` ->
gmx::Gpu...), so that the host keeps no hash table and computes no context hash.  Every compressed file, restored file,
checkpoint section and analysis table must equal the stock strict build's byte for byte.  The inputs take both branches
of IndirectHash::WriteToDisk at the compared checkpoint (tests/dev_common.py), and each test asserts that before it
compares anything.  Every subprocess has a time limit of its own; a crash, an abort or a timeout fails the test at once,
and nothing more is started on the device by it; at most two processes run at a time."""
import os
import subprocess

import pytest

from batched_common import compress_pair, gmix, need, run_many, same_outputs
from dev_common import both_branches, dense_corpus, history_worked, run_testers
from dropin_common import checkpoint_after_batches, compare, exe as exe_path, same_checkpoint
from full_common import corpus_exercises_match

pytestmark = pytest.mark.gpu

N = 2000   # the tester's input: the ring of 1 000 bytes wraps at byte 1 000, the checkpoint is at byte 1 001


def test_reference_tester_dev_per_bit_equals_stock(gpu, tmp_path):
    """2 000 bytes / 200 generated through the per-bit surface: gmx_ctx_learn / gmx_ctx_forward for every bit, Copy
    (gmx_ctx_copy, the board rebuilt from the copied ShortTermMemory), restart from a checkpoint (gmx_ctx_import of the
    nine sections read from .short, gmx_ctx_blackboard_set), generation (a perceived bit reaches the bank through
    gmx_ctx_learn at the next Predict).  Every .short holds the nine hash sections written from gmx_ctx_export and every
    context field."""
    need("ref_tester_strict", "ref_tester_dev")
    data = dense_corpus(N, 1)
    both_branches(data[:N // 2 + 1])
    da, db = run_testers([("ref_tester_strict", 200), ("ref_tester_dev", 200)], data, tmp_path, timeout=600)
    history_worked(da, N)
    compare(da, db)


def test_reference_tester_dev_run_ahead_equals_stock(gpu, tmp_path):
    """The same with RunCompression running ahead (the context bank in the ring, its values coming back for the
    analysis rows) and the other tests on the bank the batches left behind."""
    need("ref_tester_strict", "ref_tester_dev_batched")
    data = dense_corpus(N, 1)
    both_branches(data[:N // 2 + 1])
    da, db = run_testers([("ref_tester_strict", 200), ("ref_tester_dev_batched", 200)], data, tmp_path, timeout=600)
    history_worked(da, N)
    compare(da, db)


def test_gmix_dev_cli_compress_and_cross_decompress(gpu, tmp_path):
    """`gmix_dev -c` == `gmix_strict -c` on 3 000 bytes, and each build decompresses the OTHER's file."""
    need("gmix_strict", "gmix_dev")
    src = tmp_path / "input"
    data = dense_corpus(3000, 5)
    both_branches(data)   # (no checkpoint is compared here: the tables as the whole input leaves them)
    src.write_bytes(data)
    out = {}
    for exe in ("gmix_strict", "gmix_dev"):
        wd = tmp_path / exe
        wd.mkdir()
        r = subprocess.run([exe_path(exe), "-c", str(src), str(wd / "c")], cwd=wd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
        out[exe] = (wd / "c").read_bytes()
    assert len(out["gmix_strict"]) > 5 and out["gmix_strict"] == out["gmix_dev"]
    corpus_exercises_match(tmp_path / "gmix_strict", 3000)
    for exe, other in (("gmix_strict", "gmix_dev"), ("gmix_dev", "gmix_strict")):
        wd = tmp_path / exe
        r = subprocess.run([exe_path(exe), "-d", str(tmp_path / other / "c"), str(wd / "d")], cwd=wd, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (exe, r.returncode, r.stderr[-2000:])
        assert (wd / "d").read_bytes() == src.read_bytes(), f"{exe} did not restore {other}'s file"


def test_dev_run_ahead_and_lock_step(gpu, tmp_path):
    """6 000 bytes: 23 chunks of 2 048 bits and a ragged end through the ring with five banks.  The output and both
    analysis tables equal the stock build's; `gmix_dev_batched -d` restores the file through the lock step at S = 1
    (gmx_chainstep with the Match bank and the context bank attached)."""
    need("gmix_strict", "gmix_dev_batched")
    n = 6000
    data = dense_corpus(n, 1)
    both_branches(data)   # (likewise)
    src, stock, dev = compress_pair("gmix_strict", "gmix_dev_batched", data, tmp_path)
    col = corpus_exercises_match(stock, n)
    assert len(set(col)) > 10
    same_outputs(stock, dev)
    gmix("gmix_dev_batched", "-d", dev / "c", dev / "back", dev, timeout=300)
    assert (dev / "back").read_bytes() == src.read_bytes()


def test_dev_many_files_both_ways(gpu, tmp_path):
    """Four files of 1 / 613 / 1 500 / 3 000 bytes in one pool: compressed side by side (they end in different
    rounds), then restored in lock step.  Outputs equal gmix_strict's, restored files equal the inputs."""
    need("gmix_strict", "gmix_dev_many")
    files = []
    for k, n in enumerate((1, 613, 1500, 3000)):
        f = tmp_path / f"f{k}"
        f.write_bytes(dense_corpus(n, 2 + k))
        files.append(f)
    st = run_many("gmix_dev_many", files, tmp_path / "out", 2048, timeout=300)
    assert st["failed"] == 0 and st["device_bits"] == 8 * (1 + 613 + 1500 + 3000)
    for k, f in enumerate(files):
        gmix("gmix_strict", "-c", f, tmp_path / f"ref{k}", tmp_path)
        assert (tmp_path / f"ref{k}").read_bytes() == (tmp_path / "out" / f"{k}.gmix").read_bytes(), f"file {k}"
    st = run_many("gmix_dev_many", [tmp_path / "out" / f"{k}.gmix" for k in range(4)], tmp_path / "back", 2048,
                  timeout=300, extra=("-d",))
    assert st["mode"] == "decompress" and st["failed"] == 0 and st["launches"] >= 8 * 3000 + 1
    for k, f in enumerate(files):
        assert (tmp_path / "back" / f"{k}.out").read_bytes() == f.read_bytes(), f"file {k}"


def test_dev_checkpoint_hand_over(gpu, tmp_path):
    """gmix_dev_batched_ckpt after 1 001 bytes in chunks of 1 000 bits, against the stock tester's checkpoint after the
    same bytes: the bank left behind inside a byte stream, brought home (gmx_ctx_blackboard_get), written by the
    reference's serialiser and gmx::GpuIndirectHash's one export."""
    need("ref_tester_strict", "gmix_dev_batched_ckpt")
    data = dense_corpus(N, 1)
    both_branches(data[:N // 2 + 1])
    (stock,) = run_testers([("ref_tester_strict", 0)], data, tmp_path, timeout=600)
    ck = checkpoint_after_batches("gmix_dev_batched_ckpt", stock, N, 1000, tmp_path)
    same_checkpoint(os.path.join(stock, "checkpoint"), ck)
