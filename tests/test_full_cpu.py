"""The full drop-in's HOST logic without a GPU: gmx::GpuMatch / GpuMatchBank and the Match bank's place in MixerPool's
ring and lock step (gmix_amd/host/gmx_model_adapter.h), the capacity and the `match history` column of gmx_batched.h --
inside builds of the reference whose C-ABI calls are answered by the oracle and, for gmx_match_*, by
tests/helpers/match_ref.c (tests/cpp/gmx_abi_oracle_shim3.c; test-only, the product has no CPU path), beside the stock
build.  Every input makes the Match models work, and each test that reads the analysis tables proves that from the
STOCK build's memory.tsv before it compares anything.  The same comparisons on an MI355X: tests/test_gpu_full.py."""
import os

import pytest

from batched_common import compress_pair, gmix, run_many, same_outputs
from dropin_common import checkpoint_after_batches, compare, exe as exe_path, run_all, same_checkpoint
from full_common import corpus_exercises_match, match_corpus, stock_history_column


def _skip_unless(*exes):
    for exe in exes:
        if not os.path.exists(exe_path(exe)):
            pytest.skip(f"{exe_path(exe)} not built (needs the reference's sources: make -C oracle/ref_build full && make -C dropin)")


def test_full_batched_cli_writes_the_stock_file_and_tables(tmp_path):
    """5 000 bytes with a block that comes three times: 19 chunks of 2 048 bits and a ragged one, the six Match models
    recording {contexts, bit_context, bit} beside the other banks and running in front of the mixers, their
    predictions, active bits and longest_match (gate columns found by address) written into the mixers' records.
    Output and both tables equal the stock build's -- memory.tsv's last column counted from the returned
    longest_match -- the stock build decodes the file, and so does the full build itself, through the lock step."""
    _skip_unless("gmix_strict", "gmix_full_batched_shim")
    n = 5000
    src, stock, full = compress_pair("gmix_strict", "gmix_full_batched_shim", match_corpus(n, 1), tmp_path)
    col = corpus_exercises_match(stock, n)
    assert len(set(col)) > 10   # (the column moves: a constant would compare equal for the wrong reason)
    same_outputs(stock, full)
    gmix("gmix_strict", "-d", full / "c", stock / "back", stock)
    assert (stock / "back").read_bytes() == src.read_bytes()
    gmix("gmix_full_batched_shim", "-d", stock / "c", full / "back", full)
    assert (full / "back").read_bytes() == src.read_bytes()


@pytest.mark.parametrize("chunk", [8, 72, 4096])
def test_full_many_files_ragged_lengths(tmp_path, chunk):
    """Three Predictors on three threads, one gmx_match of three streams beside the group: files of 1 / 613 / 1 500
    bytes end in different rounds; chunks of one byte up to more than the longest file.  Then the three coded files
    restored together in lock step (the Match stage in front of every step)."""
    _skip_unless("gmix_strict", "gmix_full_many_shim")
    files = []
    for k, n in enumerate((1, 613, 1500)):
        f = tmp_path / f"f{k}"
        f.write_bytes(match_corpus(n, 2 + k))
        files.append(f)
    st = run_many("gmix_full_many_shim", files, tmp_path / "out", chunk)
    assert st["failed"] == 0 and st["device_bits"] == 8 * (1 + 613 + 1500)
    for k, f in enumerate(files):
        gmix("gmix_strict", "-c", f, tmp_path / f"ref{k}", tmp_path)
        assert (tmp_path / f"ref{k}").read_bytes() == (tmp_path / "out" / f"{k}.gmix").read_bytes(), f"file {k}"
    st = run_many("gmix_full_many_shim", [tmp_path / "out" / f"{k}.gmix" for k in range(3)], tmp_path / "back", chunk,
                  extra=("-d", "--cpus", "2"))
    assert st["mode"] == "decompress" and st["failed"] == 0
    for k, f in enumerate(files):
        assert (tmp_path / "back" / f"{k}.out").read_bytes() == f.read_bytes(), f"file {k}"


@pytest.mark.slow
def test_reference_tester_full_per_bit(tmp_path):
    """The reference's five tests with the Match models behind gmx::GpuMatch, per bit: compression with analysis,
    restart from a checkpoint (import of the history and match section the reference read), restart through
    Predictor::Copy, decoding with restart, generation (Predict after Perceive with no Learn).  Everything it leaves
    equals the stock build's: the history and match section of every .long, the 11 bytes per model in .short."""
    _skip_unless("ref_tester_strict", "ref_tester_full_shim")
    n = 800
    stock, full = run_all([("ref_tester_strict", 200), ("ref_tester_full_shim", 200)], n, tmp_path)
    rows = [r.split("\t") for r in open(os.path.join(stock, "memory.tsv")).read().splitlines() if r.strip()]
    assert rows[0][-1].strip() == "match history" and 0 < int(rows[-1][-1]) < n, rows[-1][-1]
    compare(stock, full)


def test_full_state_left_behind_equals_the_per_bit_loop(tmp_path):
    """Predictor::WriteCheckpoint straight after a run-ahead pass over 401 bytes (chunks of 1 000 bits, a ragged last
    one) equals the checkpoint the stock tester writes after the same bytes through its per-bit loop: the history and
    match section staged from the bank, the six models' 11 bytes, and the blackboard -- the Match slots, new_bit and
    longest_match brought home."""
    _skip_unless("ref_tester_strict", "gmix_full_batched_ckpt_shim")
    (stock,) = run_all([("ref_tester_strict", 0)], 800, tmp_path)
    ck = checkpoint_after_batches("gmix_full_batched_ckpt_shim", stock, 800, 1000, tmp_path)
    same_checkpoint(os.path.join(stock, "restart"), ck)
