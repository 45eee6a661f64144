"""The *_dev drop-in's HOST logic without a GPU: gmx::GpuBasicContexts / GpuIntervalContext / GpuSkipContext /
GpuIndirectHash and gmx::GpuCtxBank -- finding the bank by the address of an output field, the derived descriptor list
and routes, the per-bit surface, the bank's place in MixerPool's ring and in the lock step, persistence through the
.short stream -- inside builds of the reference whose C-ABI calls are answered by the oracle and, for gmx_ctx_*, by
tests/helpers/ctx_ref.c (tests/cpp/gmx_abi_oracle_shim4.c; test-only, the product has no CPU path), beside the stock
build.  Every input takes both branches of IndirectHash::WriteToDisk at the position that is compared
(tests/dev_common.py).  The same comparisons on an MI355X: tests/test_gpu_dev.py."""
import os
import re
import subprocess

import pytest

from batched_common import compress_pair, gmix, run_many, same_outputs
from dev_common import both_branches, dense_corpus, history_worked, run_testers
from dropin_common import checkpoint_after_batches, compare, exe as exe_path, same_checkpoint
from full_common import corpus_exercises_match


def _skip_unless(*exes):
    for exe in exes:
        if not os.path.exists(exe_path(exe)):
            pytest.skip(f"{exe_path(exe)} not built (needs the reference's sources: make -C oracle/ref_build full && make -C dropin)")


def test_derived_variables_and_routes_are_the_stock_ones(tmp_path):
    """What GpuCtxBank derives from the reference's Predictor -- 38 registered objects, BasicContexts' fields found by
    address among the 33 + 41 + 6 context references of the mixers, Indirect and Match models -- is
    gmix_amd.topology.stock_contexts(): 52 variables in its order and its three route arrays."""
    _skip_unless("gmix_dev_shim")
    from gmix_amd import topology
    src = tmp_path / "in"
    src.write_bytes(b"ab")
    r = subprocess.run([exe_path("gmix_dev_shim"), "-c", str(src), str(tmp_path / "c")], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, GMX_CTX_DESCRIBE="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith("[gmx ctx] ")]
    var = re.compile(r"var (\d+) kind (\d+) index (\d+) num_bits (\d+) n_bytes (\d+) outer (\d+) inner (\d+) table (\d+) bytes([ \d]*) map_div (\d+)")
    got = [var.search(l).groups() for l in lines if " var " in l]
    descs, mixer_route, ind_route, match_route = topology.stock_contexts()
    assert len(descs) == 52 and len(got) == 52
    kinds = {"zero": 0, "bit_context": 1, "recent_byte": 2, "byte_plus_recent": 3, "interval": 4, "skip": 5, "indirect_hash": 6}
    for i, ((name, kind, prm), g) in enumerate(zip(descs, got)):
        g_bytes = [int(x) for x in g[8].split()]
        g = [int(x) for x in g[:8]] + [int(g[9])]
        assert g[0] == i and g[1] == kinds[kind], (name, g)
        if kind in ("recent_byte", "byte_plus_recent"):
            assert g[2] == prm["index"], (name, g)
        if kind == "interval":
            assert g[3] == prm["num_bits"] and g[8] == 256 // (prm["map"][255] + 1), (name, g)
        if kind == "skip":
            assert g_bytes == prm["bytes_to_use"], (name, g_bytes)
        if kind == "indirect_hash":
            assert (g[5], g[7], g[6]) == (prm["outer_order"], prm["table_size"], prm["inner_order"]), (name, g)
    routes = {l.split()[3]: [int(x) for x in l.split()[4:]] for l in lines if " route " in l}
    assert routes == {"mixer": list(mixer_route), "indirect": list(ind_route), "match": list(match_route)}


@pytest.mark.slow
def test_reference_tester_dev_per_bit(tmp_path):
    """The reference's five tests with the 38 context objects behind gmx::GpuCtxBank, per bit: gmx_ctx_forward / _learn
    for every bit, restart from a checkpoint (the nine hash sections read from the .short stream and imported, the board
    rebuilt from the restored ShortTermMemory BEFORE the next bit is folded), restart through Predictor::Copy, decoding
    with restart, generation (Predict after Perceive with no Learn).  Everything it leaves equals the stock build's: the
    .short files hold the nine hash sections -- dense and sparse -- and every context field."""
    _skip_unless("ref_tester_strict", "ref_tester_dev_shim")
    n = 800
    data = dense_corpus(n, 1)
    both_branches(data[:n // 2 + 1])
    stock, dev = run_testers([("ref_tester_strict", 200), ("ref_tester_dev_shim", 200)], data, tmp_path, 1100)
    history_worked(stock, n)
    compare(stock, dev)


def test_dev_batched_cli_both_ways(tmp_path):
    """5 000 bytes: 19 chunks of 2 048 bits and a ragged one through the ring with five banks -- the context bank's
    only record is the coded bit, gmx_ctx_run_ragged writes the routed columns of the three record batches in front of
    the Match bank's run.  Output and both analysis tables equal the stock build's; the stock build decodes the file, and
    the dev build decodes the stock build's through the lock step (the context stage in front of the Match stage)."""
    _skip_unless("gmix_strict", "gmix_dev_batched_shim")
    n = 5000
    data = dense_corpus(n, 1)
    both_branches(data)
    src, stock, dev = compress_pair("gmix_strict", "gmix_dev_batched_shim", data, tmp_path)
    col = corpus_exercises_match(stock, n)
    assert len(set(col)) > 10
    same_outputs(stock, dev)
    gmix("gmix_strict", "-d", dev / "c", stock / "back", stock)
    assert (stock / "back").read_bytes() == src.read_bytes()
    gmix("gmix_dev_batched_shim", "-d", stock / "c", dev / "back", dev)
    assert (dev / "back").read_bytes() == src.read_bytes()


@pytest.mark.parametrize("chunk", [8, 2048])
def test_dev_many_files_ragged_lengths(tmp_path, chunk):
    """Three Predictors on three threads -- each finds its own bank by the address of its own ShortTermMemory -- one
    gmx_ctx of three streams beside the other banks: files of 1 / 613 / 1 500 bytes end in different rounds.  Then the
    three coded files restored together in lock step."""
    _skip_unless("gmix_strict", "gmix_dev_many_shim")
    files = []
    for k, n in enumerate((1, 613, 1500)):
        f = tmp_path / f"f{k}"
        f.write_bytes(dense_corpus(n, 2 + k))
        files.append(f)
    st = run_many("gmix_dev_many_shim", files, tmp_path / "out", chunk)
    assert st["failed"] == 0 and st["device_bits"] == 8 * (1 + 613 + 1500)
    for k, f in enumerate(files):
        gmix("gmix_strict", "-c", f, tmp_path / f"ref{k}", tmp_path)
        assert (tmp_path / f"ref{k}").read_bytes() == (tmp_path / "out" / f"{k}.gmix").read_bytes(), f"file {k}"
    st = run_many("gmix_dev_many_shim", [tmp_path / "out" / f"{k}.gmix" for k in range(3)], tmp_path / "back", chunk,
                  extra=("-d", "--cpus", "2"))
    assert st["mode"] == "decompress" and st["failed"] == 0
    for k, f in enumerate(files):
        assert (tmp_path / "back" / f"{k}.out").read_bytes() == f.read_bytes(), f"file {k}"


def test_dev_state_left_behind_equals_the_per_bit_loop(tmp_path):
    """Predictor::WriteCheckpoint straight after a run-ahead pass over 401 bytes (chunks of 1 000 bits, a ragged last
    one) equals the checkpoint the stock tester writes after the same bytes through its per-bit loop: the bank left
    behind inside a byte stream, its 38 values brought home into ShortTermMemory, its nine hash sections written into the
    .short stream by gmx::GpuIndirectHash from one gmx_ctx_export."""
    _skip_unless("ref_tester_strict", "gmix_dev_batched_ckpt_shim")
    n = 800
    data = dense_corpus(n, 1)
    both_branches(data[:n // 2 + 1])
    (stock,) = run_testers([("ref_tester_strict", 0)], data, tmp_path, 1100)
    ck = checkpoint_after_batches("gmix_dev_batched_ckpt_shim", stock, n, 1000, tmp_path)
    same_checkpoint(os.path.join(stock, "checkpoint"), ck)
