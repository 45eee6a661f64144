"""Shared by tests/test_full_cpu.py and tests/test_gpu_full.py: the full drop-in (gmx::GpuMatch beside the mixers, the
Indirect models and the LSTM; dropin/Makefile's *_full* binaries) beside the stock build of the reference, on inputs
that make the Match models work."""
import random

from batched_common import corpus


def match_corpus(n_bytes, seed=1):
    """n_bytes of text in which a block of a few hundred bytes comes three times: once straight after itself with three
    bytes changed (matches grow past 64 bits, so longest_match reaches 2 and bytes stay out of the history, and the
    match pointer runs into the end of the history: the reset of match.cpp:42-44), once more behind 48 bytes of noise.
    Short inputs get a shorter block; below 40 bytes it is plain text."""
    rng = random.Random(seed)
    if n_bytes < 40:
        return corpus(n_bytes, 100 * seed)
    block_len = min(400, n_bytes // 5)
    head_len = min(300, n_bytes // 10)
    block = bytearray(corpus(block_len, 9000 + 1000 * seed))
    changed = bytearray(block)
    for pos in rng.sample(range(block_len // 4, block_len), 3):
        changed[pos] ^= 0x55
    noise = bytes(rng.randrange(256) for _ in range(min(48, n_bytes // 20)))
    data = corpus(head_len, 500 * seed) + bytes(block) + bytes(changed) + noise + bytes(block)
    data += corpus(max(0, n_bytes - len(data)), 20000 + 700 * seed)
    return data[:n_bytes]


def stock_history_column(stock_dir):
    """The `match history` column (LongTermMemory::history.size(), predictor.cpp:500) of the STOCK build's memory.tsv."""
    rows = [r.split("\t") for r in (stock_dir / "analysis" / "memory.tsv").read_text().splitlines() if r.strip()]
    assert rows[0][-1].strip() == "match history", rows[0][-3:]
    return [int(r[-1]) for r in rows[1:]]


def corpus_exercises_match(stock_dir, n_bytes):
    """Rejects a corpus on which the Match models did nothing worth comparing: by the stock build's own table, bytes
    were kept out of the history (longest_match >= 2 happened), and the history is not empty."""
    col = stock_history_column(stock_dir)
    assert len(col) > 0
    assert 0 < col[-1] < n_bytes, f"match history {col[-1]} of {n_bytes} bytes: the corpus does not exercise the Match models"
    return col
