"""The record batches of the five bank types -- mixers, Indirect models, LSTM, Match models, context variables -- share
one implementation (GmxBatchCore in gmx_capi.cpp over the column tables of gmx_batch_rows.h).  Here each type goes
through what that code decides: the copy of the first n of max records of several streams (the one shape at which
pitch and width differ), the copy on a transfer stream of its own from 256 KiB on, a batch that outlives its bank, and
columns that a flag leaves out.  Results are compared bit for bit with the oracle that the bank's own test file uses."""
import numpy as np
import pytest

import ctx_common as cc
import goldenlib
import match_common as mc
from gmix_amd import GmxError, topology

pytestmark = pytest.mark.gpu

GMX_ERR_INVALID = -1
OWN_STREAM_MIN = 256 * 1024      # kBatchOwnStreamMin
KINDS = ["mixers", "indirect", "lstm", "match", "ctx"]
IND_MODELS = [(256, 0.02), (3, 0.1), (4096, 0.005), (1, 0.5), (65536, 0.02)]
_cache = {}


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def ind_tables():
    _, z = goldenlib.load("ind_tiny_dense")
    return z["ns_next"], z["rm_next"]


def lstm_start_weights(oracle):
    if "w0" not in _cache:
        _cache["w0"] = oracle.LstmModel().weights()
    return _cache["w0"]


class Case:
    """One bank of S streams with `warm` records already run through it (so that the records under test give results
    that differ from stream to stream and from zero), the inputs of the `n` records that follow, and the oracle's
    results for them.  fill(b, s) writes stream s's n records into batch b's host columns; results(b) -> the downloaded
    columns as a list of [S][max][...] arrays; want[s] -> the same columns' first n records for stream s."""

    def __init__(self, gpu, oracle, kind, S, warm, n):
        self.kind, self.S, self.n = kind, S, n
        T = warm + n
        getattr(self, "_" + kind)(gpu, oracle, S, warm, T)
        if warm:
            w = self.batch(warm)
            for s in range(S):
                self.fill(w, s, 0, warm)
            w.upload(warm)
            self.g.run(w, warm)
            w.wait()
            w.close()
        self.at = warm

    def _mixers(self, gpu, oracle, S, warm, T):
        topo = topology.stock(90)
        self.streams = [oracle.synth(90, 33, T, seed=31 + 7 * s, ctx_mode=3, ctx_mod=6, zero_mod=9, bit_mode=1)
                        for s in range(S)]
        self.g = gpu.MixerGroup(topo, S)
        self.batch = lambda m: gpu.Batch(self.g, m, outputs=True, mask=True)
        self.want = []
        for st in self.streams:
            p, o = oracle.Bank(90, topo.skip, topo.mixers).run(*st)
            self.want.append([u32(p[warm:]), u32(o[warm:])])
        self.results = lambda b: [u32(b.p), u32(b.outputs)]

    def _indirect(self, gpu, oracle, S, warm, T):
        tabs = ind_tables()
        self.streams = [oracle.ind_synth(len(IND_MODELS), T, seed=11 + s, ctx_mod=(40, 3, 900, 0)) for s in range(S)]
        self.g = gpu.IndirectGroup(IND_MODELS, tabs[0], tabs[1], S)
        self.batch = lambda m: gpu.IndirectBatch(self.g, m)
        self.want = []
        for st in self.streams:
            p, a = oracle.IndirectBank(IND_MODELS, *tabs).run(*st)
            self.want.append([u32(p[warm:]), a[warm:]])
        self.results = lambda b: [u32(b.predictions), b.active]

    def _lstm(self, gpu, oracle, S, warm, T):
        w0 = lstm_start_weights(oracle)
        self.streams = [oracle.lstm_synth(T, seed=11 + s, mask=15 if s == 1 else 255) for s in range(S)]
        self.g = gpu.LstmGroup(S)
        self.batch = lambda m: gpu.LstmBatch(self.g, m)
        self.want = []
        for s, (ppm, data) in enumerate(self.streams):
            self.g.set_weights(w0, stream=s)
            p, a, c = oracle.LstmModel().run(ppm, data)
            self.want.append([u32(p[warm:]), a[warm:], c[warm:]])
        self.results = lambda b: [u32(b.predictions), b.active, b.contexts]

    def _match(self, gpu, oracle, S, warm, T):
        f = mc.fixture("match_tiny")
        self.streams = [(f.ctx[8 * 61 * s:][:T], f.bc[8 * 61 * s:][:T], f.bits[8 * 61 * s:][:T]) for s in range(S)]
        self.g = gpu.MatchGroup(f.models(), len(f.data) + 64, S)
        self.batch = lambda m: gpu.MatchBatch(self.g, m)
        self.want = []
        for st in self.streams:
            p, a, lm = mc.Ref(f.models()).run(*st)
            self.want.append([p[warm:], a[warm:], lm[warm:]])
        self.results = lambda b: [u32(b.predictions), b.active, b.longest]

    def _ctx(self, gpu, oracle, S, warm, T):
        f = cc.fixture("ctx_tiny")
        self.streams = [(f.bits[8 * (37 * s + s % 3):][:T],) for s in range(S)]
        self.g = gpu.CtxGroup(f.descs, S)
        self.batch = lambda m: gpu.CtxBatch(self.g, m)
        self.want = [[cc.Ref(f.descs).run(st[0])[warm:]] for st in self.streams]
        self.results = lambda b: [b.values]

    def fill(self, b, s, t0, n):
        cols = [c[t0:t0 + n] for c in self.streams[s]]
        if self.kind == "lstm":
            b.ppm[s, :n], b.bytes[s, :n] = cols
        elif self.kind == "ctx":
            b.bits[s, :n] = cols[0]
        else:
            b.set_records(s, *cols)

    def chunk(self, b, n):
        """The next n records of every stream: filled, uploaded and run; the caller downloads."""
        for s in range(self.S):
            self.fill(b, s, self.at, n)
        b.upload(n)
        self.g.run(b, n)
        self.at += n

    def close(self):
        self.g.close()


@pytest.mark.parametrize("S", [3, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_first_five_of_eight_records(gpu, oracle, kind, S):
    """S = 3: a 2D copy, pitch = 8 records, width = 5; S = 1: one block of 5 records.  What comes back is the oracle's,
    and records 5..7 of the host arrays, which no copy may touch, are still the zeros they were made with."""
    n, cap = 5, 8
    # (the LSTM's records are bytes; after 5 138 bits of match_tiny every stream is in a match, two bits into a byte)
    c = Case(gpu, oracle, kind, S, warm={"lstm": 20, "mixers": 64, "match": 5138}.get(kind, 800), n=n)
    if kind == "match":
        assert all(active.any(axis=1).all() and longest.all() for _, active, longest in c.want)
    b = c.batch(cap)
    c.chunk(b, n)
    b.download(n)
    b.wait()
    for col, got in enumerate(c.results(b)):
        assert got.shape[:2] == (S, cap)
        for s in range(S):
            assert np.array_equal(got[s, :n], c.want[s][col]), (kind, "stream", s, "column", col)
        assert not got[:, n:].any(), (kind, "column", col, "records past n were written")
    b.close()
    c.close()


@pytest.mark.parametrize("kind", ["indirect", "lstm"])
def test_two_batches_in_turn_on_the_transfer_streams(gpu, oracle, kind):
    """The smallest upload that leaves the bank's stream (S * n * bytes per record reaches 256 KiB; one record less does
    not), three chunks through two batches used alternately as in test_double_buffered_batches_keep_their_order: the
    upload of chunk k + 1 crosses beside the kernel of chunk k, and events alone keep each batch's upload -> run ->
    download in order."""
    if kind == "lstm":
        S, n, row = 4, 64, 256 * 4 + 1
    else:
        row = 4 * len(IND_MODELS) + 5
        S = 7
        n = -(-OWN_STREAM_MIN // (row * S))
    assert (S * n - 1) * row < OWN_STREAM_MIN <= S * n * row
    chunks = 3
    c = Case(gpu, oracle, kind, S, warm=0, n=chunks * n)
    bs = [c.batch(n), c.batch(n)]
    got = None
    for k in range(chunks):
        cur = bs[k & 1]
        if k >= 2:
            cur.wait()                       # the results of chunk k - 2 are on the host ...
            got = keep(got, c.results(cur), k - 2, n)
        c.chunk(cur, n)                      # ... so its host arrays may be refilled; beside the kernel of chunk k - 1
        cur.download(n)
    for k in (chunks - 2, chunks - 1):
        bs[k & 1].wait()
        got = keep(got, c.results(bs[k & 1]), k, n)
    for col in range(len(got)):
        for s in range(S):
            assert np.array_equal(got[col][s], c.want[s][col]), (kind, "stream", s, "column", col)
    for b in bs:
        b.close()
    c.close()


def keep(got, results, k, n):
    """results of chunk k ([S][n][...] per column) into the whole run's arrays"""
    if got is None:
        got = [None] * len(results)
    for col, r in enumerate(results):
        if got[col] is None:
            got[col] = np.zeros((r.shape[0], 0) + r.shape[2:], r.dtype)
        assert got[col].shape[1] == k * n
        got[col] = np.concatenate([got[col], r[:, :n]], axis=1)
    return got


ACCESSORS = {
    "mixers": ["predictions", "active_mask", "contexts", "bits", "p", "outputs"],
    "indirect": ["contexts", "bit_contexts", "bits", "predictions", "active"],
    "lstm": ["ppm", "bytes", "predictions", "active", "contexts"],
    "match": ["contexts", "bit_contexts", "bits", "predictions", "active", "longest"],
    "ctx": ["bits", "values"],
}
CALLS = {"mixers": "gmx_batch", "indirect": "gmx_ind_batch", "lstm": "gmx_lstm_batch", "match": "gmx_match_batch",
         "ctx": "gmx_ctx_batch"}


@pytest.mark.parametrize("kind", KINDS)
def test_a_batch_whose_bank_was_closed_first_is_a_shell(gpu, oracle, kind):
    """Documented behaviour: it keeps its buffers until its own close, every accessor returns null (GmxError through
    the wrapper), upload / download / wait return GMX_ERR_INVALID without touching the device, and closing it is
    clean -- also when it had pinned arrays and had been used."""
    c = Case(gpu, oracle, kind, 2, warm=0, n=8)
    used, fresh = c.batch(8), c.batch(8)
    c.chunk(used, 8)
    used.download(8)
    used.wait()
    c.close()
    for b in (used, fresh):
        for name in ACCESSORS[kind]:
            with pytest.raises(GmxError):
                getattr(b, name)
        for call in ("upload", "download"):
            assert getattr(b.L, f"{CALLS[kind]}_{call}")(b.h, 1) == GMX_ERR_INVALID, call
            assert getattr(b.L, f"{CALLS[kind]}_{call}")(b.h, 0) == GMX_ERR_INVALID, call
        assert getattr(b.L, f"{CALLS[kind]}_wait")(b.h) == GMX_ERR_INVALID
        b.close()


def test_columns_that_a_flag_leaves_out(gpu):
    g = gpu.MixerGroup(topology.stock(90), 2)
    b = gpu.Batch(g, 8, outputs=False, mask=False, last_outputs=False)
    for name in ("active_mask", "outputs", "last_outputs"):
        with pytest.raises(GmxError):
            getattr(b, name)
    assert b.predictions.shape == (2, 8, b.n_pad) and b.p.shape == (2, 8)
    b.close()
    g.close()
    f = cc.fixture("ctx_tiny")
    cg = gpu.CtxGroup(f.descs, 2)
    cb = gpu.CtxBatch(cg, 8, values=False)
    with pytest.raises(GmxError):
        cb.values
    with pytest.raises(GmxError) as e:
        cb.download(8)
    assert e.value.status == GMX_ERR_INVALID
    assert cb.L.gmx_ctx_batch_download(cb.h, 0) == GMX_ERR_INVALID
    cb.close()
    cg.close()
