"""Host-side handles of the Match-model banks (gmx_match / gmx_match_batch of include/gmxmix.h): test and bench
harness, like indirect.py for the Indirect models; and the byte-stream generator the Match fixtures and
scripts/bench_match.py share."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GmxError, MatchDesc, check


CKPT_CHUNK = 16384  # GMX_MATCH_CKPT_CHUNK of csrc/gmx_match.h: entries a block of the checkpoint kernels walks


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def match_stream(seed, n_bytes):
    """A seeded byte stream made of what the Match models tell apart: uniform-random stretches, literal text over a
    small alphabet, copies of earlier stretches (up to 400 bytes: match_length_ reaches 255 after 32), and runs of one
    byte value (up to 700 bytes)."""
    rng = np.random.RandomState(seed)
    out = bytearray()
    kinds = 0
    while len(out) < n_bytes:
        # the first four pieces are one of each kind, then they are drawn
        kind = kinds if kinds < 4 else rng.randint(0, 4)
        kinds += 1
        if kind == 0:
            out += rng.randint(0, 256, rng.randint(20, 300)).astype(np.uint8).tobytes()
        elif kind == 1:
            out += (97 + rng.randint(0, 6, rng.randint(20, 200))).astype(np.uint8).tobytes()
        elif kind == 2 and len(out) > 64:
            n = int(rng.randint(8, 400))
            src = int(rng.randint(0, len(out) - 8))
            for i in range(n):  # (a copy may run into itself, like an LZ77 match)
                out.append(out[src + i])
        else:
            n = int(rng.randint(600, 700)) if kinds <= 5 else int(rng.randint(2, 120))
            out += bytes([int(rng.randint(0, 256))]) * n
    return np.frombuffer(bytes(out[:n_bytes]), np.uint8).copy()


def stream_bits(data):
    """(bits [8n], bit_contexts [8n]) of a byte stream: MSB first, bit_context = recent_bits - 1
    (basic-contexts.cpp:30-36)."""
    bits = np.unpackbits(np.asarray(data, np.uint8))
    b = bits.reshape(-1, 8).astype(np.uint32)
    bc = np.zeros_like(b)
    for i in range(1, 8):
        bc[:, i] = ((bc[:, i - 1] + 1) << 1 | b[:, i - 1]) - 1
    return bits, bc.reshape(-1)


class MatchGroup:
    """S banks of K Match models.  models = [(table_size, limit)] or [(table_size, limit, slot)] in construction
    order (default slots 0..K-1); history_capacity: bytes of history per stream."""

    def __init__(self, models, history_capacity, n_streams=1, device=0):
        self.L = _lib.lib()
        self.models = [(int(m[0]), int(m[1]), int(m[2]) if len(m) > 2 else i) for i, m in enumerate(models)]
        self.K = len(self.models)
        self.S = int(n_streams)
        self.slots = [m[2] for m in self.models]
        descs = (MatchDesc * max(1, self.K))(*[MatchDesc(*m) for m in self.models])
        h = C.c_void_p()
        check(self.L.gmx_match_create(C.byref(h), descs, self.K, int(history_capacity), self.S, device),
              "gmx_match_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.gmx_match_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def bank_bytes(self):
        return self.L.gmx_match_bank_bytes(self.h)

    def set_cu_mask(self, words=None):
        w = list(words) if words else []
        arr = (C.c_uint32 * max(1, len(w)))(*w)
        check(self.L.gmx_match_set_cu_mask(self.h, arr, len(w)), "gmx_match_set_cu_mask")

    def reset(self):
        check(self.L.gmx_match_reset(self.h), "gmx_match_reset")

    def sync(self):
        check(self.L.gmx_match_sync(self.h), "gmx_match_sync")

    def forward(self, contexts, bit_context, stream=0):
        c = np.ascontiguousarray(contexts, np.uint32)
        assert c.shape == (self.K,)
        pred = np.zeros(self.K, np.float32)
        act = np.zeros(self.K, np.uint8)
        lm = C.c_uint32(0)
        check(self.L.gmx_match_forward(self.h, stream, _vp(c), int(bit_context), _vp(pred), _vp(act), C.byref(lm)),
              "gmx_match_forward")
        return pred, act, lm.value

    def learn(self, bit, stream=0):
        check(self.L.gmx_match_learn(self.h, stream, int(bit)), "gmx_match_learn")

    @staticmethod
    def _cols(ctx_columns):
        cols = [int(c) for c in (ctx_columns or [])]
        return (C.c_int32 * max(1, len(cols)))(*cols), len(cols)

    def run(self, batch, n_bits=None, into=None, ctx_columns=None, timed=False):
        n_bits = batch.max_bits if n_bits is None else n_bits
        ms = C.c_float(0)
        arr, n = self._cols(ctx_columns)
        check(self.L.gmx_match_run(self.h, batch.h, n_bits, into.h if into else None, arr, n,
                                   C.byref(ms) if timed else None), "gmx_match_run")
        return ms.value if timed else None

    def run_ragged(self, batch, n_bits, into=None, ctx_columns=None):
        nb = np.ascontiguousarray(n_bits, np.uint64)
        assert nb.shape == (self.S,)
        arr, n = self._cols(ctx_columns)
        check(self.L.gmx_match_run_ragged(self.h, batch.h, nb.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          into.h if into else None, arr, n), "gmx_match_run_ragged")

    def slot_values(self, stream=0):
        """(the K blackboard slots, ShortTermMemory::new_bit) as the bank holds them."""
        v = np.zeros(self.K, np.float32)
        nb = C.c_int(0)
        check(self.L.gmx_match_slots_get(self.h, stream, v.ctypes.data_as(C.POINTER(C.c_float)), C.byref(nb)),
              "gmx_match_slots_get")
        return v, nb.value

    def set_slot_values(self, values, new_bit, stream=0):
        v = np.ascontiguousarray(values, np.float32)
        assert v.shape == (self.K,)
        check(self.L.gmx_match_slots_set(self.h, stream, v.ctypes.data_as(C.POINTER(C.c_float)), int(new_bit)),
              "gmx_match_slots_set")

    def history_size(self, stream=0):
        v = C.c_uint64(0)
        check(self.L.gmx_match_history_size(self.h, stream, C.byref(v)), "gmx_match_history_size")
        return v.value

    def export(self, stream=0):
        """(long section, short section) of one stream."""
        nl, ns = C.c_size_t(0), C.c_size_t(0)
        check(self.L.gmx_match_export(self.h, stream, None, C.byref(nl), None, C.byref(ns)), "gmx_match_export(size)")
        lb, sb = np.zeros(max(1, nl.value), np.uint8), np.zeros(max(1, ns.value), np.uint8)
        check(self.L.gmx_match_export(self.h, stream, _vp(lb), C.byref(nl), _vp(sb), C.byref(ns)), "gmx_match_export")
        return lb[:nl.value].tobytes(), sb[:ns.value].tobytes()

    def import_(self, long_bytes, short_bytes, stream=0):
        lb = np.frombuffer(long_bytes or b"\0", np.uint8)
        sb = np.frombuffer(short_bytes or b"\0", np.uint8)
        check(self.L.gmx_match_import(self.h, stream, _vp(lb), len(long_bytes), _vp(sb), len(short_bytes)),
              "gmx_match_import")

    def export_all(self, first=0, count=None):
        """(long_bytes, long_off, short_bytes) of streams [first, first + count) in one call (gmx_match_group_export):
        stream first + i's long section is long_bytes[long_off[i]:long_off[i + 1]], its short section
        short_bytes[11 K i:11 K (i + 1)] -- the bytes export(stream) gives."""
        count = self.S - first if count is None else int(count)
        off = (C.c_size_t * (max(count, 0) + 1))()
        check(self.L.gmx_match_group_export(self.h, first, count, None, 0, off, None), "gmx_match_group_export(size)")
        lb = np.zeros(max(1, off[count]), np.uint8)
        sb = np.zeros(max(1, 11 * self.K * count), np.uint8)
        check(self.L.gmx_match_group_export(self.h, first, count, _vp(lb), lb.size, off, _vp(sb)),
              "gmx_match_group_export")
        return lb[:off[count]].tobytes(), [int(o) for o in off], sb[:11 * self.K * count].tobytes()

    def import_all(self, long_bytes, long_off, short_bytes, first=0):
        """The inverse (gmx_match_group_import): section i goes to stream first + i.  A malformed section anywhere
        raises GmxError (GMX_ERR_FORMAT) and leaves every bank as it was; slot values and new_bit stay."""
        count = len(long_off) - 1
        off = (C.c_size_t * (max(count, 0) + 1))(*[int(o) for o in long_off])
        if count < 1 or off[count] > len(long_bytes):   # (the C call is not told the buffers' lengths)
            raise GmxError(-1, "gmx_match_group_import")
        if len(short_bytes) != 11 * self.K * count:
            raise GmxError(-6, "gmx_match_group_import")
        lb = np.frombuffer(long_bytes or b"\0", np.uint8)
        sb = np.frombuffer(short_bytes or b"\0", np.uint8)
        check(self.L.gmx_match_group_import(self.h, first, count, _vp(lb), off, _vp(sb)), "gmx_match_group_import")

    def copy_from(self, src, src_stream=0, dst_stream=0):
        check(self.L.gmx_match_copy(self.h, dst_stream, src.h, src_stream), "gmx_match_copy")

    def memory_usage(self, model):
        v = C.c_uint64(0)
        check(self.L.gmx_match_memory_usage(self.h, model, C.byref(v)), "gmx_match_memory_usage")
        return v.value


class MatchBatch:
    def __init__(self, group, max_bits):
        self.g = group
        self.L = group.L
        self.max_bits = int(max_bits)
        h = C.c_void_p()
        check(self.L.gmx_match_batch_create(C.byref(h), group.h, self.max_bits), "gmx_match_batch_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.gmx_match_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _view(self, fn, dtype, shape):
        ptr = fn(self.h)
        if not ptr:
            raise GmxError(-2, fn.__name__)
        n = int(np.prod(shape))
        buf = (C.c_byte * (n * np.dtype(dtype).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    @property
    def contexts(self):
        return self._view(self.L.gmx_match_batch_contexts, np.uint32, (self.g.S, self.max_bits, self.g.K))

    @property
    def bit_contexts(self):
        return self._view(self.L.gmx_match_batch_bit_contexts, np.uint32, (self.g.S, self.max_bits))

    @property
    def bits(self):
        return self._view(self.L.gmx_match_batch_bits, np.uint8, (self.g.S, self.max_bits))

    @property
    def predictions(self):
        return self._view(self.L.gmx_match_batch_predictions, np.float32, (self.g.S, self.max_bits, self.g.K))

    @property
    def active(self):
        return self._view(self.L.gmx_match_batch_active, np.uint8, (self.g.S, self.max_bits, self.g.K))

    @property
    def longest(self):
        return self._view(self.L.gmx_match_batch_longest, np.uint32, (self.g.S, self.max_bits))

    def set_records(self, stream, contexts, bit_contexts, bits):
        T = len(bits)
        self.contexts[stream, :T] = contexts
        self.bit_contexts[stream, :T] = bit_contexts
        self.bits[stream, :T] = bits

    def upload(self, n_bits=None):
        check(self.L.gmx_match_batch_upload(self.h, self.max_bits if n_bits is None else n_bits),
              "gmx_match_batch_upload")

    def download(self, n_bits=None):
        check(self.L.gmx_match_batch_download(self.h, self.max_bits if n_bits is None else n_bits),
              "gmx_match_batch_download")

    def wait(self):
        check(self.L.gmx_match_batch_wait(self.h), "gmx_match_batch_wait")
