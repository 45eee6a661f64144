"""Host-side handles of the context banks (gmx_ctx / gmx_ctx_batch of include/gmxmix.h): test and bench harness,
like match.py for the Match models."""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import CtxBlackboard, CtxDesc, CtxTargets, GmxError, check

KINDS = {"zero": 0, "bit_context": 1, "recent_byte": 2, "byte_plus_recent": 3, "interval": 4, "skip": 5,
         "indirect_hash": 6}
BATCH_VALUES = 1  # GMX_CTX_BATCH_VALUES
CKPT_CHUNK = 16384  # GMX_CTX_CKPT_CHUNK of csrc/gmx_ctx.h: entries a block of the checkpoint kernels walks


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@contextlib.contextmanager
def _stage_bytes(n):
    """GMX_CKPT_STAGE_BYTES = n for the calls inside (the library reads it at every call); None: as it is."""
    if n is None:
        yield
        return
    old = os.environ.get("GMX_CKPT_STAGE_BYTES")
    os.environ["GMX_CKPT_STAGE_BYTES"] = str(int(n))
    try:
        yield
    finally:
        if old is None:
            del os.environ["GMX_CKPT_STAGE_BYTES"]
        else:
            os.environ["GMX_CKPT_STAGE_BYTES"] = old


def make_desc(kind, index=0, map=None, num_bits=0, bytes_to_use=(), outer_order=0, table_size=0, inner_order=0):
    """One gmx_ctx_desc from the parameters topology.stock_context_descs() lists."""
    d = CtxDesc()
    d.kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    d.index = int(index)
    d.num_bits = int(num_bits)
    d.n_bytes = len(bytes_to_use)
    d.outer_order, d.inner_order, d.table_size = int(outer_order), int(inner_order), int(table_size)
    for i, b in enumerate(list(bytes_to_use)[:8]):
        d.bytes_to_use[i] = int(b)
    if map is not None:
        assert len(map) == 256
        for i, m in enumerate(map):
            d.map[i] = int(m)
    return d


def desc_array(descs):
    """A ctypes array of gmx_ctx_desc from [(name, kind, params)] or ready CtxDesc objects."""
    ds = [d if isinstance(d, CtxDesc) else make_desc(d[1], **d[2]) for d in descs]
    return (CtxDesc * max(1, len(ds)))(*ds)


def route_array(route):
    """int32 numpy array of a route (a variable index per column, -1: leave the column alone)."""
    return np.ascontiguousarray(route, np.int32)


def board_dict(bb):
    return dict(recent_bits=bb.recent_bits, new_bit=bb.new_bit, last_byte=bb.last_byte,
                rotating_history_pos=bb.rotating_history_pos, first_prediction=bb.first_prediction,
                recent_bytes=np.array(bb.recent_bytes[:], np.uint32), values=np.array(bb.values[:], np.uint32),
                rotating_history=np.array(bb.rotating_history[:], np.uint8))


class CtxGroup:
    """S banks of the V context variables `descs` describes ([(name, kind, params)], see topology)."""

    def __init__(self, descs, n_streams=1, device=0):
        self.L = _lib.lib()
        self.descs = list(descs)
        self.V = len(self.descs)
        self.S = int(n_streams)
        self.hash_vars = [i for i, d in enumerate(self.descs)
                          if (d.kind if isinstance(d, CtxDesc) else KINDS[d[1]]) == KINDS["indirect_hash"]]
        self.H = len(self.hash_vars)
        h = C.c_void_p()
        check(self.L.gmx_ctx_create(C.byref(h), desc_array(self.descs), self.V, self.S, device), "gmx_ctx_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.gmx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def bank_bytes(self):
        return self.L.gmx_ctx_bank_bytes(self.h)

    def set_cu_mask(self, words=None):
        w = list(words) if words else []
        arr = (C.c_uint32 * max(1, len(w)))(*w)
        check(self.L.gmx_ctx_set_cu_mask(self.h, arr, len(w)), "gmx_ctx_set_cu_mask")

    def reset(self):
        check(self.L.gmx_ctx_reset(self.h), "gmx_ctx_reset")

    def sync(self):
        check(self.L.gmx_ctx_sync(self.h), "gmx_ctx_sync")

    @staticmethod
    def targets(mixers=None, mixer_route=None, indirect=None, ind_route=None, match=None, match_route=None):
        """A gmx_ctx_targets; the route arrays are kept alive on the returned object."""
        t = CtxTargets()
        keep = []
        for batch, route, name in ((mixers, mixer_route, "mixer"), (indirect, ind_route, "ind"),
                                   (match, match_route, "match")):
            if batch is None:
                continue
            r = route_array(route)
            keep.append(r)
            setattr(t, {"mixer": "mixers", "ind": "indirect", "match": "match"}[name], batch.h)
            setattr(t, name + "_route", r.ctypes.data_as(C.POINTER(C.c_int32)))
            setattr(t, "n_" + name + "_route", len(r))
        t._keep = keep
        return t

    def run(self, batch, n_bits=None, targets=None, timed=False):
        n_bits = batch.max_bits if n_bits is None else n_bits
        ms = C.c_float(0)
        check(self.L.gmx_ctx_run(self.h, batch.h, n_bits, C.byref(targets) if targets is not None else None,
                                 C.byref(ms) if timed else None), "gmx_ctx_run")
        return ms.value if timed else None

    def last_kernel_ms(self):
        """(chain, expand, commit) ms of the newest timed run."""
        ms = (C.c_float * 3)()
        check(self.L.gmx_ctx_last_kernel_ms(self.h, ms), "gmx_ctx_last_kernel_ms")
        return tuple(float(x) for x in ms)

    def run_ragged(self, batch, n_bits, targets=None):
        nb = np.ascontiguousarray(n_bits, np.uint64)
        assert nb.shape == (self.S,)
        check(self.L.gmx_ctx_run_ragged(self.h, batch.h, nb.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        C.byref(targets) if targets is not None else None), "gmx_ctx_run_ragged")

    def forward(self, stream=0):
        """gmx_ctx_forward: one record of run() for one stream.  Returns (values [V], bit_context)."""
        vals = np.zeros(self.V, np.uint32)
        bc = C.c_uint32(0)
        check(self.L.gmx_ctx_forward(self.h, stream, _vp(vals), C.byref(bc)), "gmx_ctx_forward")
        return vals, bc.value

    def learn(self, bit, stream=0):
        """gmx_ctx_learn: `bit` becomes the blackboard's new_bit (a learned or a perceived bit alike)."""
        check(self.L.gmx_ctx_learn(self.h, stream, int(bit)), "gmx_ctx_learn")

    def blackboard(self, stream=0):
        bb = CtxBlackboard()
        check(self.L.gmx_ctx_blackboard_get(self.h, stream, C.byref(bb)), "gmx_ctx_blackboard_get")
        return bb

    def set_blackboard(self, bb, stream=0):
        check(self.L.gmx_ctx_blackboard_set(self.h, stream, C.byref(bb)), "gmx_ctx_blackboard_set")

    def export(self, stream=0):
        """(bytes, offsets [H + 1]) of one stream's IndirectHash sections."""
        n = C.c_size_t(0)
        off = (C.c_size_t * (self.H + 1))()
        check(self.L.gmx_ctx_export(self.h, stream, None, C.byref(n), off), "gmx_ctx_export(size)")
        buf = np.zeros(max(1, n.value), np.uint8)
        check(self.L.gmx_ctx_export(self.h, stream, _vp(buf), C.byref(n), off), "gmx_ctx_export")
        return buf[:n.value].tobytes(), [int(o) for o in off]

    def import_(self, data, stream=0):
        buf = np.frombuffer(data or b"\0", np.uint8)
        check(self.L.gmx_ctx_import(self.h, stream, _vp(buf), len(data)), "gmx_ctx_import")

    # ---- the group checkpoint (gmx_ctx_group_*, csrc/gmx_ctx_ckpt.hip)
    def _window(self, first, count):
        return int(first), self.S - int(first) if count is None else int(count)

    def group_sizes(self, first=0, count=None):
        """(off [count + 1], var_off [count][H + 1]) of a sizing call: nothing is packed."""
        first, count = self._window(first, count)
        off = (C.c_size_t * (max(count, 0) + 1))()
        var = (C.c_size_t * (max(count, 1) * (self.H + 1)))()
        check(self.L.gmx_ctx_group_export(self.h, first, count, None, 0, off, var), "gmx_ctx_group_export(size)")
        return [int(o) for o in off], [[int(var[i * (self.H + 1) + j]) for j in range(self.H + 1)]
                                       for i in range(count)]

    def group_export(self, first=0, count=None, stage_bytes=None):
        """(bytes, off [count + 1], var_off [count][H + 1]): stream first + i's sections are bytes[off[i]:off[i + 1]],
        what export(first + i) gives.  stage_bytes: GMX_CKPT_STAGE_BYTES for the two calls."""
        with _stage_bytes(stage_bytes):
            off, var = self.group_sizes(first, count)
            first, count = self._window(first, count)
            buf = np.zeros(max(1, off[-1]), np.uint8)
            o = (C.c_size_t * (count + 1))()
            v = (C.c_size_t * (count * (self.H + 1)))()
            check(self.L.gmx_ctx_group_export(self.h, first, count, _vp(buf), off[-1], o, v), "gmx_ctx_group_export")
        assert [int(x) for x in o] == off
        return buf[:off[-1]].tobytes(), off, var

    def group_import(self, data, off, first=0, stage_bytes=None):
        """The inverse of group_export: stream first + i takes data[off[i]:off[i + 1]].  A malformed section anywhere
        raises GmxError(GMX_ERR_FORMAT) and leaves every bank as it was."""
        buf = np.frombuffer(bytes(data) or b"\0", np.uint8)
        o = (C.c_size_t * len(off))(*[int(x) for x in off])
        with _stage_bytes(stage_bytes):
            check(self.L.gmx_ctx_group_import(self.h, int(first), len(off) - 1, _vp(buf), o), "gmx_ctx_group_import")

    def group_blackboards(self, first=0, count=None):
        """The blackboards of streams [first, first + count) in one gather launch and one transfer."""
        first, count = self._window(first, count)
        arr = (CtxBlackboard * max(count, 1))()
        check(self.L.gmx_ctx_group_blackboard_get(self.h, first, count, arr), "gmx_ctx_group_blackboard_get")
        return [CtxBlackboard.from_buffer_copy(arr[i]) for i in range(count)]

    def set_group_blackboards(self, boards, first=0):
        arr = (CtxBlackboard * max(len(boards), 1))(*boards)
        check(self.L.gmx_ctx_group_blackboard_set(self.h, int(first), len(boards), arr), "gmx_ctx_group_blackboard_set")

    def group_ops(self):
        """Launches, transfers and waits of the newest group call on this bank."""
        return self.L.gmx_debug_ctx_group_ops(self.h)

    def copy_from(self, src, src_stream=0, dst_stream=0):
        check(self.L.gmx_ctx_copy(self.h, dst_stream, src.h, src_stream), "gmx_ctx_copy")

    def memory_usage(self, var):
        v = C.c_uint64(0)
        check(self.L.gmx_ctx_memory_usage(self.h, var, C.byref(v)), "gmx_ctx_memory_usage")
        return v.value


class CtxBatch:
    def __init__(self, group, max_bits, values=True):
        self.g = group
        self.L = group.L
        self.max_bits = int(max_bits)
        self.flags = BATCH_VALUES if values else 0
        h = C.c_void_p()
        check(self.L.gmx_ctx_batch_create(C.byref(h), group.h, self.max_bits, self.flags), "gmx_ctx_batch_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.gmx_ctx_batch_destroy(self.h)
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
    def bits(self):
        return self._view(self.L.gmx_ctx_batch_bits, np.uint8, (self.g.S, self.max_bits))

    @property
    def values(self):
        return self._view(self.L.gmx_ctx_batch_values, np.uint32, (self.g.S, self.max_bits, self.g.V))

    def upload(self, n_bits=None):
        check(self.L.gmx_ctx_batch_upload(self.h, self.max_bits if n_bits is None else n_bits),
              "gmx_ctx_batch_upload")

    def download(self, n_bits=None):
        check(self.L.gmx_ctx_batch_download(self.h, self.max_bits if n_bits is None else n_bits),
              "gmx_ctx_batch_download")

    def wait(self):
        check(self.L.gmx_ctx_batch_wait(self.h), "gmx_ctx_batch_wait")
