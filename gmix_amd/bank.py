"""Python-side mirror of the mixer surface over the C ABI (numpy in, numpy out).

`Topology` is what `Predictor`'s constructor fixes before/while `AddMixers` runs
(predictor.cpp:17-40, 251-358); `MixerGroup` is S banks of it on one MI355X; `Batch` holds
records for the batched path.  All compute happens in libgmxmix.so on the GPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GmxError, MixerDesc, TopologyStruct, check

BATCH_OUTPUTS = 1
BATCH_MASK = 2


class Topology:
    def __init__(self, n_inputs, mixers, skip=(1,)):
        """mixers: [(layer, table_size, learning_rate), ...] in construction order."""
        self.n_inputs = int(n_inputs)
        self.mixers = [(int(l), int(t), float(np.float32(lr))) for l, t, lr in mixers]
        self.skip = [int(i) for i in skip]
        self.l0 = sum(1 for m in self.mixers if m[0] == 0)
        self.l1 = sum(1 for m in self.mixers if m[0] == 1)
        self.has_final = any(m[0] == 2 for m in self.mixers)

    @property
    def n_mixers(self):
        return len(self.mixers)

    def weight_sizes(self):
        """weight_size_ of every mixer (mixer.cpp:17-26)."""
        out, k0, k1 = [], 0, 0
        for layer, _, _ in self.mixers:
            if layer == 0:
                out.append(self.n_inputs + k0)
                k0 += 1
            elif layer == 1:
                out.append(self.l0 + k1 + len(self.skip))
                k1 += 1
            else:
                out.append(self.l0 + self.l1 + len(self.skip))
        return out

    def bytes_per_bit(self):
        """Algorithmic HBM bytes per coded bit:
        8*W (each weight read once, written once) + 4*N inputs + 4*M contexts + 4 (p out)."""
        return 8 * sum(self.weight_sizes()) + 4 * self.n_inputs + 4 * self.n_mixers + 4

    def _struct(self):
        self._descs = (MixerDesc * len(self.mixers))(*[MixerDesc(l, t, lr) for l, t, lr in self.mixers])
        self._skip = (C.c_int32 * max(1, len(self.skip)))(*self.skip)
        return TopologyStruct(self.n_inputs, len(self.skip), self._skip, len(self.mixers), self._descs)


def register_rows_eligible(topo):
    """Whether MixerGroup.set_register_rows would accept a group of this topology (host code only):
    three layers of 1..24 / 1..8 / 1 mixers, one skip input, 4..256 inputs."""
    st = topo._struct()
    rc = _lib.lib().gmx_topology_register_rows_eligible(C.byref(st))
    if rc < 0:
        raise GmxError(rc, "gmx_topology_register_rows_eligible")
    return bool(rc)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class MixerGroup:
    """S independent mixer banks on one device (gmx_group)."""

    def __init__(self, topo, n_streams=1, device=0):
        self.topo = topo
        self.S = n_streams
        self.L = _lib.lib()
        h = C.c_void_p()
        st = topo._struct()
        check(self.L.gmx_group_create(C.byref(h), C.byref(st), n_streams, device), "gmx_group_create")
        self.h = h

    def set_cu_mask(self, words=None):
        """Compute units this bank's kernels may use: 32-bit words, bit i = CU i (None: all)."""
        w = list(words) if words else []
        arr = (C.c_uint32 * max(1, len(w)))(*w)
        check(self.L.gmx_group_set_cu_mask(self.h, arr, len(w)), "gmx_group_set_cu_mask")

    def set_register_rows(self, on=True):
        """Batched runs through the register-resident kernel for any three-layer bank (off by default; GmxError
        for a topology register_rows_eligible() refuses).  May be flipped between launches."""
        check(self.L.gmx_group_set_register_rows(self.h, 1 if on else 0), "gmx_group_set_register_rows")

    def close(self):
        if getattr(self, "h", None):
            self.L.gmx_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(self.L.gmx_group_reset(self.h), "gmx_group_reset")

    def sync(self):
        check(self.L.gmx_group_sync(self.h), "gmx_group_sync")

    @property
    def bank_bytes(self):
        return self.L.gmx_group_bank_bytes(self.h)

    def timer_start(self):
        check(self.L.gmx_group_timer_start(self.h), "gmx_group_timer_start")

    def timer_stop(self):
        ms = C.c_float(0)
        check(self.L.gmx_group_timer_stop(self.h, C.byref(ms)), "gmx_group_timer_stop")
        return ms.value

    # ---- per-bit surface (Predict / Perceive+Learn) ----
    def forward(self, predictions, active, contexts, stream=0, want_all=True):
        pred = np.ascontiguousarray(predictions, np.float32)
        ctx = np.ascontiguousarray(contexts, np.uint32)
        assert pred.shape == (self.topo.n_inputs,) and ctx.shape == (self.topo.n_mixers,)
        p = C.c_float()
        out = np.zeros(self.topo.n_mixers, np.float32) if want_all else None
        if active is None:
            act, na = None, -1
        else:
            act = np.ascontiguousarray(active, np.int32)
            na = len(act)
        check(self.L.gmx_bank_forward(self.h, stream, _vp(pred), _vp(act), na, _vp(ctx), C.byref(p),
                                      _vp(out)), "gmx_bank_forward")
        return p.value, out

    def learn(self, bit, stream=0):
        check(self.L.gmx_bank_learn(self.h, stream, int(bit)), "gmx_bank_learn")

    # ---- batched surface ----
    def run(self, batch, n_bits=None, learn=True, timed=False):
        n_bits = batch.max_bits if n_bits is None else n_bits
        ms = C.c_float(0)
        check(self.L.gmx_group_run(self.h, batch.h, n_bits, 1 if learn else 0,
                                   C.byref(ms) if timed else None), "gmx_group_run")
        return ms.value if timed else None

    def run_ragged(self, batch, n_bits, learn=True):
        """Stream s runs bits [0, n_bits[s]) of its records (gmx_group_run_ragged)."""
        n = np.ascontiguousarray(n_bits, np.uint64)
        assert n.shape == (self.S,)
        check(self.L.gmx_group_run_ragged(self.h, batch.h, n.ctypes.data_as(C.POINTER(C.c_uint64)), 1 if learn else 0),
              "gmx_group_run_ragged")

    # ---- persistence ----
    def export(self, stream=0):
        """(long_bytes, short_bytes) in the reference's checkpoint format."""
        nl, ns = C.c_size_t(0), C.c_size_t(0)
        check(self.L.gmx_bank_export(self.h, stream, None, C.byref(nl), None, C.byref(ns)),
              "gmx_bank_export(size)")
        lb = np.zeros(max(nl.value, 1), np.uint8)
        sb = np.zeros(max(ns.value, 1), np.uint8)
        check(self.L.gmx_bank_export(self.h, stream, _vp(lb), C.byref(nl), _vp(sb), C.byref(ns)),
              "gmx_bank_export")
        return lb.tobytes()[:nl.value], sb.tobytes()[:ns.value]

    def import_(self, long_bytes, short_bytes, stream=0):
        lb = np.frombuffer(long_bytes, np.uint8) if len(long_bytes) else np.zeros(1, np.uint8)
        sb = np.frombuffer(short_bytes, np.uint8)
        check(self.L.gmx_bank_import(self.h, stream, _vp(lb), len(long_bytes), _vp(sb), len(short_bytes)),
              "gmx_bank_import")

    def export_all(self, first=0, count=None):
        """[(long_bytes, short_bytes)] of streams [first, first + count) in one call (gmx_group_export): the learned
        rows are found and packed on the device; section i is byte for byte export(first + i)."""
        count = self.S - first if count is None else count
        off = (C.c_size_t * (max(count, 0) + 1))()
        check(self.L.gmx_group_export(self.h, first, count, None, 0, off, None), "gmx_group_export(size)")
        if count == 0:
            return []
        ns = 24 * self.topo.n_mixers
        lb = np.zeros(max(off[count], 1), np.uint8)
        sb = np.zeros(count * ns, np.uint8)
        check(self.L.gmx_group_export(self.h, first, count, _vp(lb), off[count], off, _vp(sb)), "gmx_group_export")
        return [(lb[off[i]:off[i + 1]].tobytes(), sb[i * ns:(i + 1) * ns].tobytes()) for i in range(count)]

    def import_all(self, sections, first=0):
        """The inverse of export_all (gmx_group_import): sections[i] = (long_bytes, short_bytes) goes to stream
        first + i.  A malformed section anywhere raises GmxError and leaves every bank as it was."""
        count = len(sections)
        ns = 24 * self.topo.n_mixers
        if any(len(s) != ns for _, s in sections):
            raise GmxError(-6, "gmx_group_import(short section)")
        off = (C.c_size_t * (count + 1))()
        for i, (l, _) in enumerate(sections):
            off[i + 1] = off[i] + len(l)
        lb = np.frombuffer(b"".join(l for l, _ in sections) or b"\0", np.uint8)
        sb = np.frombuffer(b"".join(s for _, s in sections) or b"\0", np.uint8)
        check(self.L.gmx_group_import(self.h, first, count, _vp(lb), off, _vp(sb)), "gmx_group_import")

    def copy_from(self, src, src_stream=0, dst_stream=0):
        check(self.L.gmx_bank_copy(self.h, dst_stream, src.h, src_stream), "gmx_bank_copy")

    def memory_usage(self, mixer, stream=0):
        v = C.c_uint64()
        check(self.L.gmx_bank_memory_usage(self.h, stream, mixer, C.byref(v)), "gmx_bank_memory_usage")
        return v.value


class Batch:
    """Records for up to max_bits bits of every stream of a group (gmx_batch)."""

    def __init__(self, group, max_bits, outputs=True, mask=True, last_outputs=False):
        self.g = group
        self.L = group.L
        self.max_bits = int(max_bits)
        self.flags = (BATCH_OUTPUTS if outputs else 0) | (BATCH_MASK if mask else 0) | (8 if last_outputs else 0)
        h = C.c_void_p()
        check(self.L.gmx_batch_create(C.byref(h), group.h, self.max_bits, self.flags), "gmx_batch_create")
        self.h = h
        self.n_pad = self.L.gmx_batch_n_pad(h)
        self.mask_words = self.L.gmx_batch_mask_words(h)

    def close(self):
        if getattr(self, "h", None):
            self.L.gmx_batch_destroy(self.h)
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
    def predictions(self):
        return self._view(self.L.gmx_batch_predictions, np.float32, (self.g.S, self.max_bits, self.n_pad))

    @property
    def active_mask(self):
        return self._view(self.L.gmx_batch_active_mask, np.uint32, (self.g.S, self.max_bits, self.mask_words))

    @property
    def contexts(self):
        return self._view(self.L.gmx_batch_contexts, np.uint32, (self.g.S, self.max_bits, self.g.topo.n_mixers))

    @property
    def bits(self):
        return self._view(self.L.gmx_batch_bits, np.uint8, (self.g.S, self.max_bits))

    @property
    def p(self):
        return self._view(self.L.gmx_batch_p, np.float32, (self.g.S, self.max_bits))

    @property
    def last_outputs(self):
        """[S][M]: every mixer's output of each stream's last bit of the run (GMX_BATCH_LAST_OUTPUTS)."""
        return self._view(self.L.gmx_batch_last_outputs, np.float32, (self.g.S, self.g.topo.n_mixers))

    @property
    def outputs(self):
        return self._view(self.L.gmx_batch_outputs, np.float32, (self.g.S, self.max_bits, self.g.topo.n_mixers))

    def set_records(self, stream, predictions, active, contexts, bits):
        """Fill stream `stream` from raw blackboard arrays: predictions[T,N] (stale slots allowed),
        active[T,N] flags (or None = all active), contexts[T,M], bits[T]."""
        T = len(bits)
        N = self.g.topo.n_inputs
        self.predictions[stream, :T, :N] = predictions
        self.predictions[stream, :T, N:] = 0
        if self.flags & BATCH_MASK:
            a = np.ones((T, N), np.uint8) if active is None else np.asarray(active, np.uint8)
            padded = np.zeros((T, self.mask_words * 32), np.uint8)
            padded[:, :N] = a != 0
            words = np.packbits(padded.reshape(T, self.mask_words, 32), axis=2, bitorder="little")
            self.active_mask[stream, :T, :] = words.view(np.uint32).reshape(T, self.mask_words)
        elif active is not None:
            # without a mask the caller must zero silent slots itself (exact: they add nothing)
            self.predictions[stream, :T, :N] = np.where(np.asarray(active) != 0, predictions, 0)
        self.contexts[stream, :T, :] = contexts
        self.bits[stream, :T] = bits

    def upload(self, n_bits=None):
        check(self.L.gmx_batch_upload(self.h, self.max_bits if n_bits is None else n_bits), "gmx_batch_upload")

    def download(self, n_bits=None):
        check(self.L.gmx_batch_download(self.h, self.max_bits if n_bits is None else n_bits),
              "gmx_batch_download")

    def wait(self):
        check(self.L.gmx_batch_wait(self.h), "gmx_batch_wait")

    def fill_synthetic(self, n_bits=None, seed=0, restart=True, ctx_mode=0, ctx_mod=1, zero_mod=0,
                       bit_mode=0):
        check(self.L.gmx_batch_fill_synthetic(self.h, self.max_bits if n_bits is None else n_bits, seed,
                                              1 if restart else 0, ctx_mode, ctx_mod, zero_mod, bit_mode),
              "gmx_batch_fill_synthetic")


def device_count():
    n = C.c_int(0)
    check(_lib.lib().gmx_device_count(C.byref(n)), "gmx_device_count")
    return n.value


class Lockstep:
    """All streams of a group one bit at a time (gmx_lockstep): each half step one hipGraph, or -- `persistent`,
    where it applies -- S persistent waves behind one doorbell."""

    def __init__(self, group, outputs=False, persistent=False):
        self.g = group
        self.L = group.L
        h = C.c_void_p()
        flags = (BATCH_OUTPUTS if outputs else 0) | (4 if persistent else 0)  # GMX_LOCKSTEP_PERSISTENT
        check(self.L.gmx_lockstep_create(C.byref(h), group.h, flags), "gmx_lockstep_create")
        self.h = h
        self.persistent = bool(self.L.gmx_lockstep_is_persistent(h))
        # the record batch is owned by the lock-step object: a Batch view that never destroys it
        b = Batch.__new__(Batch)
        b.g, b.L, b.max_bits = group, group.L, 1
        b.flags = BATCH_MASK | (BATCH_OUTPUTS if outputs else 0)
        b.h = C.c_void_p(self.L.gmx_lockstep_batch(h))
        b.n_pad = self.L.gmx_batch_n_pad(b.h)
        b.mask_words = self.L.gmx_batch_mask_words(b.h)
        b.close = lambda: None
        self.batch = b

    def predict(self):
        check(self.L.gmx_lockstep_predict(self.h), "gmx_lockstep_predict")
        return self.batch.p[:, 0]

    def learn(self):
        check(self.L.gmx_lockstep_learn(self.h), "gmx_lockstep_learn")

    def learn_predict(self):
        """Learn the bits of the step before and predict the next records, one graph."""
        check(self.L.gmx_lockstep_learn_predict(self.h), "gmx_lockstep_learn_predict")
        return self.batch.p[:, 0]

    def close(self):
        if getattr(self, "h", None):
            self.batch.h = None
            self.L.gmx_lockstep_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


STEP_LEARN, STEP_PREDICT = 1, 2


class ChainStep:
    """S decoders in lock step through every device-side model (gmx_chainstep): one hipGraph per coded bit.  `indirect`
    / `lstm` may be None.  Fill the host views for the streams that take part, set `what`, call step()."""

    def __init__(self, group, indirect=None, lstm=None, lstm_slot=-1, mixer_ctx_col=-1, ind_ctx_col=-1):
        self.g, self.L = group, group.L
        h = C.c_void_p()
        check(self.L.gmx_chainstep_create(C.byref(h), group.h, indirect.h if indirect else None,
                                          lstm.h if lstm else None, lstm_slot, mixer_ctx_col, ind_ctx_col),
              "gmx_chainstep_create")
        self.h = h
        S, M = group.S, group.topo.n_mixers
        n_pad = (group.topo.n_inputs + 3) // 4 * 4
        mw = (group.topo.n_inputs + 31) // 32
        self.mask_words = mw

        def view(name, dtype, shape):
            ptr = getattr(self.L, "gmx_chainstep_" + name)(h)
            if not ptr:
                return None
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer((C.c_char * n).from_address(ptr), dtype=dtype).reshape(shape)

        self.predictions = view("predictions", np.float32, (S, n_pad))
        self.active_mask = view("active_mask", np.uint32, (S, mw))
        self.contexts = view("contexts", np.uint32, (S, M))
        K = indirect.K if indirect else 0
        self.ind_contexts = view("ind_contexts", np.uint32, (S, K)) if indirect else None
        self.bit_contexts = view("bit_contexts", np.uint32, (S,)) if indirect else None
        self.ppm = view("ppm", np.float32, (S, 256)) if lstm else None
        self.bits = view("bits", np.uint8, (S,))
        self.what = view("what", np.uint8, (S,))
        self.p = view("p", np.float32, (S,))
        self.outputs = view("outputs", np.float32, (S, M))
        self.match_contexts = None  # (attach_match)

    def _view(self, name, dtype, shape):
        ptr = getattr(self.L, "gmx_chainstep_" + name)(self.h)
        if not ptr:
            return None
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return np.frombuffer((C.c_char * n).from_address(ptr), dtype=dtype).reshape(shape)

    def attach_match(self, group, ctx_columns=None):
        """The Match models of `group` (a MatchGroup of as many streams) step on the device from now on
        (gmx_chainstep_attach_match): once, before the first step.  Afterwards `match_contexts` [S][K] takes the models'
        context words (byte-opening predicts and a stream's first predict), `bit_contexts` every predict's."""
        cols = [int(c) for c in (ctx_columns or [])]
        arr = (C.c_int32 * max(1, len(cols)))(*cols)
        check(self.L.gmx_chainstep_attach_match(self.h, group.h, arr, len(cols)), "gmx_chainstep_attach_match")
        self.match_contexts = self._view("match_contexts", np.uint32, (self.g.S, group.K))
        if self.bit_contexts is None:
            self.bit_contexts = self._view("bit_contexts", np.uint32, (self.g.S,))

    def attach_ctx(self, group, mixer_route, ind_route=None, match_route=None):
        """The context variables of `group` (a CtxGroup of as many streams) step on the device from now on
        (gmx_chainstep_attach_ctx): once, before the first step, after attach_match.  A route names a variable per
        column, -1 leaves the column to the caller.  Afterwards the routed columns of `contexts`, `ind_contexts` and
        `match_contexts`, and `bit_contexts`, are ignored."""
        r = _lib.CtxStepRoutes()
        keep = []
        for name, route in (("mixer", mixer_route), ("ind", ind_route), ("match", match_route)):
            if route is None:
                continue
            a = np.ascontiguousarray(route, np.int32)
            keep.append(a)
            setattr(r, name + "_route", a.ctypes.data_as(C.POINTER(C.c_int32)))
            setattr(r, "n_" + name + "_route", len(a))
        check(self.L.gmx_chainstep_attach_ctx(self.h, group.h, C.byref(r)), "gmx_chainstep_attach_ctx")

    def attach_decoder(self, ppmd_slot):
        """The arithmetic decoder and ModPPMD's range walk run on the device from now on
        (gmx_chainstep_attach_decoder): once, before the first step, after attach_match / attach_ctx.  Afterwards
        `take` [S], `decoder_ppm` [S][256], `decoded` [S] and `byte_p` [S][8] are views, and byte() decodes a whole byte
        of every stream with take[s] = 1."""
        check(self.L.gmx_chainstep_attach_decoder(self.h, int(ppmd_slot)), "gmx_chainstep_attach_decoder")
        S = self.g.S
        self.take = self._view("take", np.uint8, (S,))
        self.decoder_ppm = self._view("decoder_ppm", np.float32, (S, 256))
        self.decoded = self._view("decoded", np.uint8, (S,))
        self.byte_p = self._view("byte_p", np.float32, (S, 8))

    def set_input(self, stream, data, state=None):
        """The stream's compressed payload becomes resident on the device (gmx_chainstep_decoder_set_input).  state
        None: Decoder's constructor reads the four start bytes; (x1, x2, x, pos): resume, as decoder_state gave it."""
        buf = np.frombuffer(bytes(data), np.uint8)
        st = (C.c_uint32 * 4)(*[int(v) for v in state]) if state is not None else None
        check(self.L.gmx_chainstep_decoder_set_input(self.h, stream, buf.ctypes.data if len(buf) else None, len(buf), st),
              "gmx_chainstep_decoder_set_input")

    def decoder_state(self, stream):
        """(x1, x2, x, pos) of the stream's decoder after the last answered byte."""
        out = (C.c_uint32 * 4)()
        check(self.L.gmx_chainstep_decoder_state(self.h, stream, out), "gmx_chainstep_decoder_state")
        return tuple(int(v) for v in out)

    def byte(self):
        """Eight steps in one call for the streams with take[s] = 1 (gmx_chainstep_byte): `decoded` and `byte_p` hold
        the answers."""
        check(self.L.gmx_chainstep_byte(self.h), "gmx_chainstep_byte")

    def timed_byte(self):
        """byte() with HIP events around the byte's graph -> device milliseconds."""
        ms = C.c_float(0)
        check(self.L.gmx_chainstep_timed_byte(self.h, C.byref(ms)), "gmx_chainstep_timed_byte")
        return ms.value

    def byte_launch(self):
        check(self.L.gmx_chainstep_byte_launch(self.h), "gmx_chainstep_byte_launch")

    def byte_wait(self):
        check(self.L.gmx_chainstep_byte_wait(self.h), "gmx_chainstep_byte_wait")

    @property
    def bit_launches(self):
        """Per-bit graphs launched so far (gmx_debug_chainstep_bit_launches)."""
        return int(self.L.gmx_debug_chainstep_bit_launches(self.h))

    @property
    def commit_bytes(self):
        """Bytes of records per stream a commit moves (gmx_chainstep_commit_bytes)."""
        return int(self.L.gmx_chainstep_commit_bytes(self.h))

    def set_active(self, stream, active):
        """active[N] flags -> the stream's mask words."""
        padded = np.zeros(self.mask_words * 32, np.uint8)
        padded[:len(active)] = np.asarray(active) != 0
        self.active_mask[stream] = np.packbits(padded.reshape(self.mask_words, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)

    def commit(self, stream):
        """Optional: the stream's inputs for the coming step are complete (moved to the device now where the host can
        store there; step() does it for streams nobody committed)."""
        check(self.L.gmx_chainstep_commit(self.h, stream), "gmx_chainstep_commit")

    def step(self):
        check(self.L.gmx_chainstep_step(self.h), "gmx_chainstep_step")

    def timed_step(self):
        """step() with HIP events around the step's graph -> device milliseconds (gmx_chainstep_timed_step)."""
        ms = C.c_float(0)
        check(self.L.gmx_chainstep_timed_step(self.h, C.byref(ms)), "gmx_chainstep_timed_step")
        return ms.value

    def launch(self):
        """step() in two halves: queued when this returns ..."""
        check(self.L.gmx_chainstep_launch(self.h), "gmx_chainstep_launch")

    def wait(self):
        """... p and outputs in place when this does."""
        check(self.L.gmx_chainstep_wait(self.h), "gmx_chainstep_wait")

    def close(self):
        if getattr(self, "h", None):
            self.L.gmx_chainstep_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Encoder:
    """The reference's arithmetic Encoder for S streams on the device (gmx_encoder, include/gmxmix_encoder.h): codes a
    Batch's device bits and p, or host arrays, and returns each stream's bytes."""

    def __init__(self, n_streams, max_bits, device=0):
        self.L = _lib.lib()
        self.S = int(n_streams)
        self.max_bits = int(max_bits)
        h = C.c_void_p()
        check(self.L.gmx_encoder_create(C.byref(h), self.S, self.max_bits, device), "gmx_encoder_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.gmx_encoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _counts(self, n_bits):
        n = np.full(self.S, n_bits, np.uint64) if np.isscalar(n_bits) else np.ascontiguousarray(n_bits, np.uint64)
        assert n.shape == (self.S,)
        return n

    def reset(self, stream=-1, state=None):
        """stream -1: all.  state None: a new file; otherwise the two words of a checkpoint."""
        st = None if state is None else (C.c_uint32 * 2)(int(state[0]), int(state[1]))
        check(self.L.gmx_encoder_reset(self.h, stream, st), "gmx_encoder_reset")

    def state(self, stream):
        out = (C.c_uint32 * 2)()
        check(self.L.gmx_encoder_state(self.h, stream, out), "gmx_encoder_state")
        return int(out[0]), int(out[1])

    def encode_batch(self, batch, n_bits, timed=False):
        """Bits [0, n_bits[s]) of every stream from the batch's device arrays (an int: every stream)."""
        n = self._counts(n_bits)
        ms = C.c_float(0)
        check(self.L.gmx_encoder_encode_batch(self.h, batch.h, n.ctypes.data_as(C.POINTER(C.c_uint64)),
                                              C.byref(ms) if timed else None), "gmx_encoder_encode_batch")
        return ms.value if timed else None

    def encode(self, p, bits, n_bits):
        """Host arrays p [S][pitch] float32, bits [S][pitch] uint8."""
        p = np.ascontiguousarray(p, np.float32)
        bits = np.ascontiguousarray(bits, np.uint8)
        assert p.ndim == 2 and p.shape == bits.shape and p.shape[0] == self.S
        n = self._counts(n_bits)
        check(self.L.gmx_encoder_encode(self.h, _vp(p), _vp(bits), p.shape[1], n.ctypes.data_as(C.POINTER(C.c_uint64))),
              "gmx_encoder_encode")

    def flush(self, which=None):
        w = None if which is None else np.ascontiguousarray(np.asarray(which) != 0, np.uint8)
        assert w is None or w.shape == (self.S,)
        check(self.L.gmx_encoder_flush(self.h, _vp(w)), "gmx_encoder_flush")

    def take_launch(self):
        check(self.L.gmx_encoder_take_launch(self.h), "gmx_encoder_take_launch")

    def _taken(self):
        out = []
        for s in range(self.S):
            n = self.L.gmx_encoder_n_bytes(self.h, s)
            out.append(C.string_at(self.L.gmx_encoder_bytes(self.h, s), n) if n else b"")
        return out

    def take_wait(self):
        rc = self.L.gmx_encoder_take_wait(self.h)
        self.last_taken = self._taken() if rc in (0, -1) else None
        check(rc, "gmx_encoder_take_wait")   # (a bad p: GmxError, the other streams' bytes are in last_taken)
        return self.last_taken

    def take(self):
        """Everything coded since the last take: a list of bytes, one per stream."""
        self.take_launch()
        return self.take_wait()

    def total_bytes(self, stream):
        return int(self.L.gmx_encoder_total_bytes(self.h, stream))

    def bad_bit(self, stream):
        return int(self.L.gmx_encoder_bad_bit(self.h, stream))

    def d2h_bytes(self):
        return int(self.L.gmx_debug_encoder_d2h_bytes(self.h))


AN_INPUT, AN_MIXER, AN_FINAL_P = 0, 1, 2


class Analysis:
    """The reference's analysis averages (Predictor::RunAnalysis / UpdateEntropy) for S streams x C columns on the device
    (gmx_analysis, include/gmxmix_analysis.h): updated from a Batch's device arrays, or host arrays; a take returns the
    averages and the rows of analysis/entropy.tsv captured since the last take."""

    def __init__(self, n_streams, columns, max_samples, device=0):
        """columns: [(kind, index), ...] with kind AN_INPUT, AN_MIXER or AN_FINAL_P."""
        self.L = _lib.lib()
        self.S = int(n_streams)
        self.columns = [(int(k), int(i)) for k, i in columns]
        self.C = len(self.columns)
        cols = np.array(self.columns, np.uint32).reshape(-1, 2)
        h = C.c_void_p()
        check(self.L.gmx_analysis_create(C.byref(h), self.S, _vp(cols), self.C, int(max_samples), device),
              "gmx_analysis_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.gmx_analysis_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _counts(self, n_bits):
        n = np.full(self.S, n_bits, np.uint64) if np.isscalar(n_bits) else np.ascontiguousarray(n_bits, np.uint64)
        assert n.shape == (self.S,)
        return n

    def reset(self, stream=-1, ema=None, bits_seen=0):
        """stream -1: all.  ema None: zeros; otherwise the C averages of a checkpoint."""
        e = None if ema is None else np.ascontiguousarray(ema, np.float64)
        assert e is None or e.shape == (self.C,)
        check(self.L.gmx_analysis_reset(self.h, stream, _vp(e), int(bits_seen)), "gmx_analysis_reset")

    def set_frequency(self, frequency, stream=-1):
        check(self.L.gmx_analysis_set_frequency(self.h, stream, int(frequency)), "gmx_analysis_set_frequency")

    def update_batch(self, batch, n_bits, timed=False):
        """Bits [0, n_bits[s]) of every stream from the batch's device arrays (an int: every stream)."""
        n = self._counts(n_bits)
        ms = C.c_float(0)
        check(self.L.gmx_analysis_update_batch(self.h, batch.h, n.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               C.byref(ms) if timed else None), "gmx_analysis_update_batch")
        return ms.value if timed else None

    def update(self, values, bits, n_bits):
        """Host arrays values [S][pitch][C] float32 (a logit per column, a probability for AN_FINAL_P), bits [S][pitch]."""
        values = np.ascontiguousarray(values, np.float32)
        bits = np.ascontiguousarray(bits, np.uint8)
        assert values.ndim == 3 and values.shape == bits.shape + (self.C,) and bits.shape[0] == self.S
        n = self._counts(n_bits)
        check(self.L.gmx_analysis_update(self.h, _vp(values), _vp(bits), bits.shape[1],
                                         n.ctypes.data_as(C.POINTER(C.c_uint64))), "gmx_analysis_update")

    def take_launch(self):
        check(self.L.gmx_analysis_take_launch(self.h), "gmx_analysis_take_launch")

    def take_wait(self):
        """[(ema [C] float64, bits_seen, rows [k][C] float64, labels [k] uint64)] per stream (copies)."""
        check(self.L.gmx_analysis_take_wait(self.h), "gmx_analysis_take_wait")
        out = []
        for s in range(self.S):
            k = int(self.L.gmx_analysis_n_samples(self.h, s))
            ema = np.frombuffer(C.string_at(self.L.gmx_analysis_ema(self.h, s), 8 * self.C), np.float64)
            rows = np.zeros((0, self.C), np.float64)
            labels = np.zeros(0, np.uint64)
            if k:
                rows = np.frombuffer(C.string_at(self.L.gmx_analysis_samples(self.h, s), 8 * self.C * k),
                                     np.float64).reshape(k, self.C)
                labels = np.frombuffer(C.string_at(self.L.gmx_analysis_sample_bits(self.h, s), 8 * k), np.uint64)
            out.append((ema, int(self.L.gmx_analysis_bits_seen(self.h, s)), rows, labels))
        return out

    def take(self):
        self.take_launch()
        return self.take_wait()

    def d2h_bytes(self):
        return int(self.L.gmx_debug_analysis_d2h_bytes(self.h))


PPMD_PPM, PPMD_PREDICTIONS, PPMD_USED, PPMD_ALL = 1, 2, 4, 7


class PpmdGroup:
    """The reference's PPMD::ModPPMD for S streams on the device (gmx_ppmd, include/gmxmix_ppmd.h): per byte the
    normalised byte distribution, the model's eight bit predictions and its memory usage."""

    def __init__(self, n_streams, order=20, arena_mb=64, device=0):
        self.L = _lib.lib()
        self.S, self.order, self.arena_mb = int(n_streams), int(order), int(arena_mb)
        h = C.c_void_p()
        check(self.L.gmx_ppmd_create(C.byref(h), self.S, self.order, self.arena_mb, device), "gmx_ppmd_create")
        self.h = h
        ptr = self.L.gmx_ppmd_step_ppm(self.h)
        buf = (C.c_byte * (self.S * 1024)).from_address(ptr)
        self.step_ppm = np.frombuffer(buf, dtype=np.float32).reshape(self.S, 256)

    def close(self):
        if getattr(self, "h", None):
            self.step_ppm = None
            self.L.gmx_ppmd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def bank_bytes(self):
        return int(self.L.gmx_ppmd_bank_bytes(self.h))

    def reset(self, stream=-1):
        check(self.L.gmx_ppmd_reset(self.h, stream), "gmx_ppmd_reset")

    def sync(self):
        check(self.L.gmx_ppmd_sync(self.h), "gmx_ppmd_sync")

    def run(self, batch, n_bytes=None, timed=False):
        """The first n_bytes records of every stream; an array: n_bytes[s] of stream s (0 sits the call out)."""
        if n_bytes is None:
            n_bytes = batch.max_bytes
        if np.isscalar(n_bytes):
            ms = C.c_float(0)
            check(self.L.gmx_ppmd_run(self.h, batch.h, int(n_bytes), C.byref(ms) if timed else None), "gmx_ppmd_run")
            return ms.value if timed else None
        n = np.ascontiguousarray(n_bytes, np.uint64)
        assert n.shape == (self.S,)
        check(self.L.gmx_ppmd_run_ragged(self.h, batch.h, n.ctypes.data_as(C.POINTER(C.c_uint64))), "gmx_ppmd_run_ragged")
        return None

    def feed(self, batch, n_bytes, lstm_batch=None, mixer_batch=None, slot=0):
        check(self.L.gmx_ppmd_feed(self.h, batch.h, int(n_bytes), lstm_batch.h if lstm_batch is not None else None,
                                   mixer_batch.h if mixer_batch is not None else None, int(slot)), "gmx_ppmd_feed")

    def step_launch(self, last_byte, take=None):
        last = np.ascontiguousarray(last_byte, np.uint8)
        take = np.ones(self.S, np.uint8) if take is None else np.ascontiguousarray(take, np.uint8)
        assert last.shape == take.shape == (self.S,)
        check(self.L.gmx_ppmd_step_launch(self.h, _vp(last), _vp(take)), "gmx_ppmd_step_launch")

    def step_wait(self):
        check(self.L.gmx_ppmd_step_wait(self.h), "gmx_ppmd_step_wait")
        return self.step_ppm

    def step(self, last_byte, take=None):
        """UpdateByte(last_byte[s]) and PrepareByte of every stream with take[s] != 0 -> ppm [S][256] (the bank's pinned
        array: a view, overwritten by the next step)."""
        self.step_launch(last_byte, take)
        return self.step_wait()

    def memory_usage(self, stream):
        return int(self.L.gmx_ppmd_memory_usage(self.h, stream))

    def restores(self, stream):
        return int(self.L.gmx_ppmd_restores(self.h, stream))

    def launches(self):
        return int(self.L.gmx_debug_ppmd_launches(self.h))


class PpmdBatch:
    def __init__(self, group, max_bytes):
        self.g = group
        self.L = group.L
        self.max_bytes = int(max_bytes)
        h = C.c_void_p()
        check(self.L.gmx_ppmd_batch_create(C.byref(h), group.h, self.max_bytes), "gmx_ppmd_batch_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.gmx_ppmd_batch_destroy(self.h)
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
    def bytes(self):
        return self._view(self.L.gmx_ppmd_batch_bytes, np.uint8, (self.g.S, self.max_bytes))

    @property
    def ppm(self):
        return self._view(self.L.gmx_ppmd_batch_ppm, np.float32, (self.g.S, self.max_bytes, 256))

    @property
    def predictions(self):
        return self._view(self.L.gmx_ppmd_batch_predictions, np.float32, (self.g.S, self.max_bytes, 8))

    @property
    def active(self):
        return self._view(self.L.gmx_ppmd_batch_active, np.uint8, (self.g.S, self.max_bytes, 8))

    @property
    def used(self):
        return self._view(self.L.gmx_ppmd_batch_used, np.uint64, (self.g.S, self.max_bytes))

    def upload(self, n_bytes=None):
        check(self.L.gmx_ppmd_batch_upload(self.h, self.max_bytes if n_bytes is None else n_bytes), "gmx_ppmd_batch_upload")

    def download(self, n_bytes=None, what=PPMD_ALL):
        check(self.L.gmx_ppmd_batch_download(self.h, self.max_bytes if n_bytes is None else n_bytes, what),
              "gmx_ppmd_batch_download")

    def wait(self):
        check(self.L.gmx_ppmd_batch_wait(self.h), "gmx_ppmd_batch_wait")
