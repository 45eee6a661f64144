"""Shared by the tests of the lock step's byte calls (gmx_chainstep_byte, include/gmxmix_decoder.h): a Python restatement
of the reference's Decoder (coder/decoder.cpp) and of ModPPMD's range walk (mod_ppmd.cpp:1662-1681) that drives the
existing per-bit path gmx_chainstep_step -- the yardstick -- the chains both paths run on, and the two drivers.  A
stream's answers are logged per byte: the byte, the eight p (bit patterns) and the coder state behind it."""
import ctypes as C
import ctypes.util

import numpy as np

import ctx_common as cc
import goldenlib
import match_common as mc
import test_gpu_chainstep_match as tm
import test_gpu_ctx_targets as tt
from gmix_amd import Topology, topology

LEARN, PREDICT = 1, 2
GARBAGE = 0xDEADBEEF
F32 = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


class PyDecoder:
    """coder/decoder.cpp.  state: (x1, x2, x, pos) to resume from (ReadCheckpoint plus the read position)."""

    def __init__(self, data, state=None):
        self.data = bytes(data)
        if state is None:
            self.x1, self.x2, self.x, self.pos = 0, 0xFFFFFFFF, 0, 0
            for _ in range(4):
                self.x = ((self.x << 8) + self.read()) & 0xFFFFFFFF
        else:
            self.x1, self.x2, self.x, self.pos = (int(v) for v in state)

    def read(self):
        if self.pos >= len(self.data):
            return 0
        self.pos += 1
        return self.data[self.pos - 1]

    def next(self, p):
        pr = int(F32(1) + F32(65534) * F32(p))   # Discretize: float multiply, float add, truncation
        r = self.x2 - self.x1
        xmid = (self.x1 + (r >> 16) * pr + (((r & 0xFFFF) * pr) >> 16)) & 0xFFFFFFFF
        if self.x <= xmid:
            bit, self.x2 = 1, xmid
        else:
            bit, self.x1 = 0, (xmid + 1) & 0xFFFFFFFF
        while ((self.x1 ^ self.x2) & 0xFF000000) == 0:
            self.x1 = (self.x1 << 8) & 0xFFFFFFFF
            self.x2 = ((self.x2 << 8) + 255) & 0xFFFFFFFF
            self.x = ((self.x << 8) + self.read()) & 0xFFFFFFFF
        return bit

    def state(self):
        return (self.x1, self.x2, self.x, self.pos)


class Known:
    """The encoder's side: the bits are known, p is only recorded."""

    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8))
        self.t = 0
        self.p = []

    def next(self, p):
        self.p.append(F32(p))
        self.t += 1
        return int(self.bits[self.t - 1])

    def state(self):
        return (0, 0, 0, 0)


def logit(p):
    """Sigmoid::Logit (sigmoid.cpp:7-13): double comparisons, float clamp constants, float division, libm's logf."""
    p = F32(p)
    if float(p) < 0.0001:
        p = F32(0.0001)
    elif float(p) > 0.9999:
        p = F32(0.9999)
    return F32(_libm.logf(F32(p / (F32(1) - p))))


class PyWalk:
    """ModPPMD::Predict without PPMd: top_ / mid_ / bot_, the two std::accumulate sums, SetPrediction.  `slot` keeps its
    value over a silent bit (denom == 0)."""

    def __init__(self):
        self.top, self.mid, self.bot = 255, 127, 0
        self.slot, self.active = F32(0), False

    def step(self, ppm, opens, new_bit):
        if opens:
            self.top, self.bot = 255, 0
        elif new_bit:
            self.bot = self.mid + 1
        else:
            self.top = self.mid
        self.mid = self.bot + (self.top - self.bot) // 2
        num = F32(0)
        for v in ppm[self.mid + 1:self.top + 1]:
            num = F32(num + v)
        denom = num
        for v in ppm[self.bot:self.mid + 1]:
            denom = F32(denom + v)
        self.active = False
        if denom != 0:
            p = F32(num / denom)
            self.slot = logit(p)
            self.active = bool(p != F32(0.5))


class Stream:
    def __init__(self, src, data=None):
        self.src, self.data = src, data
        self.walk = PyWalk()
        self.pending, self.last_bit, self.k = False, 0, 0
        self.on_device = False        # the coder state the device holds is the newer one
        self.bytes, self.p, self.states = [], [], []

    def log(self):
        return (list(self.bytes), [tuple(int(v) for v in row) for row in self.p], list(self.states))


class Rig:
    """One chain: the mixers, the Indirect models, the Match models, the context bank, optionally the LSTM, and the
    lock-step object with all of them attached.  shape "small": 40 inputs, six general mixers, five Indirect and eight
    Match models, ctx_tiny's 17 variables; "stock": the reference's own shape."""

    def __init__(self, gpu, shape, S, with_lstm=False, decoder=True, lstm_seed=23):
        self.S, self.shape = S, shape
        self.lg = None
        if shape == "small":
            f = cc.fixture("ctx_tiny")
            fm = mc.fixture("match_k8")
            _, z = goldenlib.load("ind_tiny_dense")
            self.topo = Topology(40, tm.MIXERS, (1,))
            self.mixer_route = [-1, 13, -1, -1, 14, 16]   # columns 0, 2, 3 are longest_match (tm.COLS)
            self.ind_route = [0, 1, 2, 5, 4]
            self.match_route = [4, 11, 3, 5, 12, 2, 9, 7]
            self.cols = tm.COLS
            self.ppmd_slot = 11
            used = set(tm.MSLOTS) | {i for ab in tm.IND_SLOTS for i in ab}
            self.cg = gpu.CtxGroup(f.descs, S)
            self.xg = gpu.MatchGroup([(t, fm.limit, sl) for t, sl in zip(fm.tables, tm.MSLOTS)], 1024, S)
            self.ig = gpu.IndirectGroup(tm.IND_MODELS, z["ns_next"], z["rm_next"], S, slots=tm.IND_SLOTS)
            self.mg = gpu.MixerGroup(self.topo, S)
            self.cs = gpu.ChainStep(self.mg, self.ig)
        else:
            st = tt.stock()
            _, z = goldenlib.load("ind_stock41")
            islots = [(2 + 2 * i, 3 + 2 * i) for i in range(32)] + [(72 + 2 * j, 73 + 2 * j) for j in range(9)]
            self.topo = topology.stock(90)
            self.mixer_route, self.ind_route, self.match_route = st["mr"], st["ir"], st["xr"]
            self.cols = topology.stock_longest_match_columns()
            self.ppmd_slot = 0
            used = set(topology.STOCK_MATCH_SLOTS) | {i for ab in islots for i in ab} | {1}
            self.cg = gpu.CtxGroup(st["descs"], S)
            self.xg = gpu.MatchGroup(topology.stock_match(), 512, S)
            self.ig = gpu.IndirectGroup(topology.stock_indirect(), z["ns_next"], z["rm_next"], S, slots=islots)
            self.mg = gpu.MixerGroup(self.topo, S)
            if with_lstm:
                self.lg = gpu.LstmGroup(S)
                rng = np.random.default_rng(lstm_seed)
                w0 = ((rng.random((3, 50, 563), dtype=np.float32) - 0.5) * 0.2).astype(np.float32)
                for s in range(S):
                    self.lg.set_weights(w0, stream=s)
                self.cs = gpu.ChainStep(self.mg, self.ig, self.lg, lstm_slot=1, mixer_ctx_col=22, ind_ctx_col=16)
            else:
                self.cs = gpu.ChainStep(self.mg, self.ig)
        assert self.ppmd_slot not in used
        self.cs.attach_match(self.xg, self.cols)
        self.cs.attach_ctx(self.cg, self.mixer_route, self.ind_route, self.match_route)
        if decoder:
            self.cs.attach_decoder(self.ppmd_slot)

    def ppm_view(self):
        return self.cs.ppm if self.lg is not None else getattr(self.cs, "decoder_ppm", None)

    def exports(self, s):
        """Everything a stream leaves behind in the banks."""
        e = dict(mixers=self.mg.export(s), indirect=self.ig.export(s), ind_slots=u32(self.ig.slot_values(s)).tobytes(),
                 match=self.xg.export(s), match_slots=(u32(self.xg.slot_values(s)[0]).tobytes(), self.xg.slot_values(s)[1]),
                 ctx=self.cg.export(s)[0], board=cc.board_bytes(self.cg.blackboard(s)))
        if self.lg is not None:
            e["lstm"] = self.lg.export(s)
        return e

    def close(self):
        self.cs.close()
        for h in (self.lg, self.cg, self.xg, self.ig, self.mg):
            if h is not None:
                h.close()


def make_ppm(S, n_bytes, seed):
    """PPMd's stand-in: a byte distribution per stream and byte.  Every sixth is uniform (p == 0.5 at every bit: the slot
    is inactive), every sixth has no mass above 127 (denom == 0 once a decoded bit leads there: silent bits)."""
    rng = np.random.default_rng(seed)
    ppm = rng.random((S, n_bytes, 256), dtype=np.float32) + np.float32(1e-3)
    ppm[:, 2::6] = 1.0
    ppm[:, 4::6, 128:] = 0.0
    ppm /= ppm.sum(axis=2, keepdims=True, dtype=np.float32)
    return ppm.astype(np.float32)


def _garbage(cs):
    """No context is the caller's: whatever the staging arrays hold is ignored."""
    cs.contexts[:] = GARBAGE
    cs.ind_contexts[:] = GARBAGE
    cs.bit_contexts[:] = GARBAGE
    cs.match_contexts[:] = GARBAGE


def learn_only(rig, st, who):
    """A GMX_STEP_LEARN-only step for the streams of `who` whose Learn is outstanding."""
    cs = rig.cs
    who = [s for s in who if st[s].pending]
    if not who:
        return
    cs.what[:] = 0
    cs.bits[:] = 0
    for s in who:
        cs.what[s] = LEARN
        cs.bits[s] = st[s].last_bit
        st[s].pending = False
    _garbage(cs)
    cs.step()


def bits_round(rig, st, group, ppm, step=None):
    """One byte of the streams in `group` through eight per-bit steps, the host decoding (the yardstick).  Streams outside
    the group whose Learn is outstanding learn alone in the first step (they may not sit a step out)."""
    cs, slot = rig.cs, rig.ppmd_slot
    view = rig.ppm_view()
    for s in group:
        if st[s].on_device:      # the device decoded this stream's last bytes: go on from its state
            st[s].src = PyDecoder(st[s].data, cs.decoder_state(s))
            st[s].on_device = False
    for j in range(8):
        cs.what[:] = 0
        cs.bits[:] = 0
        cs.predictions[:] = 0
        cs.active_mask[:] = 0
        for s in range(rig.S):
            x = st[s]
            if s in group:
                row = ppm[s][x.k]
                if j == 0 and view is not None:
                    view[s] = row
                x.walk.step(row, j == 0, x.last_bit)
                cs.predictions[s, slot] = x.walk.slot
                if x.walk.active:
                    cs.active_mask[s, slot >> 5] = 1 << (slot & 31)
                cs.what[s] = PREDICT | (LEARN if x.pending else 0)
                cs.bits[s] = x.last_bit if x.pending else 0
            elif x.pending:
                cs.what[s] = LEARN
                cs.bits[s] = x.last_bit
                x.pending = False
        _garbage(cs)
        (step or cs.step)()
        for s in group:
            x = st[s]
            p = F32(cs.p[s])
            if j == 0:
                x.p.append([])
                x.acc = 0
            x.p[-1].append(int(p.view(np.uint32)))
            x.last_bit = x.src.next(p)
            x.acc = (x.acc << 1) | x.last_bit
            x.pending = True
    for s in group:
        x = st[s]
        x.bytes.append(x.acc)
        x.states.append(x.src.state())
        x.k += 1


def byte_begin(rig, st, group, ppm, call=None):
    """The first half of byte_round: everything up to the call (gmx_chainstep_byte, or byte_launch)."""
    cs = rig.cs
    if any(st[s].pending for s in range(rig.S) if s not in group):
        # a stream outside the group has to close its Learn in a per-bit step, which no stream with a Learn outstanding
        # may sit out: everybody learns in it, and the takers begin their byte with nothing outstanding
        learn_only(rig, st, range(rig.S))
    cs.take[:] = 0
    cs.bits[:] = 0
    for s in group:
        x = st[s]
        if not x.on_device and x.k > 0 and isinstance(x.src, PyDecoder):   # the host decoded its last bytes
            cs.set_input(s, x.data, x.src.state())
        cs.take[s] = 1
        cs.decoder_ppm[s] = ppm[s][x.k]
        if x.pending and not x.on_device:
            cs.bits[s] = x.last_bit
    _garbage(cs)
    (call or cs.byte)()


def byte_end(rig, st, group):
    """... and the answers, once they are there."""
    cs = rig.cs
    for s in group:
        x = st[s]
        byte = int(cs.decoded[s])
        x.bytes.append(byte)
        x.p.append([int(v) for v in cs.byte_p[s].view(np.uint32)])
        x.states.append(cs.decoder_state(s))
        x.last_bit, x.pending, x.on_device = byte & 1, True, True
        x.k += 1


def byte_round(rig, st, group, ppm):
    """One byte of the streams in `group` through ONE byte call (a learn-only step in front of it where a stream outside
    the group has a Learn outstanding)."""
    byte_begin(rig, st, group, ppm)
    byte_end(rig, st, group)


def decode_streams(rig, inputs):
    st = [Stream(PyDecoder(d), d) for d in inputs]
    if hasattr(rig.cs, "take"):
        for s, d in enumerate(inputs):
            rig.cs.set_input(s, d)
    return st


def assert_same(st_a, st_b, rig_a, rig_b, streams=None):
    for s in (range(len(st_a)) if streams is None else streams):
        a, b = st_a[s].log(), st_b[s].log()
        assert a[0] == b[0], ("bytes", s, a[0], b[0])
        assert a[1] == b[1], ("p", s)
        assert a[2] == b[2], ("coder state", s)
        ea, eb = rig_a.exports(s), rig_b.exports(s)
        for k in ea:
            assert ea[k] == eb[k], (k, s)
