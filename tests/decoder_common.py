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


def discretize(p):
    """Decoder::Discretize: float multiply, float add, truncation (a scalar or an array of float32)."""
    return (F32(1) + F32(65534) * np.asarray(p, F32)).astype(np.uint32)


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
        return self.next_pr(int(discretize(p)))

    def next_pr(self, pr):
        """Decode behind Discretize."""
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
        self.predict(ppm)

    def predict(self, ppm):
        """The bit prediction of [bot, top]; returns whether the slot was written."""
        self.mid = self.bot + (self.top - self.bot) // 2
        num = F32(0)
        for v in ppm[self.mid + 1:self.top + 1]:
            num = F32(num + v)
        denom = num
        for v in ppm[self.bot:self.mid + 1]:
            denom = F32(denom + v)
        self.active = False
        self.num, self.denom = num, denom
        if denom != 0:
            p = F32(num / denom)
            self.slot = logit(p)
            self.active = bool(p != F32(0.5))
        return bool(denom != 0)


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
    Match models, ctx_tiny's 17 variables; "stock": the reference's own shape.  n_inputs: another input count for
    "small" (the models keep their slots); ppmd_slot: another free slot for ModPPMD."""

    def __init__(self, gpu, shape, S, with_lstm=False, decoder=True, lstm_seed=23, n_inputs=None, ppmd_slot=None):
        self.S, self.shape = S, shape
        self.lg = None
        if shape == "small":
            f = cc.fixture("ctx_tiny")
            fm = mc.fixture("match_k8")
            _, z = goldenlib.load("ind_tiny_dense")
            self.topo = Topology(40 if n_inputs is None else n_inputs, tm.MIXERS, (1,))
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
        assert n_inputs is None or shape == "small"
        if ppmd_slot is not None:
            self.ppmd_slot = ppmd_slot
        assert self.ppmd_slot not in used and 0 <= self.ppmd_slot < self.topo.n_inputs
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


# ---- operands for the device probe of gmx_coder.h (gmx_debug_math_probe, what = 12 and 13; tests/test_gpu_coder_device.py) --
# A decode tuple is six words {x1, x2, x, p (bit pattern), next4, avail}: next4 packs the next four input bytes, the
# first in its low byte, of which the input holds only `avail`.  What Decode makes of it is six words too:
# {bit, x1, x2, x, bytes consumed, pr}.
PROBE_DECODE, PROBE_WALK = 12, 13
WALK_SENTINEL = 0xC2F60000                 # -123.0f: what the probe presets the slot to
EDGE_PR = (7, 8, 32767, 32768, 32769, 65527, 65528)
EDGE_RANGES = (0, 1, 255, 256, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 32) - 1)
M32 = 0xFFFFFFFF


def f2u(v):
    return int(F32(v).view(np.uint32))


def u2f(u):
    return np.uint32(u).view(F32)


def p_ends(pr):
    """The smallest and the largest float p in [0, 1] that Discretize takes to pr: it never decreases as p grows (a
    rounded multiply and a rounded add), so each end is a bisection over the bit patterns of the positive floats."""
    lo, hi = 0, f2u(1.0)                   # the least u with discretize(u) >= pr
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if int(discretize(u2f(mid))) >= pr else (mid + 1, hi)
    first = lo
    lo, hi = 0, f2u(1.0)                   # the least u with discretize(u) > pr
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if int(discretize(u2f(mid))) > pr else (mid + 1, hi)
    assert int(discretize(u2f(first))) == pr == int(discretize(u2f(lo - 1))), pr
    assert first == 0 or int(discretize(u2f(first - 1))) == pr - 1
    assert int(discretize(u2f(lo))) == pr + 1
    return first, lo - 1


def edge_p():
    """Bit patterns: both ends of every EDGE_PR, the clamps of Predictor::Predict -+ 1 ulp, 0.5."""
    out = [u for pr in EDGE_PR for u in p_ends(pr)]
    for v in (0.0001, 0.9999):
        out += [f2u(v) - 1, f2u(v), f2u(v) + 1]
    out.append(f2u(0.5))
    return sorted(set(out))


def xmid_of(x1, x2, pr):
    r = x2 - x1
    return (x1 + (r >> 16) * pr + (((r & 0xFFFF) * pr) >> 16)) & M32


def edge_x1(r):
    """Where a range of width r lies: at byte-aligned bases (a boundary of the top byte -- or, after one, two, three
    shifts, of the byte that is the top one by then -- outside it), straddling such a boundary, ending just below one,
    beginning on one, and at the top of the 32 bits."""
    out = [0, 0x12000000, 0x12340000, 0x12345600, 0x12345678, 0xFF000000, M32 - r]
    for q in (0x01000000, 0x80000000, 0x13000000, 0x12350000, 0x12345700, 0xFFFFFF00):
        out += [q - (r >> 1) - 1, q - r - 1, q]
    return sorted({v for v in out if 0 <= v and v + r <= M32})


def edge_tuples():
    """The constructed operands of Decode, [N][6] uint32: EDGE_RANGES x edge_x1 x edge_p x {x1, xmid - 1, xmid, xmid + 1,
    x2} (where inside [x1, x2]) x avail 0 .. 4, the input bytes seeded and never 0 (a read past the end shows)."""
    rng = np.random.default_rng(1234)
    ps = [(u, int(discretize(u2f(u)))) for u in edge_p()]
    rows = []
    for r in EDGE_RANGES:
        for x1 in edge_x1(r):
            x2 = x1 + r
            for pu, pr in ps:
                xm = xmid_of(x1, x2, pr)
                for x in sorted({v for v in (x1, xm - 1, xm, xm + 1, x2) if x1 <= v <= x2}):
                    for avail in range(5):
                        rows.append((x1, x2, x, pu, 0, avail))
    t = np.array(rows, np.uint32)
    t[:, 4] = rng.integers(1, 256, (len(t), 4), dtype=np.uint32) @ np.array([1, 1 << 8, 1 << 16, 1 << 24], np.uint32)
    return t


def random_tuples(n, seed):
    """x1 <= x <= x2 with the range's width spread over all 33 magnitudes; p from all of (0, 1), from the clamped
    interval's bit patterns, and the clamps and 0.5 themselves."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 1 << 32, n, dtype=np.uint64) >> rng.integers(0, 33, n, dtype=np.uint64)
    x1 = (rng.random(n) * (M32 - r + 1).astype(np.float64)).astype(np.uint64)
    x1 = np.minimum(x1, M32 - r)
    x = x1 + (rng.integers(0, 1 << 32, n, dtype=np.uint64) % (r + 1))
    lo, hi = f2u(0.0001), f2u(0.9999)
    p = rng.random(n, dtype=np.float32).view(np.uint32)
    kind = rng.integers(0, 8, n)
    p = np.where(kind < 3, rng.integers(lo, hi + 1, n, dtype=np.uint32), p)
    p = np.where(kind == 7, np.array([lo, hi, f2u(0.5), lo + 1], np.uint32)[rng.integers(0, 4, n)], p)
    t = np.zeros((n, 6), np.uint32)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = x1, x1 + r, x, p
    t[:, 4] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    t[:, 5] = rng.integers(0, 5, n)
    assert (t[:, 0] <= t[:, 2]).all() and (t[:, 2] <= t[:, 1]).all()
    return t


def trace_tuples(z):
    """tests/golden/decoder_trace.npz (the reference's own Decoder, recorded) as probe operands: for every bit t the state
    after t - 1, p[t] and the next four input bytes -> (tuples [N][6], expected [N][6]).  Bit and state are the recorded
    ones.  The trace has no read position: it is PyDecoder's, whose bits and states must first equal the recorded ones;
    pr is Discretize of the recorded p.  Behind a bit that shifted nothing follows the same range with x on the boundary
    that the recorded state names (below)."""
    tup, exp = [], []
    for name in (str(n) for n in z["names"]):
        data, pu = bytes(z[name + "_input"]), z[name + "_p"].astype(np.uint32)
        d = PyDecoder(data)
        for t in range(len(pu)):
            before = d.state()
            bit = d.next(pu[t].view(F32))
            x1, x2, x = (int(v) for v in z[name + "_state"][t])
            assert (bit, d.x1, d.x2, d.x) == (int(z[name + "_bits"][t]), x1, x2, x), (name, t)
            pos = before[3]
            nxt = data[pos:pos + 4]
            rest = (int(pu[t]), int.from_bytes(nxt.ljust(4, b"\xa5"), "little"), len(nxt))
            pr = int(discretize(pu[t].view(F32)))
            tup.append(before[:3] + rest)
            exp.append((bit, x1, x2, x, d.pos - pos, pr))
            # A random x never lies on the comparison's boundary, but the recorded state names it: where the bit
            # shifted nothing (x is unchanged and not 0), a recorded 1 left x2_ = xmid and a recorded 0 left
            # x1_ = xmid + 1.  The same range with x on that value gives the recorded bit, x1_ and x2_ again.
            if x == before[2] != 0:
                edge = x2 if bit else x1
                tup.append(before[:2] + (edge,) + rest)
                exp.append((bit, x1, x2, edge, 0, pr))
    return np.array(tup, np.uint32), np.array(exp, np.uint32)


def decode_expected(t):
    """PyDecoder on every tuple of t -> [N][6] uint32 {bit, x1, x2, x, consumed, pr}."""
    pr = discretize(t[:, 3].view(F32))     # (float32 multiply and add, as PyDecoder.next's)
    out = []
    for (x1, x2, x, _, next4, avail), k in zip(t.tolist(), pr.tolist()):
        d = PyDecoder(next4.to_bytes(4, "little")[:avail], (x1, x2, x, 0))
        bit = d.next_pr(k)
        out.append((bit, d.x1, d.x2, d.x, d.pos, k))
    return np.array(out, np.uint32).reshape(-1, 6)


def decode_census(t):
    """What the tuples of t exercise, by PyDecoder alone: how many shift 0 .. 4 bytes, how many have x == xmid,
    x == xmid + 1, a range below 65 536, a shift that reads past the input's end."""
    c = dict(shifts=[0] * 5, x_is_xmid=0, x_is_xmid_plus_1=0, narrow=0, reads_past_end=0)
    pr = discretize(t[:, 3].view(F32)).tolist()

    def bit_at(x1, x2, x, k):
        return PyDecoder(b"", (x1, x2, x, 0)).next_pr(k)
    for (x1, x2, x, _, next4, avail), k in zip(t.tolist(), pr):
        d = PyDecoder(b"\1\1\1\1", (x1, x2, x, 0))     # four spare bytes: pos counts the shifts
        bit = d.next_pr(k)
        c["shifts"][d.pos] += 1
        # x == xmid: the last x that decodes a 1; x == xmid + 1: the first that decodes a 0
        c["x_is_xmid"] += bit == 1 and x < M32 and bit_at(x1, x2, x + 1, k) == 0
        c["x_is_xmid_plus_1"] += bit == 0 and x > 0 and bit_at(x1, x2, x - 1, k) == 1
        c["narrow"] += (x2 - x1) >> 16 == 0
        c["reads_past_end"] += d.pos > avail
    return c


def probe_decode(L, t):
    """The tuples of t through the device's gmx_coder_decode -> [N][6] uint32 as decode_expected's."""
    x = np.zeros((len(t), 8), np.uint32)
    x[:, :6] = t
    y = np.full_like(x, GARBAGE)
    assert L.gmx_debug_math_probe(0, x.ctypes.data, y.ctypes.data, x.size, PROBE_DECODE) == 0
    assert not y[:, 6:].any()
    return y[:, :6]


def walk_pairs():
    """The 255 ranges [bot, top] with top > bot that eight bits can lead to."""
    out, level = [], [(255, 0)]
    while level:
        out += level
        nxt = []
        for top, bot in level:
            mid = bot + (top - bot) // 2
            nxt += [(t, b) for t, b in ((mid, bot), (top, mid + 1)) if t > b]
        level = nxt
    assert len(out) == 255 == len(set(out))
    return out


def walk_distributions():
    """[(name, ppm[256] float32)]: test_coder.cpp's distributions, then subnormal masses, a single mass, two masses
    1 ulp apart that a bit at every depth separates, and 200 random ones with zeros and mixed magnitudes."""
    out = [("uniform", np.full(256, F32(1) / F32(256), F32))]
    r = [88172645463325252]

    def rnd():                             # test_coder.cpp's xorshift64
        r[0] ^= (r[0] << 13) & 0xFFFFFFFFFFFFFFFF
        r[0] ^= r[0] >> 7
        r[0] ^= (r[0] << 17) & 0xFFFFFFFFFFFFFFFF
        return F32(F32((r[0] >> 40) & 0xFFFF) / F32(65536))
    out.append(("upper half zero", np.array([F32(rnd() + F32(1e-3)) if i < 128 else F32(0) for i in range(256)], F32)))
    ppm = np.array([F32(rnd() * F32(1e-7 if i % 7 == 0 else 1e3 if i % 5 == 0 else 1.0)) for i in range(256)], F32)
    ppm[[0, 16, 17, 32, 33, 34, 35, 64, 65, 66, 67, 68, 69, 70, 71, 200, 254, 255]] = 0
    out.append(("scattered zeros", ppm))
    out.append(("all zero", np.zeros(256, F32)))
    rng = np.random.default_rng(77)
    # 1e-45 .. 1e-38: bit patterns 1 .. 0x7fffff, the magnitude spread evenly over the 23 binades of the subnormals
    sub = ((1 << rng.integers(0, 23, 256)) | rng.integers(0, 1 << 22, 256)) & 0x7FFFFF
    out.append(("subnormal masses", np.maximum(sub, 1).astype(np.uint32).view(F32)))
    tiny = np.ones(256, F32)               # the quotient itself is subnormal: 2^-127 over 128
    tiny[128:] = 0
    tiny[255] = u2f(0x00400000)
    out.append(("subnormal quotient", tiny))
    for at in (0, 77, 255):
        one = np.zeros(256, F32)
        one[at] = 1
        out.append(("single mass at %d" % at, one))
    a, b = F32(0.3), u2f(f2u(0.3) + 1)
    for depth in range(8):
        for lo_mass, hi_mass in ((a, b), (b, a)):
            two = np.zeros(256, F32)
            two[0], two[(256 >> depth) - 1] = lo_mass, hi_mass
            out.append(("two masses 1 ulp apart, depth %d" % depth, two))
    for i in range(200):
        ppm = rng.random(256, dtype=np.float32)
        if i % 4 == 1:
            ppm *= F32(10) ** rng.integers(-8, 4, 256).astype(F32)
        if i % 4 == 2:
            ppm[rng.random(256) < 0.5] = 0
        if i % 4 == 3:
            lo = int(rng.integers(0, 200))
            ppm[lo:lo + int(rng.integers(1, 56))] = 0
        out.append(("random %d" % i, ppm.astype(F32)))
    return out


def walk_expected(ppm):
    """PyWalk on the 255 ranges over ppm -> ([255][3] uint32 {wrote, slot bits, active}, [(num, denom, p or None)])."""
    out, seen = np.zeros((255, 3), np.uint32), []
    for i, (top, bot) in enumerate(walk_pairs()):
        w = PyWalk()
        w.top, w.bot, w.slot = top, bot, u2f(WALK_SENTINEL)
        wrote = w.predict(ppm)
        # (a walk that writes nothing leaves the probe's presets: the sentinel, active = 1)
        out[i] = (1, f2u(w.slot), w.active) if wrote else (0, WALK_SENTINEL, 1)
        seen.append((w.num, w.denom, F32(w.num / w.denom) if wrote else None))
    return out, seen


def probe_walk(L, ppms):
    """Every range of walk_pairs over every distribution of ppms ([D][256]) through the device's
    gmx_coder_walk_predict -> [D][255][3] uint32."""
    pairs = np.array(walk_pairs(), np.uint32)
    x = np.zeros((len(ppms), 255, 260), np.uint32)
    x[:, :, 0:2] = pairs
    x[:, :, 4:] = np.ascontiguousarray(ppms, F32).view(np.uint32)[:, None, :]
    y = np.full_like(x, GARBAGE)
    assert L.gmx_debug_math_probe(0, x.ctypes.data, y.ctypes.data, x.size, PROBE_WALK) == 0
    assert not y[:, :, 3:].any()
    return y[:, :, :3]
