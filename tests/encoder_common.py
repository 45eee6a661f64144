"""What the encoder's tests share: PyEncoder, a plain restatement of the reference's Encoder with the state exposed,
the operand mixture, and the operand sets the GPU tests code (tests/test_encoder_census.py checks what they hold)."""
import numpy as np

M32 = 0xffffffff
EPS = np.float32(0.0001)
LO, HI = EPS, np.float32(1.0) - EPS
# a state from which a 1 bit emits four bytes
FOUR = (0x12ffffff, 0x13000000)


def discretize(p):
    """Encoder::Discretize: 1 + 65534 * p in float, truncated."""
    return int(np.float32(1.0) + np.float32(65534.0) * np.float32(p))


def p_ok(p):
    p = np.float32(p)
    return bool(p >= 0 and p <= 1)


class PyEncoder:
    def __init__(self, state=None):
        self.x1, self.x2 = (0, M32) if state is None else (int(state[0]), int(state[1]))
        self.out = bytearray()

    @property
    def state(self):
        return (self.x1, self.x2)

    def _shift(self):
        k = 0
        while ((self.x1 ^ self.x2) & 0xff000000) == 0:
            self.out.append(self.x2 >> 24)
            self.x1 = (self.x1 << 8) & M32
            self.x2 = ((self.x2 << 8) & M32) | 255
            k += 1
        return k

    def encode(self, bit, p):
        """Returns the number of bytes the bit emitted."""
        pr = discretize(p)
        r = (self.x2 - self.x1) & M32
        xmid = (self.x1 + (r >> 16) * pr + (((r & 0xffff) * pr) >> 16)) & M32
        if bit:
            self.x2 = xmid
        else:
            self.x1 = (xmid + 1) & M32
        return self._shift()

    def run(self, bits, p):
        """Codes until the first bad p; returns its index or -1."""
        for t, (b, q) in enumerate(zip(bits, p)):
            if not p_ok(q):
                return t
            self.encode(int(b), q)
        return -1

    def flush(self):
        k = self._shift()
        self.out.append(self.x2 >> 24)
        return k + 1


def mixture(n, seed):
    """p drawn from {0, 1e-4, 0.5, 1 - 1e-4, 1, uniform}, random bits."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 6, n)
    p = rng.random(n, dtype=np.float32)
    for k, v in enumerate((np.float32(0), LO, np.float32(0.5), HI, np.float32(1))):
        p[kind == k] = v
    bits = rng.integers(0, 2, n).astype(np.uint8)
    return p.astype(np.float32), bits


def emit_counts(bits, p, state=None):
    e = PyEncoder(state)
    return np.array([e.encode(int(b), q) for b, q in zip(bits, p)])


# ---- the operand sets of tests/test_gpu_encoder.py -----------------------------------------------------------------
S, T = 70, 300
COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]


def gpu_operands(seed=11):
    """p [S][T], bits [S][T] of the mixture and the per-stream counts: the listed ones, then random ones."""
    p = np.zeros((S, T), np.float32)
    bits = np.zeros((S, T), np.uint8)
    for s in range(S):
        p[s], bits[s] = mixture(T, seed * 1000 + s)
    rng = np.random.default_rng(seed)
    n = np.array(COUNTS + rng.integers(0, T + 1, S - len(COUNTS)).tolist(), np.uint64)
    n[64:] = [300, 1, 0, 129, 64, 257]  # the second wave's six live lanes take other paths than one another
    return p, bits, n


# Constructed states: from KIN[k - 1] a 1 bit at p = 0.5 emits exactly k bytes (xmid lands on 0x12ffffff, and x1 agrees
# with it in its top k bytes).  The last is the four-byte state of the fixture's resumed run.
KIN = [(0x12000000, 0x13ffffff), (0x12ff0000, 0x1300ffff), (0x12ffff00, 0x130000ff), (0x12ffffff, 0x13000000)]
