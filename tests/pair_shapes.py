"""Shapes of the register-resident kernel for any three-layer bank (gmix_amd/csrc/gmx_pair.hip): a seeded set that
covers every `n % 4`, both sides of every boundary between the kernel's instantiations (39|40, 103|104, 167|168
inputs), the narrowest and widest layers, the skip input at 0, 1, the middle and n-1, gate tables that are and are
not powers of two, and kernel_shapes.PATTERNS cycled (contexts above the tables, rows that persist, rows visited
more than 1024 times, silent inputs).  The CPU test pins the oracle to the reference's own Mixer on them, the GPU
test runs them through the kernel."""
import numpy as np

import kernel_shapes as ks
from gmix_amd import topology

PAIR = 4   # gmx_debug_kernel_kind of the kernel

# (n_inputs, l0, l1): the issue's input counts, the instantiations' boundaries, l0 in {1, 2, 7, 23, 24}, l1 in {1, 3, 8}
SHAPES = [
    (4, 1, 1), (5, 2, 3), (6, 7, 8), (7, 24, 1), (33, 23, 3), (39, 24, 8), (40, 5, 3), (89, 1, 8),
    (90, 24, 8), (91, 24, 8), (92, 2, 1), (93, 7, 3), (103, 23, 8), (104, 24, 1), (127, 1, 3), (128, 24, 8),
    (129, 2, 8), (167, 7, 1), (168, 23, 3), (200, 24, 8), (255, 1, 1), (256, 24, 8), (256, 2, 3), (4, 24, 8),
    (36, 7, 3), (100, 24, 3), (164, 23, 1), (7, 1, 8),
]
LONG_T = 2300   # pattern 5 alternates two contexts: every row is visited more than 1024 times


def topo_of(i):
    n, l0, l1 = SHAPES[i]
    rng = np.random.default_rng(12000 + i)
    pow2 = i % 3 == 1
    t0 = ks._tables(rng, l0, pow2, 2)
    t1 = ks._tables(rng, l1, pow2, 1)
    tf = int(rng.choice([1, 2, 4])) if pow2 else int(rng.choice([1, 2, 3, 5]))
    mixers = ([(0, t, ks.learning_rate(rng)) for t in t0] + [(1, t, ks.learning_rate(rng)) for t in t1] +
              [(2, tf, ks.learning_rate(rng))])
    return topology.Topology(n, mixers, skip=(ks.skip_index(i, n),))


def cases():
    """id -> (topology factory, T, first stream seed, synth kwargs, nolearn_from)."""
    out = {}
    for i, (n, l0, l1) in enumerate(SHAPES):
        kw = ks.pattern(i)
        T = LONG_T if i % len(ks.PATTERNS) == 5 else 380 + 23 * i
        out[f"n{n}_{l0}_{l1}_{i}"] = (lambda i=i: topo_of(i), T, 2001 + i, kw, None if i % 2 else T - 60)
    return out


def scale_topology():
    """128 inputs x 24/8/1 with tables of at most 8 rows: a thousand banks stay small."""
    rng = np.random.default_rng(12999)
    mixers = ([(0, t, ks.learning_rate(rng)) for t in ks._tables(rng, 24, False, 0, small=True)] +
              [(1, t, ks.learning_rate(rng)) for t in ks._tables(rng, 8, False, 0, small=True)] +
              [(2, 3, ks.learning_rate(rng))])
    return topology.Topology(128, mixers, skip=(64,))
