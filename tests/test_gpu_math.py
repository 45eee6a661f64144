"""Device scalar math == host scalar math (the same gmx_math.h), which tests/test_math.py
shows equals the reference's libm-based Sigmoid::Logistic: exhaustive over all float inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_device_math_equals_host_math_samples(gpu, oracle):
    L = gpu._lib.lib()
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.integers(0, 1 << 32, 2_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        np.linspace(-110, 95, 400001).astype(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 88.7228, -103.9721, -87.3], np.float32)])
    so = os.path.join(HERE, "helpers", "libmathcheck.so")
    if not os.path.exists(so):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared",
                               os.path.join(HERE, "helpers", "mathcheck.c"), "-o", so, "-lm"])
    H = C.CDLL(so)
    for what, hostfn in ((1, H.gmx_host_logistic_array), (2, H.gmx_host_squash_array)):
        y = np.zeros_like(x)
        assert L.gmx_debug_math_probe(0, x.ctypes.data, y.ctypes.data, len(x), what) == 0
        ref = np.zeros_like(x)
        hostfn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        hostfn(x.ctypes.data, ref.ctypes.data, len(x))
        same = (y.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(y) & np.isnan(ref))
        assert same.all(), x[~same][:5]
    # expf against libm directly
    y = np.zeros_like(x)
    assert L.gmx_debug_math_probe(0, x.ctypes.data, y.ctypes.data, len(x), 0) == 0
    ref = np.zeros_like(x)
    oracle.lib().gmxo_libm_expf_array(x.ctypes.data, ref.ctypes.data, len(x))
    same = (y.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(y) & np.isnan(ref))
    assert same.all(), x[~same][:5]


def test_device_logistic_exhaustive_checksum(gpu):
    """All 2^32 inputs: the device folds its results into a checksum; the host does the same
    with its own (libm-pinned) implementation."""
    L = gpu._lib.lib()
    src = os.path.join(HERE, "helpers", "rangecheck.c")
    so = os.path.join(HERE, "helpers", "librangecheck.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", src, "-o", so, "-lm"])
    H = C.CDLL(so)
    H.gmx_host_math_range.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_ulonglong)]
    for what in (0, 1, 2):
        dev = (C.c_ulonglong * 2)()
        host = (C.c_ulonglong * 2)()
        assert L.gmx_debug_math_range(0, 0, 1 << 32, what, dev) == 0
        H.gmx_host_math_range(0, 1 << 32, what, host)
        assert (dev[0], dev[1]) == (host[0], host[1]), what


def test_wave_level_short_ways_equal_the_general_expressions(gpu):
    """gmx_stock.hip's logistic and row-age division take shorter instruction sequences when a whole wave is in
    range (gmx_math.h, gmx_wave_*): the logistic over all 2^32 inputs folds to the same checksum as the general
    function (which the test above pins to libm), and the short double division equals the compiler's on 4096 x 4096
    small counter pairs and 2^32 hashed ones (what = 4 counts the differing results)."""
    L = gpu._lib.lib()
    gen = (C.c_ulonglong * 2)()
    short = (C.c_ulonglong * 2)()
    assert L.gmx_debug_math_range(0, 0, 1 << 32, 1, gen) == 0
    assert L.gmx_debug_math_range(0, 0, 1 << 32, 3, short) == 0
    assert (short[0], short[1]) == (gen[0], gen[1])
    bad = (C.c_ulonglong * 2)()
    assert L.gmx_debug_math_range(0, 0, (1 << 32) + (1 << 24), 4, bad) == 0
    assert (bad[0], bad[1]) == (0, 0), "short row-age division differs on %d pairs (xor of 1 + their indices: %d)" % (bad[1], bad[0])


# ---- the LSTM byte model's scalar math on the device (gmx_lstm.hip) ------------------------------------------------
# what values of gmx_debug_math_probe / gmx_debug_math_range (gmx_aux.hip)
LSTM_WHAT = {"logf": 5, "logit": 6, "expm1f": 7, "tanhf": 8, "logistic_lds_table": 9, "norm_scale": 10}


def _helper(name):
    """tests/helpers/<name>.c as a shared library, rebuilt when a source is newer (libm is the reference in there:
    -ffp-contract=off keeps the host compiler from fusing what the reference's build does not)."""
    src = os.path.join(HERE, "helpers", name + ".c")
    so = os.path.join(HERE, "helpers", "lib" + name + ".so")
    newest = max(os.path.getmtime(src), os.path.getmtime(os.path.join(HERE, "..", "gmix_amd", "csrc", "gmx_math.h")))
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", src, "-o", so, "-lm"])
    return C.CDLL(so)


def _edge_inputs():
    """+-0, the subnormal range's ends, FLT_MIN, 0.5, 1 -+ ulp, every threshold that gmx_logf / gmx_logit /
    gmx_expm1f / gmx_tanhf spell as a literal (each -+ 1 ulp, both signs), the layer norm's huge sums, +-inf, NaN."""
    lit = [0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x3f000000, 0x3f800000, 0x7f7fffff, 0x7f800000,
           0x4195b844, 0x42b17218, 0x3eb17218, 0x3f851592, 0x33000000,      # gmx_expm1f's branch points
           0x41b00000, 0x24000000,                                          # gmx_tanhf: 22, 2^-55
           0x3f330000, 0x3f800000 - (1 << 19), 0x3f800000 + (1 << 19),      # gmx_logf: table origin, interval ends
           0x7149f2ca, 0x7e967699, 0x5d5e0b6b, 0x3727c5ac]                  # 1e30, 1e38, 1e18, 1e-5
    lit += [int(np.float32(v).view(np.uint32)) for v in (0.0001, 0.9999, 8.8721679688e+01, 0.25, 0.75, 3.0, 6.0,
                                                         0.6931471806, 1.0397207708, 0.3465735903, 2.0 ** -25)]
    u = np.array(lit, np.int64)
    u = np.concatenate([u - 1, u, u + 1])
    u = u[(u >= 0) & (u <= 0x7fffffff)]
    u = np.concatenate([u, u | 0x80000000, [0x7fc00000, 0xffc00000, 0x7f800001]]).astype(np.uint32)
    return u.view(np.float32)


@pytest.mark.parametrize("fn", list(LSTM_WHAT))
def test_device_lstm_math_equals_libm_samples(gpu, fn):
    """gmx_logf, gmx_logit, gmx_expm1f, gmx_tanhf, the logistic with its table in LDS and the layer-norm scale
    1 / sqrtf(sq / 50 + 1e-5f) as gfx950 computes them, against this machine's libm (and the host compiler's
    correctly rounded divide and sqrtf) on random bit patterns and the edges of every branch: names the inputs."""
    L, H = gpu._lib.lib(), _helper("mathcheck")
    H.gmx_libm_lstm_array.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.integers(0, 1 << 32, 2_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        np.linspace(-30, 30, 200001).astype(np.float32), _edge_inputs()])
    y, ref = np.zeros_like(x), np.zeros_like(x)
    assert L.gmx_debug_math_probe(0, x.ctypes.data, y.ctypes.data, len(x), LSTM_WHAT[fn]) == 0
    H.gmx_libm_lstm_array(x.ctypes.data, ref.ctypes.data, len(x), LSTM_WHAT[fn])
    same = (y.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(y) & np.isnan(ref))
    bad = np.nonzero(~same)[0]
    assert len(bad) == 0, (len(bad), [(hex(x.view(np.uint32)[i]), hex(y.view(np.uint32)[i]), hex(ref.view(np.uint32)[i]))
                                     for i in bad[:5]])


@pytest.mark.parametrize("fn", list(LSTM_WHAT))
def test_device_lstm_math_exhaustive_checksum(gpu, fn):
    """The same six functions over all 2^32 float inputs: the device folds its result bit patterns into
    {xor-fold, sum}, the host folds libm's."""
    L, H = gpu._lib.lib(), _helper("rangecheck")
    H.gmx_host_math_range.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_ulonglong)]
    dev, host = (C.c_ulonglong * 2)(), (C.c_ulonglong * 2)()
    assert L.gmx_debug_math_range(0, 0, 1 << 32, LSTM_WHAT[fn], dev) == 0
    H.gmx_host_math_range(0, 1 << 32, LSTM_WHAT[fn], host)
    assert (dev[0], dev[1]) == (host[0], host[1]), fn


def test_device_adam_step_equals_host_on_operand_tuples(gpu):
    """w - alpha * ((m / d1) / sqrtf(v / d2 + eps)) as the LSTM kernel evaluates it (the probe calls the kernel's own
    gmx_lstm_adam_step) against gcc's IEEE divide and sqrtf: a grid of every step count t = 1 .. 3000 (alpha,
    d1 = 1 - beta1^t, d2 = 1 - beta2^t as the library's host side makes them) x v from 0 through the subnormals to
    1e30 x m x w, then 2^26 hashed tuples over all finite operands.  Counts the differing results; must be 0."""
    L, H = gpu._lib.lib(), _helper("mathcheck")
    H.gmx_adam_grid_size.restype = C.c_uint64
    H.gmx_adam_tuples.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    H.gmx_libm_adam_array.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    total, chunk = H.gmx_adam_grid_size() + (1 << 26), 1 << 22
    assert H.gmx_adam_grid_size() >= 3000 * 100
    x, y, ref = (np.zeros(6 * chunk, np.float32) for _ in range(3))
    mismatches, first = 0, None
    for lo in range(0, total, chunk):
        n = min(chunk, total - lo)
        H.gmx_adam_tuples(lo, n, x.ctypes.data)
        assert L.gmx_debug_math_probe(0, x.ctypes.data, y.ctypes.data, 6 * n, 11) == 0
        H.gmx_libm_adam_array(x.ctypes.data, ref.ctypes.data, n)
        yy, rr = y[:6 * n:6], ref[:6 * n:6]
        bad = np.nonzero((yy.view(np.uint32) != rr.view(np.uint32)) & ~(np.isnan(yy) & np.isnan(rr)))[0]
        mismatches += len(bad)
        if len(bad) and first is None:
            j = int(bad[0])
            first = dict(tuple_index=lo + j, w_alpha_m_d1_v_d2=[hex(v) for v in x[6 * j:6 * j + 6].view(np.uint32)],
                         device=hex(yy.view(np.uint32)[j]), host=hex(rr.view(np.uint32)[j]))
    assert mismatches == 0, (mismatches, first)
