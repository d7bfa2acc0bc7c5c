"""The streaming BLAS-1 exports through the C-ABI, bit for bit, inside guarded buffers: bcnn_hip_axpy, bcnn_hip_scal,
bcnn_hip_copy_f32 (csrc/blas1.hip), bcnn_hip_fill_f32 (csrc/runtime.hip), and the per-channel exports bcnn_hip_add_bias,
_scales, _grad_bias, _grad_scales on tensors that do not start on a 16-byte boundary.

What each case reaches:
  map2_kernel (axpy, scal)   x and y both 16-byte aligned: float4 body, then a scalar tail when n % 4 != 0 (n < 4: tail
                             only); either one misaligned: the scalar branch. One float4 per thread and a grid capped at
                             2048 workgroups of 256: the second sweep starts past 2 097 152 elements.
  scal, a == 0 / a == 1      a memset / nothing at all: +0 over NaN, NaN payloads untouched
  copy_f32                   a device copy of bits; x == y returns at once
  fill_f32_kernel            scalar head up to a 16-byte boundary (more than n when n < head), float4 body, scalar tail;
                             a zero of either sign is a memset (the contract stated in include/bcnn_hip.h)
  per-channel exports        4-byte accesses when the tensor is misaligned: ChanMapBody's scalar loop in the flat and the
                             plane map, SumUnalignedF and DotUnalignedF in the reductions (hw % 4 == 0 keeps the vec4
                             grouping, so the sums are the aligned call's bits)
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _next_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SWEEP = 2048 * 256 * 4                 # elements one sweep of the capped map2 / fill grid covers: 2 097 152
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1027, SWEEP, SWEEP + 7, 2 * SWEEP + 1201]
SUBSET = [3, 7, 1027, SWEEP + 7]
AXPY_CASES = ([((0, 0), n) for n in SIZES] + [((1, 0), n) for n in SIZES] +
              [(s, n) for s in ((0, 1), (1, 1), (2, 2)) for n in SUBSET])
ident = lambda v: "-".join(str(q) for q in v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  (first, so that one HIP runtime serves torch and the library)
    from bcnn_amd import _lib
    return _lib.load()


def f(x):
    return C.c_float(x)


@functools.lru_cache(maxsize=None)
def operands(n):
    """x, y in [-2, 2] (read-only, shared), with exact zeros of both signs and ones scattered over both"""
    rs = np.random.RandomState(n % 100003)
    x, y = rs.uniform(-2, 2, n).astype(F32), rs.uniform(-2, 2, n).astype(F32)
    for a in (x, y):
        pos = rs.randint(0, n, 6)
        a[pos] = np.array([0.0, -0.0, 1.0, -1.0, 0.0, 1.0], F32)[:pos.size]
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def any_bits(n):
    """n random 32-bit words: every class of float, NaNs with payloads and infinities among them"""
    w = np.random.RandomState(n % 100003 + 1).randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    w[::5] = np.uint32(0x7FC00000) | (w[::5] & np.uint32(0x3FFFFF))        # a quiet NaN with a payload, every fifth word
    w[1::11] = np.uint32(0xFF800001) | (w[1::11] & np.uint32(0x3FFFFF))     # negative (signalling) NaNs
    v = w.view(F32)
    v.setflags(write=False)
    return v


# ---- bcnn_hip_axpy --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts,n", AXPY_CASES, ids=ident)
def test_axpy_rounds_the_product_and_the_sum_separately(L, shifts, n):
    x, y = operands(n)
    gx = R.Guarded(x, shifts[0])
    for a in (0.37, -1.0, 0.0, 1.0):
        gy = R.Guarded(y, shifts[1])
        L.bcnn_hip_axpy(n, f(a), gx.ptr, gy.ptr)
        L.bcnn_hip_sync()
        want = (x * F32(a)).astype(F32) + y            # fl(fl(x * a) + y): numpy rounds each operation on its own
        R.assert_bits("axpy n%d a%g shifts %s" % (n, a, shifts), gy.read(), want)
    gx.assert_unchanged("x")


def test_axpy_of_no_elements_touches_nothing(L):
    x, y = operands(7)
    gx, gy = R.Guarded(x), R.Guarded(y)
    L.bcnn_hip_axpy(0, f(0.37), gx.ptr, gy.ptr)
    L.bcnn_hip_sync()
    gx.assert_unchanged("x")
    gy.assert_unchanged("y")


# ---- bcnn_hip_scal --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shift", [0, 1])
def test_scal(L, shift, n):
    x, _ = operands(n)
    gx = R.Guarded(x, shift)
    L.bcnn_hip_scal(n, f(0.37), gx.ptr)
    L.bcnn_hip_sync()
    R.assert_bits("scal 0.37 n%d" % n, gx.read(), x * F32(0.37))
    nan = any_bits(n)
    gx = R.Guarded(nan, shift)
    L.bcnn_hip_scal(n, f(1.0), gx.ptr)
    L.bcnn_hip_sync()
    gx.assert_unchanged("scal by 1 leaves every word, NaN payloads included")
    L.bcnn_hip_scal(n, f(0.0), gx.ptr)
    L.bcnn_hip_sync()
    assert not np.any(R.bits(gx.read())), "scal by 0 stores +0 over NaN and infinity"


# ---- bcnn_hip_copy_f32 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shifts", [(0, 0), (1, 3)], ids=ident)
def test_copy_moves_bits(L, shifts, n):
    x = any_bits(n)
    gx, gy = R.Guarded(x, shifts[0]), R.Guarded(np.full(n, 7.5, F32), shifts[1])
    L.bcnn_hip_copy_f32(n, gx.ptr, gy.ptr)
    L.bcnn_hip_sync()
    R.assert_bits("copy n%d" % n, gy.read(), x)
    gx.assert_unchanged("x")


def test_copy_onto_itself_and_of_nothing(L):
    x = any_bits(1027)
    gx, gy = R.Guarded(x, 1), R.Guarded(np.full(1027, 7.5, F32))
    L.bcnn_hip_copy_f32(1027, gx.ptr, gx.ptr)
    L.bcnn_hip_copy_f32(0, gx.ptr, gy.ptr)
    L.bcnn_hip_sync()
    gx.assert_unchanged("x == y")
    gy.assert_unchanged("n == 0")


# ---- bcnn_hip_fill_f32 ----------------------------------------------------------------------------------------------------------
FILL_SIZES = [1, 2, 3, 4, 5, 7, 1027, SWEEP + 7]


@pytest.mark.parametrize("n", FILL_SIZES)
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_fill(L, shift, n):
    sentinel = np.full(n, R.SENTINEL, np.uint32).view(F32)
    # -0.0f: a zero of either sign takes the memset and stores +0.0f (include/bcnn_hip.h)
    for value, want in ((1.5, F32(1.5)), (0.0, F32(0)), (-0.0, F32(0))):
        gx = R.Guarded(sentinel, shift)                # every word must be overwritten; read() checks the bands
        L.bcnn_hip_fill_f32(gx.ptr, n, f(value))
        L.bcnn_hip_sync()
        R.assert_bits("fill %r n%d shift %d" % (value, n, shift), gx.read(), np.full(n, want, F32))


def test_fill_of_no_elements_touches_nothing(L):
    gx = R.Guarded(np.full(7, 7.5, F32), 1)
    L.bcnn_hip_fill_f32(gx.ptr, 0, f(1.5))
    L.bcnn_hip_sync()
    gx.assert_unchanged("n == 0")


# ---- the per-channel exports on misaligned tensors --------------------------------------------------------------------------
CHAN_SHAPES = [(3, 5, 37),
               (4, 8, 48),      # flat map, hw % 4 == 0: float4 groups when aligned
               (2, 4, 1024),    # plane map
               (2, 3, 4100),    # plane map with a tail
               (23, 3, 196)]    # two reduction splits
SUM_TOL = 1e-5                  # relative to the largest magnitude: the bar test_blas1_exports.py holds the reductions to


@functools.lru_cache(maxsize=None)
def chan_case(n, c, hw):
    from tests.test_blas1_exports import _case
    x, g, v, acc0 = _case(n, c, hw, 3)                 # v[0] == 1.0 and v[2] == 0.0: the quirks of both maps
    xs, gs = x.astype(F64), g.astype(F64)
    want = {"grad_bias": acc0 + gs.sum(axis=(0, 2)), "grad_scales": acc0 + (gs * xs).sum(axis=(0, 2))}   # float64
    sc = (x * v[None, :, None]).astype(F32)            # one float32 product; a scale of 0 gives +0, of 1 leaves the value
    sc[:, v == 0, :] = 0
    sc[:, v == 1, :] = x[:, v == 1, :]
    want["scales"] = sc
    ab = (x + v[None, :, None]).astype(F32)            # one float32 sum; a bias of exactly 0 or 1 adds nothing
    skip = (v == 0) | (v == 1)
    ab[:, skip, :] = x[:, skip, :]
    want["add_bias"] = ab
    return x, g, v, acc0, want


def rel(got, want):
    return float(np.abs(np.asarray(got, F64) - want).max() / max(float(np.abs(want).max()), 1e-30))


@pytest.mark.parametrize("n,c,hw", CHAN_SHAPES)
def test_per_channel_maps_on_misaligned_tensors(L, n, c, hw):
    x, _, v, _, want = chan_case(n, c, hw)
    gv = R.Guarded(v)
    for name, fn in (("add_bias", L.bcnn_hip_add_bias), ("scales", L.bcnn_hip_scales)):
        for s in (0, 1, 2, 3):
            gy = R.Guarded(x, s)
            fn(gy.ptr, gv.ptr, n, c, hw)
            L.bcnn_hip_sync()
            R.assert_bits("%s shift %d" % (name, s), gy.read(), want[name])
    gv.assert_unchanged("the per-channel vector")


@pytest.mark.parametrize("n,c,hw", CHAN_SHAPES)
def test_per_channel_sums_on_misaligned_tensors(L, n, c, hw):
    x, g, _, acc0, want = chan_case(n, c, hw)

    def grad_bias(sg):
        gg, ga = R.Guarded(g, sg), R.Guarded(acc0)
        L.bcnn_hip_grad_bias(ga.ptr, gg.ptr, n, c, hw)
        L.bcnn_hip_sync()
        gg.assert_unchanged("g")
        return ga.read()

    def grad_scales(sx, sg):
        gx, gg, ga = R.Guarded(x, sx), R.Guarded(g, sg), R.Guarded(acc0)
        L.bcnn_hip_grad_scales(gx.ptr, gg.ptr, n, c, hw, ga.ptr)
        L.bcnn_hip_sync()
        gx.assert_unchanged("x_norm")
        gg.assert_unchanged("g")
        return ga.read()

    aligned_b, aligned_s = grad_bias(0), grad_scales(0, 0)
    assert rel(aligned_b, want["grad_bias"]) <= SUM_TOL
    assert rel(aligned_s, want["grad_scales"]) <= SUM_TOL
    for s in (1, 2, 3):
        got = grad_bias(s)
        assert rel(got, want["grad_bias"]) <= SUM_TOL, s
        R.assert_bits("grad_bias shift %d against the aligned call" % s, got, aligned_b)
        for sx, sg in ((s, 0), (0, s), (s, s)):
            got = grad_scales(sx, sg)
            assert rel(got, want["grad_scales"]) <= SUM_TOL, (sx, sg)
            R.assert_bits("grad_scales shifts (%d, %d) against the aligned call" % (sx, sg), got, aligned_s)
