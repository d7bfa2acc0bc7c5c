"""Kernel-level tests of csrc/next.hip through the C-ABI: bcnn_hip_eltwise_forward / _backward, bcnn_hip_axpy_strided,
bcnn_hip_add_rowvec and bcnn_hip_softmax_forward against the numpy restatements of tests/_next_ref.py (pinned to the
reference by test_next_ref_pinning.py).

Every device tensor is a view between two bands of sentinel words (_next_ref.Guarded); reading a result back asserts that
the bands are bit-unchanged. Which branch each case reaches, from the dispatch conditions in next.hip:
  eltwise_fwd_kernel / eltwise_bwd_kernel (cheap activation, all pointers 16-byte aligned)
      n < 4                      scalar tail only
      n % 4 == 0                 float4 body only
      otherwise                  float4 body + scalar tail
      b_count % 4 != 0           the float4 group that b_count ends in takes the per-component branch
      n > 2048 * 256 * 4         second sweep of the grid-stride loop (the grid is capped at 2048 blocks)
  three-pass fallback            TANH / LOGISTIC / SOFTPLUS forward, SOFTPLUS backward, or any misaligned pointer
  axpy_strided_kernel, add_rowvec_kernel: second sweep past 2048 * 256 elements
  softmax_kernel: one wave per row; C > 64 gives a lane more than one channel, n * HW > 8192 enters the wave-stride loop
"""
import ctypes as C

import numpy as np
import pytest

from tests import _next_ref as R
from tests.test_hip_parity import ACT_TOL

pytestmark = pytest.mark.gpu

F32 = np.float32
SWEEP = 2048 * 256 * 4                     # elements one sweep of the capped eltwise grid covers
BIG = SWEEP + 4096 + 3                     # second sweep, ending in a scalar tail
SIZES = [1, 3, 4, 5, 1023, 1024, 1027]
FUSED = [R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU, R.ACT_RAMP, R.ACT_ABS, R.ACT_CLAMP]
ACTS = FUSED + [R.ACT_TANH, R.ACT_LOGISTIC, R.ACT_SOFTPLUS]    # PReLU left out: the node has no slopes
act_id = lambda a: R.ACT_NAMES[a]


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  (first, so that one HIP runtime serves torch and the library)
    from bcnn_amd import _lib
    return _lib.load()


def b_counts(n):
    """n, an aligned fraction, b_count % 4 in {1, 2, 3} and b_count < 4 (b_count >= 1: the node never passes 0)"""
    half = (n // 2) // 4 * 4
    return sorted({c for c in (n, half, half + 1, half + 2, half + 3, 1, 2, 3) if 1 <= c <= n})


def operands(n, b_count, act, seed):
    """a, b with a + b in [-2, 2] and, scattered over the tensor, sums that are exactly 0 and 1, one ulp either side of 1,
    just either side of 0, and exact zeros in both operands"""
    rs = np.random.RandomState(seed)
    a = rs.uniform(-1, 1, n).astype(F32)
    b = rs.uniform(-1, 1, b_count).astype(F32)
    one = F32(1)
    special = [F32(0), one, np.nextafter(one, F32(2)), np.nextafter(one, F32(0)), F32(1e-6), F32(-1e-6), F32(-0.5),
               F32(-1.5), F32(2)]
    if R.FWD_BAR[act] != R.ACT:            # the double-precision activations lose 1e-30 next to 1 by design
        special += [F32(1e-30), F32(-1e-30)]
    pos = rs.permutation(n)[:len(special)]
    for p, s in zip(pos, rs.permutation(len(special))):
        a[p] = special[s]
        if p < b_count:
            b[p] = F32(0)
    if n >= 64:                            # 0.75 + 0.25 and -0.25 + 0.25 under the second operand
        q = rs.permutation(b_count)[:2] if b_count >= 2 else []
        for p, v in zip(q, (F32(0.75), F32(-0.25))):
            a[p], b[p] = v, F32(0.25)
    return a, b


def run_forward(L, a, b, n, b_count, act, shift=(0, 0, 0)):
    ga, gb, gy = R.Guarded(a, shift[0]), R.Guarded(b, shift[1]), R.Guarded(np.full(n, 7.5, F32), shift[2])
    L.bcnn_hip_eltwise_forward(ga.ptr, gb.ptr, gy.ptr, n, b_count, act)
    L.bcnn_hip_sync()
    ga.assert_unchanged("a")
    gb.assert_unchanged("b")
    return gy.read()


def check_forward(L, n, b_count, act, seed, shift=(0, 0, 0)):
    a, b = operands(n, b_count, act, seed)
    got = run_forward(L, a, b, n, b_count, act, shift)
    want32, want64 = R.eltwise_forward(a, b, b_count, act)
    R.assert_bar(R.FWD_BAR[act], "eltwise_fwd/%s/n%d/b%d" % (R.ACT_NAMES[act], n, b_count), got, want32, want64, ACT_TOL)
    return got


@pytest.mark.parametrize("act", ACTS, ids=act_id)
@pytest.mark.parametrize("n", SIZES)
def test_eltwise_forward(L, n, act):
    for b_count in b_counts(n):
        check_forward(L, n, b_count, act, 11 * n + b_count)


@pytest.mark.parametrize("b_count", [BIG, 1000001, SWEEP + 1030], ids=["all", "first_sweep", "second_sweep"])
def test_eltwise_forward_second_sweep(L, b_count):
    check_forward(L, BIG, b_count, R.ACT_RELU, 5)


@pytest.mark.parametrize("act", [R.ACT_RELU, R.ACT_RAMP, R.ACT_LOGISTIC], ids=act_id)
def test_eltwise_forward_misaligned_pointers_take_the_fallback(L, act):
    n, b_count = 1027, 515
    aligned = check_forward(L, n, b_count, act, 3)
    for which in range(3):                 # a, b, y in turn one float off a 16-byte boundary
        shift = tuple(int(i == which) for i in range(3))
        got = check_forward(L, n, b_count, act, 3, shift)
        R.assert_bar(R.FWD_BAR[act] if R.FWD_BAR[act] != R.ACT else R.EXACT, "fwd shift %s" % (shift,), got, aligned,
                     aligned, ACT_TOL)     # LOGISTIC runs the same three passes both times: identical bits


def backward_operands(n, b_count, act, seed):
    a, b = operands(n, b_count, act, seed)
    y = R.act_forward32(R.eltwise_sum32(a, b, b_count), act)     # post-activation values, exact 0 and 1 among them
    rs = np.random.RandomState(seed + 1)
    dy = rs.uniform(-1, 1, n).astype(F32)
    dy[rs.permutation(n)[:max(1, n // 16)]] = F32(0)
    return y, dy, rs.uniform(-1, 1, n).astype(F32), rs.uniform(-1, 1, b_count).astype(F32)


def check_backward(L, n, b_count, act, seed, with_da=True, with_db=True, overwrite=0, shift=(0, 0, 0, 0)):
    y, dy, da, db = backward_operands(n, b_count, act, seed)
    tag = "eltwise_bwd/%s/n%d/b%d/da%d/db%d/ow%d" % (R.ACT_NAMES[act], n, b_count, with_da, with_db, overwrite)
    gy, gdy = R.Guarded(y, shift[0]), R.Guarded(dy, shift[1])
    # overwrite_a: da holds zeros semantically and must not be read -- a NaN there would come out
    gda = R.Guarded(np.full(n, np.nan, F32) if overwrite else da, shift[2]) if with_da else None
    gdb = R.Guarded(db, shift[3]) if with_db else None
    L.bcnn_hip_eltwise_backward(gy.ptr, gdy.ptr, gda.ptr if gda else None, gdb.ptr if gdb else None, n, b_count, act,
                                overwrite)
    L.bcnn_hip_sync()
    gy.assert_unchanged("y")
    g, da_w, db_w, g64 = R.eltwise_backward(y, dy, da if with_da else None, db if with_db else None, b_count, act, overwrite)
    bar = R.BWD_BAR[act]
    out = {"dy": gdy.read()}
    if act == R.ACT_NONE:
        gdy.assert_unchanged("dy under NONE")
    R.assert_bar(bar, tag + "/dy", out["dy"], g, g64, ACT_TOL)
    if bar != R.EXACT:
        # the two accumulations are one float32 add each of the g that was stored: bit-exact given the device's own g
        # (a tolerance on a sum that may cancel would have to be absolute, and would then check less)
        _, da_w, db_w, _ = R.eltwise_backward(y, out["dy"], da if with_da else None, db if with_db else None, b_count,
                                              R.ACT_NONE, overwrite)
    if with_da:
        out["da"] = gda.read()
        assert not np.isnan(out["da"]).any(), tag
        R.assert_bits(tag + "/da", out["da"], da_w)
    if with_db:
        out["db"] = gdb.read()             # exactly b_count elements: the band starts where b_count ends
        R.assert_bits(tag + "/db", out["db"], db_w)
    return out


SWITCHES = [(1, 1), (0, 1), (1, 0)]


@pytest.mark.parametrize("act", ACTS, ids=act_id)
@pytest.mark.parametrize("n", SIZES)
def test_eltwise_backward(L, n, act):
    for b_count in b_counts(n):
        # every switch combination at two sizes with a tail, both overwrite modes with both gradients everywhere
        combos = [(da, db, ow) for da, db in SWITCHES for ow in (0, 1)] if n in (5, 1027) else [(1, 1, 0), (1, 1, 1)]
        for with_da, with_db, ow in combos:
            check_backward(L, n, b_count, act, 7 * n + b_count, bool(with_da), bool(with_db), ow)


@pytest.mark.parametrize("b_count,ow", [(BIG, 0), (1000001, 1), (SWEEP + 1030, 0)],
                         ids=["all", "first_sweep_overwrite", "second_sweep"])
def test_eltwise_backward_second_sweep(L, b_count, ow):
    check_backward(L, BIG, b_count, R.ACT_RELU, 9, True, True, ow)


@pytest.mark.parametrize("act", [R.ACT_RELU, R.ACT_TANH, R.ACT_LOGISTIC], ids=act_id)
def test_eltwise_backward_misaligned_pointers_take_the_fallback(L, act):
    n, b_count = 1027, 515
    for ow in (0, 1):
        aligned = check_backward(L, n, b_count, act, 3, True, True, ow)
        for which in range(4):             # y, dy, da, db in turn
            shift = tuple(int(i == which) for i in range(4))
            got = check_backward(L, n, b_count, act, 3, True, True, ow, shift)
            for key in aligned:
                R.assert_bar(R.BWD_BAR[act], "bwd shift %s %s" % (shift, key), got[key], aligned[key], aligned[key], ACT_TOL)


# ---- bcnn_hip_axpy_strided ------------------------------------------------------------------------------------------------
AXPY_CASES = {  # nb, sy, sx, (xc, xh, xw), (yc, yh, yw)
    "fwd_up2": (1, 2, 1, (3, 4, 4), (3, 8, 8)),                 # eltwise forward, destination twice the source
    "bwd_down2": (1, 1, 2, (3, 8, 8), (3, 4, 4)),               # its backward: strides swapped
    "xc_lt_yc_nb3": (3, 2, 1, (2, 4, 4), (5, 8, 8)),
    "xc_gt_yc_nb3": (3, 2, 1, (5, 4, 4), (2, 8, 8)),
    "nonsquare_fwd": (3, 2, 1, (4, 3, 5), (3, 6, 10)),
    "nonsquare_bwd": (3, 1, 2, (3, 6, 10), (4, 3, 5)),
    "past_a_sweep": (4, 2, 1, (16, 96, 96), (16, 192, 192)),    # 589 824 elements > 2048 * 256
}


def run_axpy_strided(L, name, a):
    nb, sy, sx, xdim, ydim = AXPY_CASES[name]
    mindim = tuple(min(p, q) for p, q in zip(xdim, ydim))
    rs = np.random.RandomState(len(name))
    x = rs.uniform(-1, 1, (nb,) + xdim).astype(F32)
    y = rs.uniform(-1, 1, (nb,) + ydim).astype(F32)
    gx, gy = R.Guarded(x), R.Guarded(y)
    L.bcnn_hip_axpy_strided(nb, C.c_float(a), gx.ptr, gy.ptr, sy, sx, *xdim, *ydim, *mindim)
    L.bcnn_hip_sync()
    gx.assert_unchanged("x")
    want32, want64 = R.axpy_strided(nb, a, x, y, sy, sx, xdim, ydim, mindim)
    touched = np.zeros(y.shape, bool)
    touched[:, :mindim[0], 0:(mindim[1] - 1) * sy + 1:sy, 0:(mindim[2] - 1) * sy + 1:sy] = True
    assert touched.sum() == nb * int(np.prod(mindim))
    return gy.read().reshape(y.shape), y, want32, want64, touched


@pytest.mark.parametrize("a", [1.0, 0.5, -2.0])
@pytest.mark.parametrize("name", list(AXPY_CASES))
def test_axpy_strided_exact_scales_are_bit_exact(L, name, a):
    got, y0, want32, _, touched = run_axpy_strided(L, name, a)
    R.assert_bits("axpy_strided/%s/a%g" % (name, a), got, want32)    # the untouched elements of y included
    assert np.array_equal(R.bits(got)[~touched], R.bits(y0)[~touched])


@pytest.mark.parametrize("name", ["fwd_up2", "nonsquare_bwd"])
def test_axpy_strided_inexact_scale(L, name):
    got, y0, want32, _, touched = run_axpy_strided(L, name, 0.37)
    assert np.array_equal(R.bits(got)[~touched], R.bits(y0)[~touched])
    R.assert_fma("axpy_strided/%s/a0.37" % name, got, want32)


# ---- bcnn_hip_add_rowvec --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 7), (128, 1000), (600, 1000)])
def test_add_rowvec(L, rows, cols):
    rs = np.random.RandomState(rows + cols)
    y = rs.uniform(-1, 1, (rows, cols)).astype(F32)
    v = rs.uniform(-1, 1, cols).astype(F32)
    v[0] = F32(1)                          # plain axpy: no 0 / 1 quirk
    v[cols // 2] = F32(0)
    gy, gv = R.Guarded(y), R.Guarded(v)
    L.bcnn_hip_add_rowvec(gy.ptr, gv.ptr, rows, cols)
    L.bcnn_hip_sync()
    gv.assert_unchanged("v")
    R.assert_bits("add_rowvec/%dx%d" % (rows, cols), gy.read().reshape(rows, cols), R.add_rowvec(y, v))


# ---- bcnn_hip_softmax_forward ---------------------------------------------------------------------------------------------
def run_softmax(L, n, c, hw):
    x = R.softmax_inputs(n, c, hw, 100 * c + hw + n)
    gx, gy = R.Guarded(x), R.Guarded(np.full(x.size, -3.0, F32))
    L.bcnn_hip_softmax_forward(gx.ptr, gy.ptr, n, c, hw)
    L.bcnn_hip_sync()
    gx.assert_unchanged("x")
    R.check_softmax(gy.read(), x, "softmax/n%d_c%d_hw%d" % (n, c, hw))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [1, 5, 49])
@pytest.mark.parametrize("c", [1, 2, 10, 63, 64, 65, 130, 1000])
def test_softmax_forward(L, c, hw, n):
    run_softmax(L, n, c, hw)


def test_softmax_forward_wave_stride_loop(L):
    run_softmax(L, 3, 5, 3000)             # 9000 rows > 2048 blocks x 4 waves
