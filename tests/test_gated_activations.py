"""The five appended activations at the kernel level (bcnn_amd/csrc/common.h, activation.hip), through bcnn_amd.ops.

relu6, hard_sigmoid, hard_swish are float arithmetic the build does not contract: forward and backward are held to the
float32 numpy expression of the same formula, bit for bit (int32 views). The kink rows (-3, 0, 3, 6, +-0.0) pin the `<` / `<=`
choices of torch. A NaN input gives a NaN output; its payload is not compared.
swish and mish are held to torch float64 on the same float32 inputs, per element:
    |got - ref| <= 2 |torch_float32 - ref| + ulp32(ref)
with torch_float32 torch's own CPU silu / mish (forward) and autograd (backward) in float32.
    Measured once, MI355X, the inputs of this file (in ulp32 of the float64 value, worst element): see DESIGN.md section 22.
The saved input of the forward is the input bit for bit, and a null buffer does not change y. relu6 / hard_sigmoid through the
entry points that take an `act` argument (activation, eltwise, a convolution + batch-norm node) equal the separate in-place
pass bit for bit: every consumer took that route."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SIZES = [1, 3, 4, 5, 63, 64, 65, 1027, 4 * 256 * 17 + 2]
SPECIALS = np.array([-3.0, 0.0, 3.0, 6.0, -0.0, 1e-30, -1e-30, 30.0, -30.0, 88.0, -88.0, np.nan, -6.0, 2.999999, 3.0000002],
                    F32)


def _inputs(size, seed=0):
    """linspace(-8, 8) with the special values over its head and, where they fit twice, over its tail (the scalar tail of
    the kernels); sizes below the list take a rotating part of it"""
    x = np.linspace(-8, 8, size).astype(F32)
    k = len(SPECIALS)
    if size >= 2 * k:
        x[:k] = SPECIALS
        x[-k:] = SPECIALS[::-1]
    else:
        for i in range(size):
            x[i] = SPECIALS[(i + size) % k]
    dy = np.random.RandomState(size + seed).uniform(-2, 2, size).astype(F32)
    return x, dy


def _dev(a, offset=0):
    """a device copy of `a`; offset = 1 puts it one float past a 16-byte boundary (the kernels' unaligned-base route)"""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
    return view


def _same_bits(got, want, what):
    got, want = np.asarray(got, F32).ravel(), np.asarray(want, F32).ravel()
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), "%s: NaNs at %s, expected at %s" % (what, np.flatnonzero(nan_g), np.flatnonzero(nan_w))
    bad = np.flatnonzero((got.view(np.int32) != want.view(np.int32)) & ~nan_g)
    assert bad.size == 0, "%s: %d elements differ, first at %d: got %r want %r" % (what, bad.size, bad[0], got[bad[0]],
                                                                                     want[bad[0]])


# ---- the float32 expressions of the issue's table ---------------------------------------------------------------------------
def _clip6(v):
    return np.minimum(np.maximum(v, F32(0)), F32(6))


def _fwd32(x, name):
    with np.errstate(all="ignore"):
        if name == "relu6":
            return (_clip6(x) + F32(0)).astype(F32)      # + 0: +0.0 for every x <= 0
        if name == "hard_sigmoid":
            return (_clip6(x + F32(3)) / F32(6)).astype(F32)
        return ((x * _clip6(x + F32(3))) / F32(6)).astype(F32)


def _bwd32(x, y, dy, name):
    """relu6 / hard_sigmoid from the output y, hard_swish from the input x"""
    with np.errstate(all="ignore"):
        if name == "relu6":
            fac = ((y > 0) & (y < 6)).astype(F32)
        elif name == "hard_sigmoid":
            fac = np.where((y > 0) & (y < 1), F32(1) / F32(6), F32(0)).astype(F32)
        else:
            fac = np.where(x < -3, F32(0), np.where(x <= 3, x / F32(3) + F32(0.5), F32(1))).astype(F32)
        return (dy * fac).astype(F32)


CASES = [(s, 0) for s in SIZES] + [(1027, 1)]


@pytest.mark.parametrize("size,offset", CASES)
@pytest.mark.parametrize("name", ["relu6", "hard_sigmoid"])
def test_output_derivative_activations_bitwise(name, size, offset):
    from bcnn_amd import ops
    x, dy = _inputs(size)
    t = _dev(x, offset)
    ops.activation_forward(t, ops.ACT_ALL[name])
    y = t.cpu().numpy()
    _same_bits(y, _fwd32(x, name), name + " forward")
    g = _dev(dy, offset)
    ops.activation_backward(t, g, ops.ACT_ALL[name])
    _same_bits(g.cpu().numpy(), _bwd32(x, y, dy, name), name + " backward")
    # the keep entry point takes every id: same bits, and the input is kept
    t2, kept = _dev(x, offset), _dev(np.zeros_like(x), offset)
    ops.activation_forward_keep(t2, kept, ops.ACT_ALL[name])
    _same_bits(t2.cpu().numpy(), y, name + " forward_keep")
    assert np.array_equal(kept.cpu().numpy().view(np.int32), x.view(np.int32))


@pytest.mark.parametrize("size,offset", CASES)
def test_hard_swish_bitwise_and_saved_input(size, offset):
    from bcnn_amd import ops
    act = ops.ACT_ALL["hard_swish"]
    x, dy = _inputs(size)
    t, kept = _dev(x, offset), _dev(np.full_like(x, 7.0), offset)
    ops.activation_forward_keep(t, kept, act)
    _same_bits(t.cpu().numpy(), _fwd32(x, "hard_swish"), "hard_swish forward")
    assert np.array_equal(kept.cpu().numpy().view(np.int32), x.view(np.int32)), "the saved input is the input"
    for fwd in (lambda v: ops.activation_forward_keep(v, None, act), lambda v: ops.activation_forward(v, act)):
        t2 = _dev(x, offset)
        fwd(t2)
        assert torch.equal(t2.view(torch.int32), t.view(torch.int32)), "a null buffer changes nothing in y"
    g = _dev(dy, offset)
    ops.activation_backward_from_input(kept, g, act)
    _same_bits(g.cpu().numpy(), _bwd32(x, None, dy, "hard_swish"), "hard_swish backward")


def _torch_pair(fn, x, dy, dtype):
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    y = fn(xt)
    y.backward(torch.tensor(dy, dtype=dtype))
    return y.detach().numpy().astype(np.float64), xt.grad.numpy().astype(np.float64)


def _held_to_float64(got, ref, t32, what):
    """|got - ref| <= 2 |torch32 - ref| + ulp32(ref) per element; NaN where the reference is NaN. Returns the worst error of
    the kernel and of torch float32, both in ulp32(ref)."""
    got = np.asarray(got, np.float64).ravel()
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN must propagate, and only NaN"
    ok = ~nan
    ulp = np.spacing(np.abs(ref[ok]).astype(F32)).astype(np.float64)
    err, terr = np.abs(got[ok] - ref[ok]), np.abs(t32[ok] - ref[ok])
    print("%s: kernel %.3f ulp, torch float32 %.3f ulp (worst element each)" % (what, (err / ulp).max(), (terr / ulp).max()))
    bad = np.flatnonzero(err > 2 * terr + ulp)
    assert bad.size == 0, "%s: %d elements outside the bar, first %d: err %.3g, torch %.3g, ulp %.3g" % (
        what, bad.size, bad[0], err[bad[0]], terr[bad[0]], ulp[bad[0]])
    return (err / ulp).max(), (terr / ulp).max()


@pytest.mark.parametrize("size,offset", CASES)
@pytest.mark.parametrize("name", ["swish", "mish"])
def test_swish_mish_against_float64(name, size, offset):
    from bcnn_amd import ops
    act = ops.ACT_ALL[name]
    fn = F.silu if name == "swish" else F.mish
    x, dy = _inputs(size)
    y64, dx64 = _torch_pair(fn, x, dy, torch.float64)
    y32, dx32 = _torch_pair(fn, x, dy, torch.float32)
    t, kept = _dev(x, offset), _dev(np.full_like(x, 7.0), offset)
    ops.activation_forward_keep(t, kept, act)
    _held_to_float64(t.cpu().numpy(), y64, y32, name + " forward")
    assert np.array_equal(kept.cpu().numpy().view(np.int32), x.view(np.int32)), "the saved input is the input"
    for fwd in (lambda v: ops.activation_forward_keep(v, None, act), lambda v: ops.activation_forward(v, act)):
        t2 = _dev(x, offset)
        fwd(t2)
        assert torch.equal(t2.view(torch.int32), t.view(torch.int32)), "a null buffer changes nothing in y"
    g = _dev(dy, offset)
    ops.activation_backward_from_input(kept, g, act)
    _held_to_float64(g.cpu().numpy(), dx64, dx32, name + " backward")


# ---- relu6 / hard_sigmoid through the entry points that take an activation ---------------------------------------------------
@pytest.mark.parametrize("size", [5, 64, 1027, 4 * 256 * 17 + 2])
def test_eltwise_with_relu6_is_add_then_the_separate_pass(size):
    from bcnn_amd import _lib, ops
    L = _lib.load()
    act = ops.ACT_ALL["relu6"]
    a, dy = _inputs(size)
    b = np.random.RandomState(size).uniform(-4, 4, size).astype(F32)
    ta, tb, ty = _dev(a), _dev(b), _dev(np.zeros_like(a))
    L.bcnn_hip_eltwise_forward(ta.data_ptr(), tb.data_ptr(), ty.data_ptr(), size, size, act)
    y = ty.cpu().numpy()
    with np.errstate(all="ignore"):
        s = (a + b).astype(F32)
    _same_bits(y, _fwd32(s, "relu6"), "eltwise forward")
    da0 = np.random.RandomState(size + 1).uniform(-1, 1, size).astype(F32)
    db0 = np.random.RandomState(size + 2).uniform(-1, 1, size).astype(F32)
    tdy, tda, tdb = _dev(dy), _dev(da0), _dev(db0)
    L.bcnn_hip_eltwise_backward(ty.data_ptr(), tdy.data_ptr(), tda.data_ptr(), tdb.data_ptr(), size, size, act, 0)
    g = _bwd32(None, y, dy, "relu6")
    _same_bits(tdy.cpu().numpy(), g, "eltwise dy")
    _same_bits(tda.cpu().numpy(), da0 + g, "eltwise da")
    _same_bits(tdb.cpu().numpy(), db0 + g, "eltwise db")


@pytest.mark.parametrize("name", ["relu6", "hard_sigmoid"])
@pytest.mark.parametrize("bn", [0, 1])
def test_conv_node_equals_act_none_plus_the_separate_pass(name, bn):
    """one convolution (+ batch-norm) node with the activation against the same node with NONE and the stand-alone pass around
    it: y, dx, dw, db and the batch-norm gradients, bit for bit"""
    from bcnn_amd import ops
    from tests import _hip_cases as HC
    act = ops.ACT_ALL[name]
    rs = np.random.RandomState(3)
    n, c, h, w, f, k = 2, 5, 9, 7, 6, 3
    case = dict(op="conv", n=n, c=c, h=h, w=w, f=f, k=k, s=1, p=1, g=1, bn=bn, act=act, input_grad=1, mode=1,
                x=rs.uniform(-1, 1, (n, c, h, w)).astype(F32), wt=rs.uniform(-2, 2, (f, c, k, k)).astype(F32),
                bias=rs.uniform(-0.5, 3.5, (f,)).astype(F32), dy=rs.uniform(-1, 1, (n, f, h, w)).astype(F32),
                run_mean0=np.zeros(f, F32), run_var0=np.ones(f, F32), scales=rs.uniform(1.5, 3, f).astype(F32))
    fused = HC.run_hip(case)
    # the same node with NONE; the activation around it by hand
    plain = dict(case, act=0, forward_only=1)
    y_pre = HC.run_hip(plain)["y"]
    ty = HC.D(y_pre)
    ops.activation_forward(ty, act)
    y = HC.H(ty)
    assert (y > 0).any() and (y == 0).any() and (y == (6 if name == "relu6" else 1)).any(), "both kinks are exercised"
    _same_bits(fused["y"], y, "y")
    tdy = HC.D(case["dy"])
    ops.activation_backward(ty, tdy, act)
    # backward of the NONE node on the hand-made gradient: the forward first (it fills the batch-norm state), then backward
    manual = HC.run_hip(dict(case, act=0, dy=HC.H(tdy)))
    for key in ("dx", "dw", "db") + (("dscales", "dmean", "dvar") if bn else ()):
        _same_bits(fused[key], manual[key], key)
