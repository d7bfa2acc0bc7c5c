"""What the fused depthwise entry points (bcnn_hip_depthwise_forward_stats / _forward_bnin / _backward_bn / _backward_bnin /
_backward_bn_bnin / _backward_bnin_sums) have to compute, composed from the restatements the project already pins; nothing here
is taken from the kernels. TEST INFRASTRUCTURE ONLY.

  input path   xin = act_in(affine(normalize(raw, mean, var), scale, bias)): tests/_bn_ref.py normalize32 / affine32 (eps 1e-6,
               bcnn_scal and bcnn_add_scalar quirks: bcnn_batchnorm_layer.c:196-242) and tests/_next_ref.py act_forward32 --
               the values the producer's apply sweep would have written. input64: the same in float64.
  forward      y = orc_dw(x = xin32)["y"], the C oracle's depthwise forward (bcnn_depthwise_conv_layer.c:165-293); the statistics
               a following batch-norm starts from are the per-channel sums of y and y * y, in float64.
  gradient     entering the depthwise backward: dy itself, or, with a batch-norm node behind the layer,
               bwd_apply32(dz, y, mean, var, scales, dmean, dvar, M) (eps 1e-5, M = N OH OW: bcnn_batchnorm_layer.c:292-296).
  backward     orc_dw on xin32 and that gradient (bcnn_depthwise_conv_layer.c:295-547): g = gradient * act'(y) (what a call
               without batch-norm writes back over dy), dx (+)= w * g -- the gradient with respect to xin --, dw += sum xin * g,
               db += sum g. grads64: the same sums in float64 with the sum of the terms' magnitudes, for forward-error bounds.
  producer     the sums its batch-norm backward starts with (bcnn_batchnorm_layer.c:263-281): S1 = sum g', S2 = sum g' (raw -
               mean), g' = dx * act_in'(xin) over the complete dx, in float64.
tests/test_dw_fused_ref_pinning.py holds the pieces to each other and to the oracle on the CPU."""
import numpy as np

from oracle import orc_bind as ob
from tests import _bn_ref as B
from tests import _next_ref as R

F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # unit roundoff of float32


# (n, c, h, w, stride), the family whose kernels take it ("dwm": depthwise_march.hip, "dwl": depthwise_lds.hip): the shapes of
# tests/test_depthwise_fused_bn.py, whose docstring derives the geometry
SHAPES = [
    ((2, 5, 9, 12, 1), "dwm"), ((2, 5, 9, 12, 2), "dwm"), ((2, 3, 17, 10, 1), "dwm"), ((2, 3, 17, 10, 2), "dwm"),
    ((3, 5, 15, 7, 1), "dwm"), ((1, 2, 57, 8, 1), "dwm"), ((1, 2, 8, 256, 1), "dwm"), ((2, 3, 1, 1, 1), "dwm"),
    ((2, 11, 9, 13, 2), "dwl"), ((1, 2, 3, 130, 2), "dwl"), ((1, 2, 20, 67, 1), "dwl"), ((1, 3, 33, 35, 2), "dwl"),
    ((1, 2, 65, 67, 1), "dwl"), ((1, 2, 65, 67, 2), "dwl"), ((1, 2, 4, 260, 1), "dwl"), ((2, 3, 2, 3, 2), "dwl"),
]


class Case:
    """the tensors and per-channel vectors of one layer (float32, C-contiguous)"""


def out_hw(h, w, s):
    return (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1


def quirk_vector(rs, c, lo, hi, zero_at, one_at):
    """uniform values with an exact 0.0 and an exact 1.0 where the reference's bcnn_scal / bcnn_add_scalar select on them"""
    v = rs.uniform(lo, hi, c).astype(F32)
    for idx, val in ((zero_at, 0.0), (one_at, 1.0)):
        if idx is not None and idx < c:
            v[idx] = val
    return v


def make_case(n, c, h, w, s, act, in_act, seed=0, quirks=True):
    """A 3x3 / pad 1 depthwise layer behind a batch-normalised producer and in front of a batch-norm node. With `quirks` the
    vectors hold the exact values the reference's bcnn_scal / bcnn_add_scalar / bcnn_add_bias select on, placed so that the
    scale-0 channel (whose normalised input is a constant) keeps a random producer bias and a random depthwise bias:
      producer scale      0.0 in channel 0, 1.0 in channel 1
      producer bias       0.0 in channel 2 and 1.0 in channel 3 (c == 3: 0.0 in channel 2, 1.0 in channel 1; c == 2: 1.0 in channel 1)
      depthwise bias      0.0 / 1.0 in the last two channels (c == 3: channels 1 / 2; c == 2: 1.0 in channel 1)
      batch-norm behind   scale 1.0 in channel 0, 0.0 in the last one
    With c < 5 the quirks crowd the channels (c == 2: channel 1 is an identity affine): those shapes run a second time without
    `quirks`, every vector random, so that the ordinary multiply and add on load run on them too."""
    rs = np.random.RandomState(4000 + seed)
    q = (lambda *at: at) if quirks else (lambda *at: (None, None))
    p = Case()
    p.n, p.c, p.h, p.w, p.s, p.act, p.in_act = n, c, h, w, s, act, in_act
    p.oh, p.ow = out_hw(h, w, s)
    p.M = n * p.oh * p.ow
    p.in_mean = rs.uniform(-0.5, 0.5, c).astype(F32)
    p.in_var = rs.uniform(0.3, 1.5, c).astype(F32)
    p.raw = (rs.uniform(-1.5, 1.5, (n, c, h, w)) + p.in_mean.reshape(1, c, 1, 1)).astype(F32)
    p.in_scale = quirk_vector(rs, c, 0.5, 1.5, *q(0, 1))
    p.in_scale[2:] *= np.where(np.arange(c)[2:] % 2, -1, 1).astype(F32)
    p.in_bias = quirk_vector(rs, c, -0.4, 0.4, *q(2 if c >= 3 else None, 3 if c >= 4 else 1))
    p.wt = rs.uniform(-0.5, 0.5, c * 9).astype(F32)
    p.bias = quirk_vector(rs, c, -0.2, 0.2, *q(c - 2 if c >= 3 else None, c - 1 if c >= 2 else None))
    p.bn_mean = rs.uniform(-0.3, 0.3, c).astype(F32)
    p.bn_var = rs.uniform(0.3, 1.5, c).astype(F32)
    p.bn_scale = quirk_vector(rs, c, 0.5, 1.5, *q(c - 1 if c > 1 else None, 0))
    p.bn_dmean = rs.uniform(-0.5, 0.5, c).astype(F32)
    p.bn_dvar = rs.uniform(-0.5, 0.5, c).astype(F32)
    p.dz = rs.uniform(-1, 1, (n, c, p.oh, p.ow)).astype(F32)
    p.dx0 = rs.uniform(-1, 1, (n, c, h, w)).astype(F32)
    p.dw0 = rs.uniform(-1, 1, c * 9).astype(F32)
    p.db0 = rs.uniform(-1, 1, c).astype(F32)
    return p


# ---- the input path -----------------------------------------------------------------------------------------------------------
def input32(raw, mean, var, scale, bias, in_act):
    n, c, h, w = raw.shape
    xn = B.normalize32(raw.reshape(n, c, h * w), mean, var)
    return np.ascontiguousarray(R.act_forward32(B.affine32(xn, scale, bias), in_act).reshape(n, c, h, w))


def _act64(v, act):
    if act == R.ACT_RELU:
        return v * (v > 0)
    if act == R.ACT_LRELU:
        return np.where(v > 0, v, F64(F32(0.1)) * v)
    if act == R.ACT_ABS:
        return np.abs(v)
    if act == R.ACT_CLAMP:
        return np.clip(v, 0.0, 1.0)
    assert act == R.ACT_NONE, act
    return v


def input64(raw, mean, var, scale, bias, in_act):
    """float64 throughout on the float32 inputs; the quirks are O(1) effects (scale 0: memset; bias 1: not added) and stay"""
    n, c, h, w = raw.shape
    ch = lambda v: np.asarray(v, F32).astype(F64).reshape(1, c, 1, 1)
    xn = (raw.astype(F64) - ch(mean)) / np.sqrt(ch(var) + F64(B.EPS_FWD))
    v = np.where(ch(scale) == 0, 0.0, xn * ch(scale))
    v = np.where((ch(bias) != 0) & (ch(bias) != 1), v + ch(bias), v)
    return _act64(v, in_act)


def case_input32(p):
    return input32(p.raw, p.in_mean, p.in_var, p.in_scale, p.in_bias, p.in_act)


# ---- the layer, through the oracle ----------------------------------------------------------------------------------------------
def _orc(p, x, grad, dx0):
    return ob.orc_dw(dict(n=p.n, c=p.c, h=p.h, w=p.w, k=3, s=p.s, p=1, act=p.act, input_grad=1, x=np.ascontiguousarray(x, F32),
                          wt=p.wt, bias=p.bias, dy=np.ascontiguousarray(grad, F32), dx0=np.ascontiguousarray(dx0, F32),
                          dw0=p.dw0, db0=p.db0))


def forward(p, x):
    """(y, [C][2] float64 sums of y and y * y, [C][2] sums of their magnitudes)"""
    y = _orc(p, x, np.zeros((p.n, p.c, p.oh, p.ow), F32), p.dx0)["y"]
    y64 = y.astype(F64)
    st = np.stack([y64.sum(axis=(0, 2, 3)), (y64 * y64).sum(axis=(0, 2, 3))], axis=1)
    mag = np.stack([np.abs(y64).sum(axis=(0, 2, 3)), (y64 * y64).sum(axis=(0, 2, 3))], axis=1)
    return y, st, mag


def gradient_in(p, y, bn):
    """what enters the depthwise backward: dz through the following batch-norm's apply (`bn`), or dz taken as dy"""
    if not bn:
        return p.dz
    hw = p.oh * p.ow
    g = B.bwd_apply32(p.dz.reshape(p.n, p.c, hw), y.reshape(p.n, p.c, hw), p.bn_mean, p.bn_var, p.bn_scale, p.bn_dmean,
                      p.bn_dvar, p.M)
    return np.ascontiguousarray(g.reshape(p.dz.shape))


def backward(p, x, bn, overwrite):
    """dict g (= dy * act'(y) of the gradient that came in), dx, dw, db in the oracle's float32 order, and y"""
    y = forward(p, x)[0]
    o = _orc(p, x, gradient_in(p, y, bn), np.zeros_like(p.dx0) if overwrite else p.dx0)
    assert np.array_equal(o["y"], y)
    return dict(y=y, g=o["dy_out"], dx=o["dx"], dw=o["dw"], db=o["db"])


# ---- the same sums in float64 --------------------------------------------------------------------------------------------------
def _taps(x, oh, ow, s):
    """x zero-padded by one; yields (kh, kw, the (n, c, oh, ow) window of inputs that tap meets)"""
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    for kh in range(3):
        for kw in range(3):
            yield kh, kw, xp[:, :, kh:kh + (oh - 1) * s + 1:s, kw:kw + (ow - 1) * s + 1:s]


def dwconv64(x, wt, bias, s):
    """pre-activation output of the layer in float64 (bias with the bcnn_add_bias quirk)"""
    n, c, h, w = x.shape
    oh, ow = out_hw(h, w, s)
    w9 = np.asarray(wt, F32).astype(F64).reshape(c, 3, 3)
    acc = np.zeros((n, c, oh, ow), F64)
    for kh, kw, win in _taps(np.asarray(x).astype(F64), oh, ow, s):
        acc += w9[:, kh, kw].reshape(1, c, 1, 1) * win
    b = np.asarray(bias, F32).astype(F64).reshape(1, c, 1, 1)
    return np.where((b != 0) & (b != 1), acc + b, acc)


def grads64(x, g, wt, s, dx0, dw0, db0):
    """float64 dx, dw, db from float32-valued x and g, and dw_mag / db_mag: the sums of the magnitudes of every term of dw / db
    (the carry-in included) that a forward-error bound of a float32 summation in any order is a multiple of"""
    n, c, h, w = x.shape
    oh, ow = g.shape[2:]
    x64, g64 = np.asarray(x).astype(F64), np.asarray(g).astype(F64)
    w9 = np.asarray(wt, F32).astype(F64).reshape(c, 3, 3)
    dw, mag = np.asarray(dw0, F32).astype(F64).reshape(c, 3, 3).copy(), np.abs(np.asarray(dw0, F32).astype(F64)).reshape(c, 3, 3)
    dxp = np.zeros((n, c, h + 2, w + 2), F64)
    for kh, kw, win in _taps(x64, oh, ow, s):
        dw[:, kh, kw] += (win * g64).sum(axis=(0, 2, 3))
        mag[:, kh, kw] += np.abs(win * g64).sum(axis=(0, 2, 3))
        dxp[:, :, kh:kh + (oh - 1) * s + 1:s, kw:kw + (ow - 1) * s + 1:s] += w9[:, kh, kw].reshape(1, c, 1, 1) * g64
    d0 = np.asarray(db0, F32).astype(F64)
    return dict(dx=np.asarray(dx0, F32).astype(F64) + dxp[:, :, 1:-1, 1:-1], dw=dw.reshape(-1), dw_mag=mag.reshape(-1),
                db=d0 + g64.sum(axis=(0, 2, 3)), db_mag=np.abs(d0) + np.abs(g64).sum(axis=(0, 2, 3)))


def in_sums64(dx, xin, raw, mean, in_act):
    """([C][2] S1, S2 of the producer's batch-norm backward over the complete dx, [C][2] sums of the terms' magnitudes)"""
    c = raw.shape[1]
    gp = np.asarray(dx, F32).astype(F64) * R.act_factor64(xin, in_act)
    d = raw.astype(F64) - np.asarray(mean, F32).astype(F64).reshape(1, c, 1, 1)
    ax = (0, 2, 3)
    return (np.stack([gp.sum(axis=ax), (gp * d).sum(axis=ax)], axis=1),
            np.stack([np.abs(gp).sum(axis=ax), np.abs(gp * d).sum(axis=ax)], axis=1))


def sum_bound(k, mag):
    """forward-error bound of a float32 sum of k terms in any order and grouping, each term itself one or two roundings away
    from its exact value, then one conversion and one add of the result: (k + 2) u sum |terms| (the form of _next_ref.gemm64)"""
    return (k + 2) * U * np.asarray(mag, F64)
