"""Pins the reference of the fused depthwise entry points (tests/_dw_fused_ref.py) on the CPU, on the shapes the GPU test
(tests/test_depthwise_fused_bn.py) runs:
  * its float32 composition (the pieces of _bn_ref.py / _next_ref.py and the C oracle's depthwise layer) and its float64 form
    agree to rounding -- every bar below is a count of float32 roundings times the magnitudes that enter the result;
  * with mean 0, var + eps == 1, scale 1, bias 0 and no activation the input path is the identity, so the composition is
    orc_dw on `raw`;
  * the backward behind a batch-norm node is orc_dw fed with _bn_ref's own apply, which agrees with its float64 apply;
  * the producer's sums S1 / S2 are the db / dscales of _bn_ref.backward64 run on the producer with g' = dx * act_in'(xin).
Shapes with fewer than five channels, where the quirk values crowd the channels, run once more with every vector random.
This is what makes _dw_fused_ref.py a statement of the reference and not of the HIP kernels."""
import numpy as np
import pytest

from oracle import orc_bind as ob
from tests import _bn_ref as B
from tests import _dw_fused_ref as D
from tests import _next_ref as R

F32, F64 = np.float32, np.float64
U = D.U
PAIRS = [(R.ACT_RELU, R.ACT_RELU), (R.ACT_LRELU, R.ACT_NONE), (R.ACT_NONE, R.ACT_LRELU), (R.ACT_CLAMP, R.ACT_RELU),
         (R.ACT_ABS, R.ACT_LRELU)]
# (shape, pair, quirk channels): shapes with fewer than five channels also without the quirks, every vector random
CASES = [(sh, PAIRS[i % len(PAIRS)], True) for i, (sh, _) in enumerate(D.SHAPES)]
CASES += [(sh, PAIRS[(i + 1) % len(PAIRS)], False) for i, (sh, _) in enumerate(D.SHAPES) if sh[1] < 5]
IDS = ["n%d_c%d_%dx%d_s%d_%s_%s%s" % (sh + (R.ACT_NAMES[a], R.ACT_NAMES[b], "" if q else "_random")) for sh, (a, b), q in CASES]


def _within(tag, got, want, bound):
    ratio = np.abs(np.asarray(got, F64) - want) / np.maximum(bound, 1e-300)
    assert ratio.max() <= 1.0, "%s: %.3g x its bound at %s" % (tag, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


@pytest.mark.parametrize("shape,pair,quirks", CASES, ids=IDS)
def test_float32_composition_and_float64_form_agree_to_rounding(shape, pair, quirks):
    p = D.make_case(*shape, act=pair[0], in_act=pair[1], seed=sum(shape), quirks=quirks)
    for v in (p.in_scale, p.in_bias, p.bias, p.bn_scale):
        assert bool(np.isin(v, (0.0, 1.0)).any()) == (quirks and p.c > 1), v
    if quirks and p.c > 1:   # the scale-0 channel keeps a random bias and a random depthwise bias
        assert p.in_scale[0] == 0 and p.in_bias[0] not in (0.0, 1.0) and p.bias[0] not in (0.0, 1.0)
    c = p.c
    ch = lambda v: np.asarray(v, F32).astype(F64).reshape(1, c, 1, 1)
    # input path: subtract, sqrt, divide, multiply, add, activation multiply -- each one rounding of a value no larger than
    # |xn scale| + |bias| + its own result: 8 u of that magnitude covers the chain
    x32 = D.case_input32(p)
    x64 = D.input64(p.raw, p.in_mean, p.in_var, p.in_scale, p.in_bias, p.in_act)
    xn = np.abs(p.raw.astype(F64) - ch(p.in_mean)) / np.sqrt(ch(p.in_var) + F64(B.EPS_FWD))
    _within("xin", x32, x64, 8 * U * (xn * np.abs(ch(p.in_scale)) + np.abs(ch(p.in_bias)) + U))
    # forward: nine products and nine adds, the bias add, the activation's multiply, on the float32 input
    y, st, _ = D.forward(p, x32)
    pre = D.dwconv64(x32, p.wt, p.bias, p.s)
    mag = D.dwconv64(np.abs(x32), np.abs(p.wt), np.abs(p.bias), p.s)
    _within("y", y, D._act64(pre, p.act), (9 + 3) * U * (mag + U))
    assert np.array_equal(st[:, 0], y.astype(F64).sum(axis=(0, 2, 3)))
    # backward, both gradients that can enter it
    for bn in (False, True):
        for overwrite in (False, True):
            o = D.backward(p, x32, bn, overwrite)
            gin = D.gradient_in(p, y, bn)
            g64 = gin.astype(F64) * R.act_factor64(y, p.act)
            _within("g", o["g"], g64, 2 * U * np.abs(g64) + 1e-45)
            dx0 = np.zeros_like(p.dx0) if overwrite else p.dx0
            w64 = D.grads64(x32, o["g"], p.wt, p.s, dx0, p.dw0, p.db0)
            dxm = D.grads64(x32, np.abs(o["g"]), np.abs(p.wt), p.s, np.abs(dx0), p.dw0, p.db0)["dx"]
            _within("dx", o["dx"], w64["dx"], (9 + 2) * U * (dxm + U))
            _within("dw", o["dw"], w64["dw"], D.sum_bound(p.M, w64["dw_mag"]))
            _within("db", o["db"], w64["db"], D.sum_bound(p.M, w64["db_mag"]))
    # the producer's sums against _bn_ref's own statement of a batch-norm backward (bcnn_batchnorm_layer.c:263-281) run on the
    # producer: its incoming gradient is g' = dx * act_in'(xin), its input is raw; db is S1 and dscales is S2 / sqrt(var + 1e-6).
    # backward64 takes a float32 gradient: g' is one (exact for a derivative of 0 or 1; one rounding of 2^-24 for the leaky
    # producer, whose sums no kernel emits); the rest is float64 summation noise, 1e-12 of the magnitudes
    s, m = D.in_sums64(o["dx"], x32, p.raw, p.in_mean, p.in_act)
    gp = (o["dx"] * R.act_factor32(x32, p.in_act)).astype(F32)
    hw, z = p.h * p.w, np.zeros(c, F32)
    b = B.backward64(gp.reshape(p.n, c, hw), p.raw.reshape(p.n, c, hw), np.ones(c, F32), p.in_mean, p.in_var, z, z)
    s2 = b["dscales"] * np.sqrt(p.in_var.astype(F64) + F64(B.EPS_FWD))
    tol = (1e-12 if p.in_act in (R.ACT_NONE, R.ACT_RELU) else 2 * U) * m + 1e-300
    assert (np.abs(s[:, 0] - b["db"]) <= tol[:, 0]).all() and (np.abs(s[:, 1] - s2) <= tol[:, 1]).all()
    assert (m >= np.abs(s)).all() and (m[:, 1] > 0).any()


@pytest.mark.parametrize("shape", [sh for sh, _ in D.SHAPES], ids=lambda s: "n%d_c%d_%dx%d_s%d" % s)
def test_identity_input_path_reduces_to_the_oracle_on_raw(shape):
    p = D.make_case(*shape, act=R.ACT_LRELU, in_act=R.ACT_NONE, seed=1)
    c = p.c
    p.in_mean, p.in_scale, p.in_bias = np.zeros(c, F32), np.ones(c, F32), np.zeros(c, F32)
    p.in_var = np.full(c, F32(1) - F32(1e-6), F32)
    assert np.all(p.in_var + B.EPS_FWD == F32(1)) and np.all(p.in_var < 1)
    x = D.case_input32(p)
    assert np.array_equal(x, p.raw)
    want = ob.orc_dw(dict(n=p.n, c=c, h=p.h, w=p.w, k=3, s=p.s, p=1, act=p.act, input_grad=1, x=p.raw, wt=p.wt, bias=p.bias,
                          dy=p.dz, dx0=p.dx0, dw0=p.dw0, db0=p.db0))
    got = D.backward(p, x, bn=False, overwrite=False)
    assert np.array_equal(D.forward(p, x)[0], want["y"])
    for key, ref in (("g", "dy_out"), ("dx", "dx"), ("dw", "dw"), ("db", "db")):
        R.assert_bits(key, got[key], want[ref])


@pytest.mark.parametrize("shape", [sh for sh, _ in D.SHAPES], ids=lambda s: "n%d_c%d_%dx%d_s%d" % s)
def test_backward_behind_batchnorm_is_the_oracle_fed_with_the_batchnorm_apply(shape):
    p = D.make_case(*shape, act=R.ACT_RELU, in_act=R.ACT_RELU, seed=2)
    x = D.case_input32(p)
    y = D.forward(p, x)[0]
    hw, c = p.oh * p.ow, p.c
    gin = B.bwd_apply32(p.dz.reshape(p.n, c, hw), y.reshape(p.n, c, hw), p.bn_mean, p.bn_var, p.bn_scale, p.bn_dmean, p.bn_dvar,
                        p.M).reshape(p.dz.shape)
    want = ob.orc_dw(dict(n=p.n, c=c, h=p.h, w=p.w, k=3, s=p.s, p=1, act=p.act, input_grad=1, x=x, wt=p.wt, bias=p.bias,
                          dy=np.ascontiguousarray(gin), dx0=p.dx0, dw0=p.dw0, db0=p.db0))
    got = D.backward(p, x, bn=True, overwrite=False)
    for key, ref in (("g", "dy_out"), ("dx", "dx"), ("dw", "dw"), ("db", "db")):
        R.assert_bits(key, got[key], want[ref])
    # the apply itself against float64: three terms of one to three roundings each, summed left to right
    ch = lambda v: np.asarray(v, F32).astype(F64).reshape(1, c, 1, 1)
    gs = np.where(ch(p.bn_scale) == 0, 0.0, p.dz.astype(F64) * ch(p.bn_scale))
    t1 = gs / np.sqrt(ch(p.bn_var) + F64(B.EPS_BWD))
    t2 = ch(p.bn_dvar) * 2.0 * (y.astype(F64) - ch(p.bn_mean)) / p.M
    t3 = ch(p.bn_dmean) / p.M
    _within("apply", gin, t1 + t2 + t3, 6 * U * (np.abs(t1) + np.abs(t2) + np.abs(t3)) + 1e-45)
    assert np.any(p.bn_scale == 0) and np.any(p.bn_scale == 1)
