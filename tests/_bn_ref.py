"""Plain numpy restatements of batch normalisation (bcnn_batchnorm_layer.c:196-242 forward, :263-281 sums and finalize,
:292-296 apply), for the kernel-level tests of csrc/batchnorm.hip and csrc/chan_reduce.h (test_batchnorm_edges.py).
TEST INFRASTRUCTURE ONLY.

Two forms of every step:
  *32   float32, one rounding per operation, in the order csrc/bn_math.h documents: subtract, correctly rounded divide, the
        bcnn_scal quirks (scale 0 gives 0, scale 1 skips the multiply), the bcnn_add_scalar quirk (a bias of exactly 0 or 1 is
        not added), then the activation map of tests/_next_ref.py. The finalize steps are written as the kernels write them
        (sums combined in double, rounded to float once, then float operations); the library is built with
        -ffp-contract=off and uses explicit _rn intrinsics, so numpy float32 arithmetic reproduces every step.
  *64   float64 throughout: what the project's tolerance bars are measured against.
test_bn_ref_pinning.py holds the float64 form to the C oracle and, where it is present, to the reference itself, so this file
states the reference and not the HIP code.

exact_inputs() draws tensors whose per-channel sums are exact in float32 IN ANY ORDER (small integers, means that are
multiples of 1/4): S, SS, S1, S2 are then known exactly on the host, every later step is a fixed chain of correctly rounded
operations, and the kernels are compared by value with np.array_equal instead of with a tolerance."""
import functools

import numpy as np

from tests._next_ref import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SOFTPLUS, ACT_TANH, F32, F64, act_factor32, act_factor64,
                             act_forward64)

MODE_PREDICT, MODE_TRAIN, MODE_VALID = 0, 1, 2
EPS_FWD, EPS_BWD = F32(0.000001), F32(0.00001)


def chan(v, c, dtype=F32):
    return np.asarray(v, dtype).reshape(1, c, 1)


def quiet(fn):
    """a constant channel divides 0 by almost 0 and a NaN pre-fill may pass through: no warnings from the restatement"""
    @functools.wraps(fn)
    def inner(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    return inner


# ---- float32, one rounding per operation ------------------------------------------------------------------------------------
@quiet
def normalize32(x, mean, var):
    """_norm_forward, :170-181: (x - mean) / sqrtf(var + 1e-6f); x is (n, c, hw)"""
    c = x.shape[1]
    rs = np.sqrt(chan(var, c) + EPS_FWD)
    return ((np.asarray(x, F32) - chan(mean, c)) / rs).astype(F32)


@quiet
def affine32(xn, scales, bias):
    """bcnn_scales then bcnn_add_bias with their quirks"""
    c = xn.shape[1]
    sc, b = chan(scales, c), chan(bias, c)
    v = np.where(sc == 0, F32(0), np.where(sc == 1, xn, xn * sc)).astype(F32)
    return np.where((b != 0) & (b != 1), v + b, v).astype(F32)


@quiet
def predict32(x, scales, bias):
    """scale_and_add_bias, :183-194: x * scale + bias, no quirks"""
    c = x.shape[1]
    return (np.asarray(x, F32) * chan(scales, c) + chan(bias, c)).astype(F32)


@quiet
def stats_finalize32(S, SS, M, run_mean0, run_var0):
    """(mean, var, run_mean, run_var) from the exact per-channel sums: mean = f32(S) * (1f / f32(M)),
    var = f32(SS) * inv - mean * mean, running = 0.1 * batch + 0.9 * running"""
    inv = F32(1) / F32(M)
    mean = (np.asarray(S, F64).astype(F32) * inv).astype(F32)
    var = (np.asarray(SS, F64).astype(F32) * inv - mean * mean).astype(F32)
    run_mean = (mean * F32(0.1) + np.asarray(run_mean0, F32) * F32(0.9)).astype(F32)
    run_var = (var * F32(0.1) + np.asarray(run_var0, F32) * F32(0.9)).astype(F32)
    return mean, var, run_mean, run_var


@quiet
def bwd_finalize32(S1, S2, scales, var, dscales0, dbias0):
    """(dbias, dscales, dmean, dvar) from the exact sums S1 = sum g, S2 = sum g (x - mean), as the finalize kernels write it"""
    S1, S2 = np.asarray(S1, F64), np.asarray(S2, F64)
    v, sc = np.asarray(var, F32), np.asarray(scales, F32)
    dbias = (np.asarray(dbias0, F32) + S1.astype(F32)).astype(F32)
    dscales = (np.asarray(dscales0, F32) + (S2 / np.sqrt(v + EPS_FWD).astype(F64)).astype(F32)).astype(F32)
    dmean = ((S1 * sc.astype(F64)).astype(F32) * (F32(-1) / np.sqrt(v + EPS_BWD))).astype(F32)
    dvar = ((S2 * sc.astype(F64)).astype(F32) * (F32(-0.5) / (v * np.sqrt(v) + EPS_BWD))).astype(F32)
    return dbias, dscales, dmean, dvar


@quiet
def bwd_apply32(g, x, mean, var, scales, dmean, dvar, M):
    """_normalize_backward, :292-296, on g = dy * act'(y) after bcnn_scales:
    (g * scale) / sqrtf(var + 1e-5f) + ((dvar * 2) * (x - mean)) / M + dmean / M, summed left to right"""
    c = x.shape[1]
    sc = chan(scales, c)
    g = np.asarray(g, F32)
    gs = np.where(sc == 0, F32(0), np.where(sc == 1, g, g * sc)).astype(F32)
    t1 = (gs / np.sqrt(chan(var, c) + EPS_BWD)).astype(F32)
    t2 = (((chan(dvar, c) * F32(2)) * (np.asarray(x, F32) - chan(mean, c))) / F32(M)).astype(F32)
    return ((t1 + t2) + chan(dmean, c) / F32(M)).astype(F32)


def act_grad32(dy, y, act):
    """dy * act'(y), one float32 multiply (dy itself for NONE)"""
    if act == ACT_NONE:
        return np.asarray(dy, F32).copy()
    return (np.asarray(dy, F32) * act_factor32(y, act)).astype(F32)


# ---- float64 ----------------------------------------------------------------------------------------------------------------
@quiet
def forward64(x, run_mean0, run_var0, scales, bias, mode, act=ACT_NONE):
    """bcnn_forward_batchnorm_cpu in float64 on the float32 inputs; x is (n, c, hw). Returns the keys of oracle.orc_bind.orc_bn
    plus x_norm; `y` is the activation evaluated in float64 on the float32-rounded pre-activation value."""
    x = np.asarray(x, F32).astype(F64)
    n, c, hw = x.shape
    sc, b = chan(scales, c).astype(F64), chan(bias, c).astype(F64)
    out = {"run_mean": np.asarray(run_mean0, F64).copy(), "run_var": np.asarray(run_var0, F64).copy()}
    if mode == MODE_PREDICT:
        pre = x * sc + b
    else:
        mean, var = out["run_mean"], out["run_var"]
        if mode == MODE_TRAIN:
            mean = x.mean(axis=(0, 2))
            var = (x * x).mean(axis=(0, 2)) - mean * mean
            out["saved_mean"], out["saved_var"] = mean, var
            out["run_mean"] = F64(F32(0.1)) * mean + F64(F32(0.9)) * out["run_mean"]
            out["run_var"] = F64(F32(0.1)) * var + F64(F32(0.9)) * out["run_var"]
        xn = (x - chan(mean, c, F64)) / np.sqrt(chan(var, c, F64) + F64(EPS_FWD))
        out["x_norm"] = xn
        pre = np.where(sc == 0, 0.0, xn * sc)
        pre = np.where((b != 0) & (b != 1), pre + b, pre)       # the bcnn_add_scalar quirk is an O(1) effect: kept
    out["pre"] = pre
    out["y"] = act_forward64(pre.astype(F32), act)
    return out


@quiet
def backward64(dy, x, scales, mean, var, dscales0, dbias0, y=None, act=ACT_NONE):
    """bcnn_backward_batchnorm_cpu in float64 (after the activation backward of a fused node): db, dscales, dmean, dvar and
    dy_out (= dx)"""
    x, g = np.asarray(x, F32).astype(F64), np.asarray(dy, F32).astype(F64)
    n, c, hw = x.shape
    M = n * hw
    if act != ACT_NONE:
        g = g * act_factor64(y, act)
    m, v, sc = chan(mean, c).astype(F64), chan(var, c).astype(F64), chan(scales, c).astype(F64)
    d = x - m
    out = {"db": np.asarray(dbias0, F64) + g.sum(axis=(0, 2)),
           "dscales": np.asarray(dscales0, F64) + (g * d / np.sqrt(v + F64(EPS_FWD))).sum(axis=(0, 2))}
    gs = g * sc
    rs5 = np.sqrt(v + F64(EPS_BWD))
    out["dmean"] = gs.sum(axis=(0, 2)) * (-1.0 / rs5.ravel())
    out["dvar"] = (gs * d).sum(axis=(0, 2)) * (-0.5 / (v.ravel() * np.sqrt(v.ravel()) + F64(EPS_BWD)))
    out["dy_out"] = gs / rs5 + chan(out["dvar"], c, F64) * 2.0 * d / M + chan(out["dmean"], c, F64) / M
    out["dx"] = out["dy_out"]
    return out


# ---- inputs whose sums are exact ----------------------------------------------------------------------------------------------
GRAIN = 16.0        # every summand is a multiple of 1 / GRAIN (x - mean: 1/4; the tanh factor 3/4 on top: 1/16)
LIMIT = 2.0 ** 24


def channel_sums(v, n, c, hw):
    return np.asarray(v, F64).reshape(n, c, hw).sum(axis=(0, 2))


def assert_exact_sums(what, v, n, c, hw):
    """every element a multiple of 1 / GRAIN and GRAIN * sum |v| < 2^24 per channel: any partial sum, in any order and
    any grouping, is then a multiple of 1 / GRAIN below 2^24 / GRAIN and therefore a float32 number"""
    s = np.asarray(v, F64).reshape(n, c, hw) * GRAIN
    assert np.array_equal(s, np.round(s)), "%s: not a multiple of 1/%d" % (what, GRAIN)
    assert float(np.abs(s).sum(axis=(0, 2)).max()) < LIMIT, "%s: a partial sum may leave the exact range" % what


class Case:
    """the tensors and per-channel constants of one test case (hashable by identity: expectations are cached per case)"""


def channel_params(c, rs):
    """per-channel constants that tell the channels apart (a wrong channel index is an O(1) error), with the special
    channels of the reference's quirks: 1: scale 1 and bias 0; 2: scale 0; 3: bias 1; the last one (c >= 4): var 0"""
    j = np.arange(c)
    p = Case()
    p.scales = (F32(0.37) * (1 + j % 17) * np.where(j % 2, -1, 1)).astype(F32)
    p.bias = (F32(0.81) * (j % 13 - 6) + F32(0.05)).astype(F32)
    p.mean = (0.25 * (j % 11 - 5)).astype(F32)                      # multiples of 1/4
    p.var = (F32(0.3) + F32(0.47) * (j % 7)).astype(F32)
    p.run_mean0 = (p.mean + rs.uniform(-0.2, 0.2, c)).astype(F32)
    p.run_var0 = (p.var * rs.uniform(0.8, 1.2, c)).astype(F32)
    p.dscales0 = rs.uniform(-3, 3, c).astype(F32)                   # carry-in: both gradients accumulate
    p.dbias0 = rs.uniform(-3, 3, c).astype(F32)
    p.const = c - 1 if c >= 4 else -1
    if c >= 2:
        p.scales[1], p.bias[1] = 1, 0
    if c >= 3:
        p.scales[2] = 0
    if c >= 5:
        p.bias[3] = 1
    if p.const >= 0:
        p.var[p.const] = 0
        p.mean[p.const] = 1
    return p


# post-activation values whose derivative factor is exact, so that g = dy * act'(y) stays on the grid:
#   RELU 0 / 1; LRELU 1 / 0.1f with dy a multiple of 10 (10 * 0.1f and 20 * 0.1f round to 1 and 2); TANH 1 - y * y = 1 or 3/4;
#   SOFTPLUS 1 / (1 + (float)exp(-y)) = 1/2 at y = 0 and 1 at y = 100 (exp(-100) vanishes next to 1 in float32)
EXACT_Y = {ACT_RELU: [-1.0, 0.0, 2.0], ACT_LRELU: [-1.0, 0.0, 2.0], ACT_TANH: [-0.5, 0.0, 0.5], ACT_SOFTPLUS: [0.0, 100.0]}


@functools.lru_cache(maxsize=None)
def exact_inputs(n, c, hw, dy_max=2, act=ACT_NONE):
    """x integers in -4..4, dy integers in -dy_max..dy_max (times 10 for LRELU), statistics as channel_params. The generator
    asserts its own precondition: per channel, sum x^2 and GRAIN * sum |g (x - mean)| stay below 2^24. Cached: the tensors
    are shared between tests and must not be modified."""
    rs = np.random.RandomState((n * 1000003 + c * 10007 + hw * 101 + act) % (2 ** 31))
    p = channel_params(c, rs)
    p.n, p.c, p.hw, p.M, p.act = n, c, hw, n * hw, act
    p.x = rs.randint(-4, 5, (n, c, hw)).astype(F32)
    if p.const >= 0:
        p.x[:, p.const, :] = 1                                      # a constant channel: var = 0
    p.dy = (rs.randint(-dy_max, dy_max + 1, (n, c, hw)) * (10 if act == ACT_LRELU else 1)).astype(F32)
    p.y = rs.choice(EXACT_Y[act], (n, c, hw)).astype(F32) if act != ACT_NONE else None
    p.g = act_grad32(p.dy, p.y, act)
    assert_exact_sums("x", p.x, n, c, hw)
    assert_exact_sums("x^2", p.x.astype(F64) ** 2, n, c, hw)
    assert_exact_sums("g", p.g, n, c, hw)
    d32 = (p.x - chan(p.mean, c)).astype(F32)
    prod = (p.g * d32).astype(F32)
    assert np.array_equal(prod.astype(F64), p.g.astype(F64) * (p.x.astype(F64) - chan(p.mean, c, F64)))   # exact products
    assert_exact_sums("g (x - mean)", prod, n, c, hw)
    p.S, p.SS = channel_sums(p.x, n, c, hw), channel_sums(p.x.astype(F64) ** 2, n, c, hw)
    p.S1, p.S2 = channel_sums(p.g, n, c, hw), channel_sums(prod, n, c, hw)
    for a in (p.x, p.dy, p.g) + ((p.y,) if p.y is not None else ()):
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def uniform_inputs(n, c, hw):
    """the realism case: uniform float data with per-channel offsets; held to the float64 form under the project's bars"""
    rs = np.random.RandomState(n + 7 * c + 13 * hw)
    p = channel_params(c, rs)
    p.n, p.c, p.hw, p.M, p.act = n, c, hw, n * hw, ACT_NONE
    p.x = (rs.uniform(-1, 1, (n, c, hw)) + chan(p.mean, c)).astype(F32)
    p.dy = rs.uniform(-0.1, 0.1, (n, c, hw)).astype(F32)
    x64 = p.x.astype(F64)
    p.mean = x64.mean(axis=(0, 2)).astype(F32)                      # consistent statistics for the entry points that take them
    p.var = ((x64 * x64).mean(axis=(0, 2)) - x64.mean(axis=(0, 2)) ** 2).astype(F32)
    p.y = None
    for a in (p.x, p.dy):
        a.setflags(write=False)
    return p


def split_exact(rs, total, splits, spread=1000):
    """`splits` random integers that add up to the integer `total` (float64 array, one row per channel): the partials a
    wide finalize kernel is given. Every part is a float32 number and every partial sum is exact in the kernels' double
    accumulators, so the result is the same bit pattern for every `splits`."""
    total = np.asarray(total, F64)
    parts = rs.randint(-spread, spread + 1, (total.size, splits)).astype(F64)
    parts[:, -1] = total - parts[:, :-1].sum(axis=1)
    assert np.array_equal(parts.sum(axis=1), total) and np.array_equal(parts.astype(F32).astype(F64), parts)
    assert float(np.abs(parts).sum(axis=1).max()) * GRAIN < 2.0 ** 52
    return parts
