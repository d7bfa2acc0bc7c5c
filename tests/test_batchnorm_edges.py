"""Batch normalisation (csrc/batchnorm.hip) and the per-channel sweeps it runs on (csrc/chan_reduce.h), entry point by entry
point through the C-ABI, at the shapes where the dispatch conditions change. The six bn_* goldens stay at M <= 768 and
HW <= 256: one split per channel, the first sweep of flat_map_kernel, no activation, no x_norm.

The bar comes from the inputs (tests/_bn_ref.py: exact_inputs): x, dy are small integers and the statistics passed in are
multiples of 1/4, so every partial sum of StatsF / BwdSumsF is exact in float32 in any order, S, SS, S1, S2 are known on the
host, and everything behind them is a fixed chain of correctly rounded float32 operations. Every result is compared BY VALUE
(np.array_equal; signed zeros are equal, bn_math.h: -0 / d gives +0) with the float32 form of _bn_ref.py; only the separate
tanh pass gets the ACT bar of _next_ref.assert_bar. One realism case per entry point (uniform float data) is held to the
float64 form under the bars of test_hip_parity.py. Every device tensor is a Guarded view, outputs are pre-filled with NaN.

  reductions (splits = min(ceil(1024 / C), ceil(M / 4096), 1024), M = N * HW)
      (2, 3, 100)      vector path, one split, most threads idle
      (23, 3, 196)     two splits of 2256: the second starts mid-image; a 1024-element stride hops five images
      (90, 3, 49)      scalar path, two splits, ragged last slice
      (5, 5, 1..3)     planes shorter than a float4
      (10, 1, 4096)    ten splits, one channel
      (9, 300, 1024)   ceil(1024 / C) = 4 but ceil(M / 4096) = 3: M decides
      (3, 257, 20)     crosses the 256-thread finalize block
  maps (plane_map_kernel for HW >= 1024, else flat_map_kernel; one flat sweep covers 2048 x 1024 elements)
      HW 1024 / 1027 / 4100 / 5000   one row; planes off 16 bytes, a 3-element tail; a chunk of 4 elements; ragged
      (186, 31, 729)   4 203 414 elements: three sweeps, the carried (in, c) step taken twice
      (7, 1, 49), (5, 5, 1..3), totals of 1, 3, 4 and 5 elements
  pointers one float off 16 bytes: only the entry points whose every sweep carries an alignment flag (_apply,
  _backward_apply, _forward in VALID / PREDICT mode); the reduction sweeps require aligned tensors (include/bcnn_hip.h)."""
import functools
import types

import numpy as np
import pytest

from tests import _bn_ref as B
from tests import _golden as G
from tests import _next_ref as R
from tests.test_hip_parity import ACT_TOL, REL_TOL, VAR_KEYS

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TRAIN, VALID, PREDICT = B.MODE_TRAIN, B.MODE_VALID, B.MODE_PREDICT
MODE_NAMES = {TRAIN: "train", VALID: "valid", PREDICT: "predict"}

REDUCE_SHAPES = [(2, 3, 100), (23, 3, 196), (90, 3, 49), (5, 5, 1), (5, 5, 2), (5, 5, 3), (10, 1, 4096), (9, 300, 1024),
                 (3, 257, 20)]
MAP_SHAPES = [(2, 3, 1024), (2, 3, 1027), (1, 2, 4100), (2, 2, 5000), (186, 31, 729), (7, 1, 49), (5, 5, 1), (5, 5, 2),
              (5, 5, 3), (1, 1, 1), (3, 1, 1), (2, 2, 1), (1, 5, 1)]
VARIANT_SHAPES = [(7, 5, 196), (2, 5, 1027)]        # one flat-map and one plane-map shape, all special channels present
MISALIGNED_SHAPES = [(4, 3, 100), (2, 3, 1024)]     # HW % 4 == 0: aligned pointers take the float4 bodies here
WIDE_SPLITS = [1, 63, 1024, 3073, 9001]             # 3073: the first value that enters the four-in-flight loop
WIDE_CHANNELS = [1, 5]
FWD_ACTS = [R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU, R.ACT_CLAMP, R.ACT_RAMP, R.ACT_ABS, R.ACT_TANH]
BWD_ACTS = [R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU, R.ACT_SOFTPLUS, R.ACT_TANH]
REAL_SHAPE = (23, 5, 196)                           # two splits per channel, a slice boundary inside an image

shape_id = lambda s: "x".join(str(v) for v in s)
act_id = lambda a: R.ACT_NAMES[a]


def key(shape, act=R.ACT_NONE):
    """arguments of exact_inputs: dy from -1..1 in the largest case, -2..2 elsewhere"""
    return tuple(shape) + (1 if int(np.prod(shape)) > 4000000 else 2, act)


def case(shape, act=R.ACT_NONE):
    return B.exact_inputs(*key(shape, act))


def all_exact_cases():
    """every exact_inputs() argument tuple this module draws (test_bn_ref_pinning.py generates each on the CPU)"""
    out = [key(s) for s in REDUCE_SHAPES + MAP_SHAPES + VARIANT_SHAPES + MISALIGNED_SHAPES]
    out += [key(s, a) for s in VARIANT_SHAPES for a in BWD_ACTS]
    out += [key((2, c, 100)) for c in WIDE_CHANNELS]
    return sorted(set(out))


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401
    from bcnn_amd import _lib
    return _lib.load()


# ---- buffers and comparisons ---------------------------------------------------------------------------------------------
def nan(size, shift=0):
    return R.Guarded(np.full(size, np.nan, F32), shift)


def ptr(g):
    return None if g is None else g.ptr


def same(tag, got, want):
    """equal by value, element by element; a NaN (an output element the kernel skipped) is never equal"""
    got, want = np.asarray(got, F32).ravel(), np.asarray(want, F32).ravel()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(~(got == want))
        raise AssertionError("%s: %d of %d elements differ, first at %d: got %r want %r"
                             % (tag, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


def close(tag, got, want64):
    """the bars of test_hip_parity.py: REL_TOL through G.assert_close; rtol 1e-4 / atol 1e-6 for the variance keys"""
    got, want64 = np.asarray(got, F32).ravel(), np.asarray(want64, F64).ravel()
    if tag.split("/")[-1] in VAR_KEYS:
        assert np.allclose(got, want64, rtol=1e-4, atol=1e-6), (tag, np.abs(got - want64).max())
    else:
        G.assert_close(tag, got, want64, REL_TOL, rtol=REL_TOL, afrac=REL_TOL / 10)


def check_y(tag, got, pre32, act):
    """y = act(pre): the cheap activations are exact float32 steps fused into the sweep (the library is built without
    contraction); tanh is the separate bcnn_hip_activation_forward pass and gets its ACT bar"""
    if R.FWD_BAR[act] == R.ACT:
        R.assert_bar(R.ACT, tag, got, None, R.act_forward64(pre32, act), ACT_TOL)
    else:
        same(tag, got, R.act_forward32(pre32, act))


# ---- forward -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expect_forward(p, mode):
    """the float32 form on exact inputs (computed once per case and mode, shared, never modified)"""
    e = types.SimpleNamespace(xn=None)
    if mode == PREDICT:
        e.pre = B.predict32(p.x, p.scales, p.bias)
        return e
    if mode == TRAIN:
        e.mean, e.var, e.run_mean, e.run_var = B.stats_finalize32(p.S, p.SS, p.M, p.run_mean0, p.run_var0)
    else:
        e.mean, e.var = p.run_mean0, p.run_var0
    e.xn = B.normalize32(p.x, e.mean, e.var)
    e.pre = B.affine32(e.xn, p.scales, p.bias)
    return e


def run_forward(L, p, mode, act=R.ACT_NONE, xn=True, ws="sep", shift=(), stats=None):
    total, c = p.n * p.c * p.hw, p.c
    sh = lambda k: 1 if k in shift else 0
    t = types.SimpleNamespace()
    t.x, t.y = R.Guarded(p.x, sh("x")), nan(total, sh("y"))
    t.run_mean, t.run_var = R.Guarded(p.run_mean0), R.Guarded(p.run_var0)
    t.scales, t.bias = R.Guarded(p.scales), R.Guarded(p.bias)
    t.saved_mean, t.saved_var = nan(c), nan(c)
    t.xn = nan(total, sh("xn")) if xn else None
    t.ws = t.x if ws == "x" else (nan(total, sh("ws")) if ws == "sep" else None)
    args = [t.x.ptr, t.y.ptr, t.run_mean.ptr, t.run_var.ptr, t.scales.ptr, t.bias.ptr, t.saved_mean.ptr, t.saved_var.ptr,
            ptr(t.xn), ptr(t.ws), p.n, p.c, p.hw, mode, act]
    if stats is None:
        L.bcnn_hip_batchnorm_forward(*args)
    else:
        t.stats = R.Guarded(stats)
        L.bcnn_hip_batchnorm_forward_stats(*(args + [t.stats.ptr, stats.shape[1]]))
    L.bcnn_hip_sync()
    return t


def check_forward(tag, p, t, mode, act, exact=True):
    """every tensor of a forward call: what must be written is compared, what must be left alone is bit-unchanged"""
    for name in ("scales", "bias") + (("x",) if t.ws is not t.x else ()):
        getattr(t, name).assert_unchanged(tag + "/" + name)
    if exact:
        e = expect_forward(p, mode)
        cmp, pre, xn = same, e.pre, e.xn
        stats = dict(saved_mean=getattr(e, "mean", None), saved_var=getattr(e, "var", None),
                     run_mean=getattr(e, "run_mean", None), run_var=getattr(e, "run_var", None))
    else:
        f = B.forward64(p.x, p.run_mean0, p.run_var0, p.scales, p.bias, mode, act)
        cmp, xn, stats = close, f.get("x_norm"), f
    if mode == TRAIN:
        for k in ("saved_mean", "saved_var", "run_mean", "run_var"):
            cmp(tag + "/" + k, getattr(t, k).read(), stats[k])
    else:
        for k in ("saved_mean", "saved_var", "run_mean", "run_var"):
            getattr(t, k).assert_unchanged(tag + "/" + k)
    if exact:
        check_y(tag + "/y", t.y.read(), pre, act)
    else:
        close(tag + "/y", t.y.read(), f["y"])
    if t.xn is not None:
        if mode == TRAIN:
            cmp(tag + "/x_norm", t.xn.read(), xn)
        else:
            t.xn.assert_unchanged(tag + "/x_norm")
    if t.ws is t.x:
        same(tag + "/x as workspace", t.x.read(), p.x)
    elif t.ws is not None:
        if mode == PREDICT:
            t.ws.assert_unchanged(tag + "/workspace")
        else:
            same(tag + "/workspace", t.ws.read(), p.x)


def run_apply(L, p, act, shift=()):
    t = types.SimpleNamespace()
    t.x, t.y = R.Guarded(p.x, 1 if "x" in shift else 0), nan(p.x.size, 1 if "y" in shift else 0)
    t.consts = [R.Guarded(v) for v in (p.scales, p.bias, p.mean, p.var)]
    L.bcnn_hip_batchnorm_apply(t.x.ptr, t.y.ptr, *([g.ptr for g in t.consts] + [p.n, p.c, p.hw, act]))
    L.bcnn_hip_sync()
    for g in [t.x] + t.consts:
        g.assert_unchanged("apply input")
    return t


def check_apply(tag, p, t, act):
    check_y(tag + "/y", t.y.read(), B.affine32(B.normalize32(p.x, p.mean, p.var), p.scales, p.bias), act)


# ---- backward ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expect_backward(p):
    e = types.SimpleNamespace()
    e.db, e.dscales, e.dmean, e.dvar = B.bwd_finalize32(p.S1, p.S2, p.scales, p.var, p.dscales0, p.dbias0)
    e.dx = B.bwd_apply32(p.g, p.x, p.mean, p.var, p.scales, e.dmean, e.dvar, p.M)
    return e


def backward_buffers(p, dx="sep", shift=()):
    sh = lambda k: 1 if k in shift else 0
    t = types.SimpleNamespace()
    t.dy, t.x = R.Guarded(p.dy, sh("dy")), R.Guarded(p.x, sh("x"))
    t.dx = t.dy if dx == "same" else (nan(p.x.size, sh("dx")) if dx == "sep" else None)
    t.y = R.Guarded(p.y) if p.y is not None else None
    t.scales, t.mean, t.var = R.Guarded(p.scales), R.Guarded(p.mean), R.Guarded(p.var)
    t.dscales, t.db = R.Guarded(p.dscales0), R.Guarded(p.dbias0)      # non-zero carry-in
    t.dmean, t.dvar = nan(p.c), nan(p.c)                               # overwritten, not accumulated
    return t


def run_backward(L, p, dx="sep"):
    t = backward_buffers(p, dx)
    L.bcnn_hip_batchnorm_backward(t.dy.ptr, ptr(t.dx), ptr(t.y), p.act, t.scales.ptr, t.dscales.ptr, t.db.ptr, t.mean.ptr,
                                  t.var.ptr, t.dmean.ptr, t.dvar.ptr, None, t.x.ptr, p.n, p.c, p.hw)
    L.bcnn_hip_sync()
    return t


def run_backward_sums(L, p):
    t = backward_buffers(p, None)
    L.bcnn_hip_batchnorm_backward_sums(t.dy.ptr, t.scales.ptr, t.dscales.ptr, t.db.ptr, t.mean.ptr, t.var.ptr, t.dmean.ptr,
                                       t.dvar.ptr, t.x.ptr, p.n, p.c, p.hw)
    L.bcnn_hip_sync()
    return t


def check_backward(tag, p, t, exact=True, sums_only=False):
    for name in ("x", "scales", "mean", "var") + (("y",) if t.y is not None else ()) + (("dy",) if sums_only else ()):
        getattr(t, name).assert_unchanged(tag + "/" + name)
    if exact:
        e, cmp = expect_backward(p), same
        want = dict(db=e.db, dscales=e.dscales, dmean=e.dmean, dvar=e.dvar, dy_out=e.dx)
    else:
        want, cmp = B.backward64(p.dy, p.x, p.scales, p.mean, p.var, p.dscales0, p.dbias0), close
    for k in ("db", "dscales", "dmean", "dvar"):
        cmp(tag + "/" + k, getattr(t, k).read(), want[k])
    if sums_only:
        return
    cmp(tag + "/dy_out", t.dy.read(), want["dy_out"])
    if t.dx is not None and t.dx is not t.dy:
        cmp(tag + "/dx", t.dx.read(), want["dy_out"])


def given_gradients(p):
    """dmean / dvar handed to _backward_apply: any floats, different per channel"""
    return (p.dbias0 * F32(7.3)).astype(F32), (p.dscales0 * F32(1.7)).astype(F32)


def run_backward_apply(L, p, dx="sep", shift=(), dmean=None, dvar=None):
    t = backward_buffers(p, dx, shift)
    if dmean is None:
        dmean, dvar = given_gradients(p)
    t.dmean, t.dvar = R.Guarded(dmean), R.Guarded(dvar)
    L.bcnn_hip_batchnorm_backward_apply(t.dy.ptr, ptr(t.dx), t.scales.ptr, t.mean.ptr, t.var.ptr, t.dmean.ptr, t.dvar.ptr,
                                        t.x.ptr, p.n, p.c, p.hw)
    L.bcnn_hip_sync()
    for name in ("x", "scales", "mean", "var", "dmean", "dvar", "dscales", "db"):
        getattr(t, name).assert_unchanged(name)
    return t


def check_backward_apply(tag, p, t):
    dmean, dvar = given_gradients(p)
    want = B.bwd_apply32(p.dy, p.x, p.mean, p.var, p.scales, dmean, dvar, p.M)
    same(tag + "/dy_out", t.dy.read(), want)
    if t.dx is not None and t.dx is not t.dy:
        same(tag + "/dx", t.dx.read(), want)


def run_stats_only(L, p, stats=None):
    t = types.SimpleNamespace(ws=None, xn=None)
    t.x, t.scales, t.bias = R.Guarded(p.x), R.Guarded(p.scales), R.Guarded(p.bias)
    t.run_mean, t.run_var, t.saved_mean, t.saved_var = R.Guarded(p.run_mean0), R.Guarded(p.run_var0), nan(p.c), nan(p.c)
    t.stats = R.Guarded(stats) if stats is not None else None
    L.bcnn_hip_batchnorm_forward_stats_only(t.x.ptr, t.run_mean.ptr, t.run_var.ptr, t.scales.ptr, t.bias.ptr,
                                            t.saved_mean.ptr, t.saved_var.ptr, p.n, p.c, p.hw, ptr(t.stats),
                                            0 if stats is None else stats.shape[1])
    L.bcnn_hip_sync()
    return t


def check_stats(tag, p, t, exact=True):
    for name in ("x", "scales", "bias"):
        getattr(t, name).assert_unchanged(tag + "/" + name)
    if exact:
        e, cmp = expect_forward(p, TRAIN), same
        want = dict(saved_mean=e.mean, saved_var=e.var, run_mean=e.run_mean, run_var=e.run_var)
    else:
        want, cmp = B.forward64(p.x, p.run_mean0, p.run_var0, p.scales, p.bias, TRAIN), close
    for k in ("saved_mean", "saved_var", "run_mean", "run_var"):
        cmp(tag + "/" + k, getattr(t, k).read(), want[k])


# ---- the reductions at their dispatch edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["forward", "backward", "backward_sums", "stats_only"])
@pytest.mark.parametrize("shape", REDUCE_SHAPES, ids=shape_id)
def test_reductions_are_exact_on_exact_inputs(L, shape, entry):
    p = case(shape)
    tag = "%s/%s" % (entry, shape_id(shape))
    if entry == "forward":
        check_forward(tag, p, run_forward(L, p, TRAIN), TRAIN, R.ACT_NONE)
    elif entry == "backward":
        check_backward(tag, p, run_backward(L, p))
    elif entry == "backward_sums":
        check_backward(tag, p, run_backward_sums(L, p), sums_only=True)
    else:
        check_stats(tag, p, run_stats_only(L, p))


# ---- the maps at their dispatch edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["forward_train", "forward_valid", "forward_predict", "apply", "backward", "backward_apply"])
@pytest.mark.parametrize("shape", MAP_SHAPES, ids=shape_id)
def test_maps_are_exact_on_exact_inputs(L, shape, entry):
    p = case(shape)
    tag = "%s/%s" % (entry, shape_id(shape))
    if entry.startswith("forward"):
        mode = {"forward_train": TRAIN, "forward_valid": VALID, "forward_predict": PREDICT}[entry]
        check_forward(tag, p, run_forward(L, p, mode), mode, R.ACT_NONE)
    elif entry == "apply":
        check_apply(tag, p, run_apply(L, p, R.ACT_RELU), R.ACT_RELU)
    elif entry == "backward":
        check_backward(tag, p, run_backward(L, p))
    else:
        check_backward_apply(tag, p, run_backward_apply(L, p))


MISALIGNED = {"apply": ("x", "y"), "backward_apply": ("dy", "dx", "x"), "forward_valid": ("x", "y", "ws", "xn"),
              "forward_predict": ("x", "y", "xn")}


@pytest.mark.parametrize("entry", sorted(MISALIGNED))
@pytest.mark.parametrize("shape", MISALIGNED_SHAPES, ids=shape_id)
def test_maps_with_pointers_one_float_off_16_bytes(L, shape, entry):
    """one tensor at a time, then all of them: any misaligned tensor must send the whole sweep down the scalar bodies"""
    p = case(shape)
    names = MISALIGNED[entry]
    for shift in [(k,) for k in names] + [names]:
        tag = "%s/%s/off:%s" % (entry, shape_id(shape), "+".join(shift))
        if entry == "apply":
            check_apply(tag, p, run_apply(L, p, R.ACT_NONE, shift), R.ACT_NONE)
        elif entry == "backward_apply":
            check_backward_apply(tag, p, run_backward_apply(L, p, "sep", shift))
        else:
            mode = VALID if entry == "forward_valid" else PREDICT
            check_forward(tag, p, run_forward(L, p, mode, R.ACT_LRELU, shift=shift), mode, R.ACT_LRELU)


# ---- variants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", FWD_ACTS, ids=act_id)
@pytest.mark.parametrize("mode", [TRAIN, VALID, PREDICT], ids=lambda m: MODE_NAMES[m])
@pytest.mark.parametrize("shape", VARIANT_SHAPES, ids=shape_id)
def test_forward_modes_and_activations(L, shape, mode, act):
    """the cheap activations fused into the sweep; TANH through the separate pass and its hw / c arguments"""
    p = case(shape)
    check_forward("fwd/%s/%s/%s" % (shape_id(shape), MODE_NAMES[mode], act_id(act)), p, run_forward(L, p, mode, act), mode, act)


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_ABS, R.ACT_TANH], ids=act_id)
@pytest.mark.parametrize("shape", VARIANT_SHAPES, ids=shape_id)
def test_apply_activations(L, shape, act):
    p = case(shape)
    check_apply("apply/%s/%s" % (shape_id(shape), act_id(act)), p, run_apply(L, p, act), act)


@pytest.mark.parametrize("mode,xn,ws", [(TRAIN, False, "sep"), (TRAIN, True, "x"), (TRAIN, True, None), (TRAIN, False, None),
                                        (TRAIN, False, "x"), (VALID, True, "x"), (VALID, False, None), (PREDICT, False, None)],
                         ids=["train-noxn-sep", "train-xn-inplace", "train-xn-nows", "train-noxn-nows", "train-noxn-inplace",
                              "valid-xn-inplace", "valid-noxn-nows", "predict-noxn-nows"])
@pytest.mark.parametrize("shape", VARIANT_SHAPES, ids=shape_id)
def test_forward_optional_outputs(L, shape, mode, xn, ws):
    """x_norm given or NULL; the workspace separate (the other tests), the input itself, or NULL"""
    p = case(shape)
    tag = "fwd/%s/%s/xn=%s/ws=%s" % (shape_id(shape), MODE_NAMES[mode], xn, ws)
    check_forward(tag, p, run_forward(L, p, mode, R.ACT_RELU, xn=xn, ws=ws), mode, R.ACT_RELU)


@pytest.mark.parametrize("dx", ["sep", "same", None], ids=lambda v: "dx=%s" % v)
@pytest.mark.parametrize("act", BWD_ACTS, ids=act_id)
@pytest.mark.parametrize("shape", VARIANT_SHAPES, ids=shape_id)
def test_backward_activations_and_outputs(L, shape, act, dx):
    """RELU / LRELU / TANH with y given: the use_y branch of both functors (y is drawn independently of x, so reading x
    for y shows); SOFTPLUS: the detour through bcnn_hip_activation_backward. The derivative factors are exact for the
    drawn y (_bn_ref.EXACT_Y), so the sums stay exact."""
    p = case(shape, act)
    check_backward("bwd/%s/%s/dx=%s" % (shape_id(shape), act_id(act), dx), p, run_backward(L, p, dx))


@pytest.mark.parametrize("dx", ["same", None], ids=lambda v: "dx=%s" % v)
@pytest.mark.parametrize("shape", VARIANT_SHAPES, ids=shape_id)
def test_backward_apply_outputs(L, shape, dx):
    p = case(shape)
    check_backward_apply("bwd_apply/%s/dx=%s" % (shape_id(shape), dx), p, run_backward_apply(L, p, dx))


# ---- the wide finalize kernels, partials made here ---------------------------------------------------------------------------
def partials(rs, a, b, splits):
    """(c, splits, 2) float32: the exact sums a, b split into `splits` random integer parts"""
    return np.stack([B.split_exact(rs, a, splits), B.split_exact(rs, b, splits)], axis=2).astype(F32)


@pytest.mark.parametrize("c", WIDE_CHANNELS)
@pytest.mark.parametrize("splits", WIDE_SPLITS)
def test_wide_statistics_finalize(L, splits, c):
    p = case((2, c, 100))
    st = partials(np.random.RandomState(splits + c), p.S, p.SS, splits)
    tag = "wide_stats/c%d/splits%d" % (c, splits)
    t = run_forward(L, p, TRAIN, R.ACT_NONE, stats=st)
    t.stats.assert_unchanged(tag + "/stats")
    check_forward(tag + "/forward_stats", p, t, TRAIN, R.ACT_NONE)
    t = run_stats_only(L, p, st)
    t.stats.assert_unchanged(tag + "/stats")
    check_stats(tag + "/stats_only", p, t)


@functools.lru_cache(maxsize=None)
def sums_on_device(L, c):
    """what _backward_sums leaves for the tensors the partials come from (run once per channel count)"""
    t = run_backward_sums(L, case((2, c, 100)))
    return {k: getattr(t, k).read() for k in ("db", "dscales", "dmean", "dvar")}


@pytest.mark.parametrize("c", WIDE_CHANNELS)
@pytest.mark.parametrize("splits", WIDE_SPLITS)
def test_wide_backward_finalize(L, splits, c):
    p = case((2, c, 100))
    sums = R.Guarded(partials(np.random.RandomState(splits + 7 * c), p.S1, p.S2, splits))
    t = backward_buffers(p, None)
    L.bcnn_hip_batchnorm_backward_finalize(sums.ptr, splits, t.scales.ptr, t.dscales.ptr, t.db.ptr, t.var.ptr, t.dmean.ptr,
                                           t.dvar.ptr, c)
    L.bcnn_hip_sync()
    sums.assert_unchanged("sums")
    tag = "wide_bwd/c%d/splits%d" % (c, splits)
    check_backward(tag, p, t, sums_only=True)
    for k, v in sums_on_device(L, c).items():
        same(tag + "/" + k + " against _backward_sums", getattr(t, k).read(), v)


# ---- realism: uniform float data against the float64 form, the project's bars --------------------------------------------
def image_partials(a, b):
    """(c, n, 2): one partial per image, each a float64 sum rounded to float32"""
    return np.stack([a.astype(F64).sum(axis=2).T, b.astype(F64).sum(axis=2).T], axis=2).astype(F32)


@pytest.mark.parametrize("entry", ["forward", "forward_valid", "apply", "backward", "backward_sums", "backward_apply",
                                   "forward_stats", "stats_only", "backward_finalize"])
def test_uniform_data_against_float64(L, entry):
    p = B.uniform_inputs(*REAL_SHAPE)
    tag = "real/" + entry
    x64 = p.x.astype(F64)
    if entry == "forward":
        check_forward(tag, p, run_forward(L, p, TRAIN), TRAIN, R.ACT_NONE, exact=False)
    elif entry == "forward_valid":
        check_forward(tag, p, run_forward(L, p, VALID), VALID, R.ACT_NONE, exact=False)
    elif entry == "apply":
        t = run_apply(L, p, R.ACT_NONE)
        close(tag + "/y", t.y.read(), B.forward64(p.x, p.mean, p.var, p.scales, p.bias, VALID)["y"])
    elif entry == "backward":
        check_backward(tag, p, run_backward(L, p), exact=False)
    elif entry == "backward_sums":
        check_backward(tag, p, run_backward_sums(L, p), exact=False, sums_only=True)
    elif entry == "backward_apply":
        b = B.backward64(p.dy, p.x, p.scales, p.mean, p.var, p.dscales0, p.dbias0)
        t = run_backward_apply(L, p, "sep", dmean=b["dmean"].astype(F32), dvar=b["dvar"].astype(F32))
        close(tag + "/dy_out", t.dy.read(), b["dy_out"])
        close(tag + "/dx", t.dx.read(), b["dy_out"])
    elif entry == "forward_stats":
        t = run_forward(L, p, TRAIN, stats=image_partials(x64, x64 * x64))
        check_forward(tag, p, t, TRAIN, R.ACT_NONE, exact=False)
    elif entry == "stats_only":
        check_stats(tag, p, run_stats_only(L, p, image_partials(x64, x64 * x64)), exact=False)
    else:
        g = p.dy.astype(F64)
        sums = R.Guarded(image_partials(g, g * (x64 - B.chan(p.mean, p.c, F64))))
        t = backward_buffers(p, None)
        L.bcnn_hip_batchnorm_backward_finalize(sums.ptr, p.n, t.scales.ptr, t.dscales.ptr, t.db.ptr, t.var.ptr, t.dmean.ptr,
                                               t.dvar.ptr, p.c)
        L.bcnn_hip_sync()
        check_backward(tag, p, t, exact=False, sums_only=True)


# ---- determinism: two calls on the same buffers give identical bits -------------------------------------------------------------
def test_forward_is_deterministic(L):
    p = B.uniform_inputs(*REAL_SHAPE)
    outs = []
    t = None
    for _ in range(2):
        if t is None:
            t = run_forward(L, p, TRAIN, R.ACT_RELU)
        else:                                    # the same device buffers again; the running statistics are in / out
            t.run_mean, t.run_var = R.Guarded(p.run_mean0), R.Guarded(p.run_var0)
            L.bcnn_hip_batchnorm_forward(t.x.ptr, t.y.ptr, t.run_mean.ptr, t.run_var.ptr, t.scales.ptr, t.bias.ptr,
                                         t.saved_mean.ptr, t.saved_var.ptr, t.xn.ptr, t.ws.ptr, p.n, p.c, p.hw, TRAIN, R.ACT_RELU)
            L.bcnn_hip_sync()
        outs.append([getattr(t, k).read() for k in ("y", "xn", "ws", "saved_mean", "saved_var", "run_mean", "run_var")])
    for a, b in zip(*outs):
        R.assert_bits("forward twice", a, b)


def test_backward_is_deterministic(L):
    p = B.uniform_inputs(*REAL_SHAPE)
    outs = []
    t = run_backward(L, p)
    outs.append([getattr(t, k).read() for k in ("dy", "dx", "db", "dscales", "dmean", "dvar")])
    t.dy, t.dscales, t.db = R.Guarded(p.dy), R.Guarded(p.dscales0), R.Guarded(p.dbias0)     # the in / out tensors
    L.bcnn_hip_batchnorm_backward(t.dy.ptr, t.dx.ptr, None, R.ACT_NONE, t.scales.ptr, t.dscales.ptr, t.db.ptr, t.mean.ptr,
                                  t.var.ptr, t.dmean.ptr, t.dvar.ptr, None, t.x.ptr, p.n, p.c, p.hw)
    L.bcnn_hip_sync()
    outs.append([getattr(t, k).read() for k in ("dy", "dx", "db", "dscales", "dmean", "dvar")])
    for a, b in zip(*outs):
        R.assert_bits("backward twice", a, b)


def test_wide_finalize_is_deterministic(L):
    p = B.uniform_inputs(*REAL_SHAPE)
    splits = 3073
    sums = R.Guarded(np.random.RandomState(5).uniform(-1, 1, (p.c, splits, 2)).astype(F32))
    outs = []
    for _ in range(2):
        t = backward_buffers(p, None)
        L.bcnn_hip_batchnorm_backward_finalize(sums.ptr, splits, t.scales.ptr, t.dscales.ptr, t.db.ptr, t.var.ptr,
                                               t.dmean.ptr, t.dvar.ptr, p.c)
        L.bcnn_hip_sync()
        outs.append([getattr(t, k).read() for k in ("db", "dscales", "dmean", "dvar")])
    for a, b in zip(*outs):
        R.assert_bits("finalize twice", a, b)
