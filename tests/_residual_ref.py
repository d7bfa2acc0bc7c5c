"""Plain restatements of the residual block's conv node: convolution + batch-norm (no activation) whose output is the first
operand of the eltwise node behind it (bcnn_conv_layer.c:367-485 then bcnn_eltwise_layer.c:82-113; backward
bcnn_eltwise_layer.c:115-152 then bcnn_conv_layer.c:487-587), for tests/test_conv_residual.py. TEST INFRASTRUCTURE ONLY.

  forward   raw = conv(x, w)                         no bias: the batch-norm follows
            TRAIN-mode statistics of raw, running statistics moved      (_bn_ref.forward64, 1e-6 divisor)
            v = bn(raw); v[:rc] += res[:rc]          rc = min(res_count, total): the reference adds its second operand to
            out = act(v)                             the first res_count FLAT elements only
  backward  g = dout * act'(out)                     act' from the POST-activation value (_next_ref.act_factor*)
            dres[:rc] += g[:rc]
            batch-norm backward of g                 (_bn_ref.backward64, its own 1e-5 divisor): dscales, dbias accumulate,
                                                     dmean, dvar, dy
            dw += dW(x, dy); dx = dX(w, dy)          dx overwritten; a 1x1 kernel reads / writes the raw [c][oh * ow] prefix
                                                     of each image whatever stride and pad say (bcnn_conv_layer.c:445-446)

Two forms: chain64 (float64, what the bars are measured against) and chain32 (float32, one rounding per operation with the
*32 helpers of _bn_ref.py; the sums combined in double as the kernels do). chain32 is held to chain64 under the project's bar
on the CPU (test_conv_residual.py::test_float32_restatement_meets_the_bar): the bar is reachable by float32 arithmetic alone
at every shape used.

The inputs are drawn so that the tests bite (preconditions(), asserted on the CPU): the second operand is as large as the
batch-norm output, so act' of act(bn + res) differs from act' of act(bn) inside [0, rc), in the last four elements before rc
and in the first four behind it; adding res changes the value of out[rc - 1] and would change that of out[rc] (an off-by-one
in either direction shows in the forward output); and no pre-activation value lies so close to a kink of act' that an
implementation inside the forward bar could land on the other side of it. SEEDS holds, per shape, the first seed whose draw passes for every
(res_count, activation) the tests run (find_seed() is how they were found)."""
import functools
import types

import numpy as np

from tests import _bn_ref as B
from tests import _next_ref as R

F32, F64 = np.float32, np.float64

# id -> (n, c, h, w), f, k, stride, pad
SHAPES = {
    "A": ((2, 3, 8, 8), 8, 3, 1, 1),
    "B": ((2, 4, 7, 7), 3, 3, 1, 1),
    "C": ((4, 2, 5, 5), 6, 1, 1, 0),
    "D": ((2, 4, 8, 8), 8, 1, 2, 0),
    "E": ((1, 3, 32, 32), 4, 3, 1, 1),
    "F": ((2, 2, 65, 64), 3, 3, 1, 1),
}
CHEAP_ACTS = [R.ACT_NONE, R.ACT_RELU, R.ACT_RAMP, R.ACT_LRELU, R.ACT_ABS, R.ACT_CLAMP]
MASK_ACTS = (R.ACT_RELU, R.ACT_LRELU, R.ACT_CLAMP)      # the preconditions on the act' mask are asserted for these
KINKS = {R.ACT_RELU: (0.0,), R.ACT_LRELU: (0.0,), R.ACT_RAMP: (0.0,), R.ACT_CLAMP: (0.0, 1.0)}   # where act' jumps
# (shape, res_count, activation): every case of the op tests
RC = {"A": [512, 320, 511, 510, 509, 0, 1024, 1031], "B": [147, 98], "C": [150, 75], "D": [128], "E": [4096, 2048],
      "F": [12480, 8257]}
CASES = [(s, rc, R.ACT_RELU) for s in "ABCDEF" for rc in RC[s]]
CASES += [("A", rc, a) for rc in (512, 510) for a in CHEAP_ACTS if a != R.ACT_RELU]
CASES += [("B", rc, a) for rc in RC["B"] for a in CHEAP_ACTS if a != R.ACT_RELU]
SEEDS = {"A": 537, "B": 8, "C": 6, "D": 1, "E": 5, "F": 51}
# an element whose pre-activation value is nearer to a kink than the forward bar allows an implementation to be off
# (tests._golden: 1e-5 of the tensor's largest magnitude for values near zero) may take either side of it
KINK_MARGIN = 1e-5


def case_id(case):
    return "%s-rc%d-%s" % (case[0], case[1], R.ACT_NAMES[case[2]])


def geometry(shape):
    (n, c, h, w), f, k, s, p = SHAPES[shape]
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return types.SimpleNamespace(n=n, c=c, h=h, w=w, f=f, k=k, s=s, p=p, oh=oh, ow=ow, hw=oh * ow, M=n * oh * ow,
                                 total=n * f * oh * ow)


@functools.lru_cache(maxsize=None)
def inputs(shape, seed=None):
    """the tensors of one shape (shared between tests, read-only): scales in [0.5, 1.5], res uniform in [-2, 2]; what the
    calls accumulate into (dw, dscales, dbias, dres) starts from finite garbage"""
    g = geometry(shape)
    rs = np.random.RandomState(1000 * (ord(shape) - 64) + (SEEDS[shape] if seed is None else seed))
    p = types.SimpleNamespace(shape=shape, g=g)
    p.x = rs.uniform(-1, 1, (g.n, g.c, g.h, g.w)).astype(F32)
    p.w = rs.uniform(-1, 1, (g.f, g.c, g.k, g.k)).astype(F32)
    p.scales = rs.uniform(0.5, 1.5, g.f).astype(F32)
    p.bias = rs.uniform(-0.5, 0.5, g.f).astype(F32)
    p.run_mean0 = rs.uniform(-0.2, 0.2, g.f).astype(F32)
    p.run_var0 = rs.uniform(0.8, 1.2, g.f).astype(F32)
    p.res = rs.uniform(-2, 2, g.total).astype(F32)
    p.dout = rs.uniform(-1, 1, g.total).astype(F32)
    p.dres0 = rs.uniform(-3, 3, g.total).astype(F32)
    p.dw0 = rs.uniform(-1, 1, p.w.shape).astype(F32)
    p.dscales0 = rs.uniform(-3, 3, g.f).astype(F32)
    p.dbias0 = rs.uniform(-3, 3, g.f).astype(F32)
    assert not np.any((p.scales == 0) | (p.scales == 1) | (p.bias == 0) | (p.bias == 1))   # the quirk channels: _bn_ref's tests
    for v in vars(p).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


# ---- the convolution, in the precision of its arguments ------------------------------------------------------------------------
def _t(a, dtype):
    import torch
    return torch.from_numpy(np.array(a, dtype))      # a copy: the shared inputs are read-only


def conv(x, w, g, dtype):
    """(n, f, hw) raw convolution output"""
    import torch
    if g.k == 1:
        xr = np.asarray(x, dtype).reshape(g.n, -1)[:, :g.c * g.hw].reshape(g.n, g.c, g.hw)
        return np.einsum("fc,ncq->nfq", np.asarray(w, dtype).reshape(g.f, g.c), xr).astype(dtype)
    y = torch.nn.functional.conv2d(_t(x, dtype), _t(w, dtype), stride=g.s, padding=g.p)
    return y.numpy().reshape(g.n, g.f, g.hw)


def conv_grads(x, w, dy, g, dtype):
    """(dW, dX, prefix): dX is (n, c * h * w); prefix: how many elements per image it defines (1x1: the raw view), else all"""
    import torch
    dy = np.asarray(dy, dtype).reshape(g.n, g.f, g.hw)
    if g.k == 1:
        xr = np.asarray(x, dtype).reshape(g.n, -1)[:, :g.c * g.hw].reshape(g.n, g.c, g.hw)
        dw = np.einsum("nfq,ncq->fc", dy, xr).astype(dtype).reshape(g.f, g.c, 1, 1)
        dx = np.einsum("fc,nfq->ncq", np.asarray(w, dtype).reshape(g.f, g.c), dy).astype(dtype).reshape(g.n, g.c * g.hw)
        return dw, dx, g.c * g.hw
    x_t, w_t, dy_t = _t(x, dtype), _t(w, dtype), _t(dy.reshape(g.n, g.f, g.oh, g.ow), dtype)
    dw = torch.nn.grad.conv2d_weight(x_t, w_t.shape, dy_t, stride=g.s, padding=g.p).numpy()
    dx = torch.nn.grad.conv2d_input(x_t.shape, w_t, dy_t, stride=g.s, padding=g.p).numpy()
    return dw, dx.reshape(g.n, -1), g.c * g.h * g.w


FWD_KEYS = ("out", "saved_mean", "saved_var", "run_mean", "run_var", "bn_workspace")
BWD_KEYS = ("dres", "dscales", "dbias", "dmean", "dvar", "dy", "dw", "dx")


# ---- float64 ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bn64(shape, seed=None):
    """what does not depend on (res_count, act): the convolution and the batch-norm forward in float64"""
    p = inputs(shape, seed)
    raw = conv(p.x, p.w, p.g, F64)
    f = B.forward64(raw, p.run_mean0, p.run_var0, p.scales, p.bias, B.MODE_TRAIN)
    return raw, f


@functools.lru_cache(maxsize=None)
def chain64(shape, rc, act, seed=None):
    """every output of the forward and the backward pass, float64 (`pre`: bn(raw) before the residual add; `v`: the argument
    of the activation; `g`: the gradient behind the activation backward). Cached and shared: never modify."""
    p = inputs(shape, seed)
    g = p.g
    rcc = min(rc, g.total)
    raw, f = _bn64(shape, seed)
    e = {k: f[k] for k in ("saved_mean", "saved_var", "run_mean", "run_var")}
    e["bn_workspace"] = raw
    e["pre"] = f["pre"].ravel()
    v = e["pre"].copy()
    v[:rcc] += p.res[:rcc].astype(F64)
    e["v"] = v
    e["out"] = R.act_forward64(v.astype(F32), act)
    gg = p.dout.astype(F64) * R.act_factor64(e["out"], act)
    e["g"] = gg
    e["dres"] = p.dres0.astype(F64)
    e["dres"][:rcc] += gg[:rcc]
    b = B.backward64(gg.reshape(g.n, g.f, g.hw), raw, p.scales, e["saved_mean"], e["saved_var"], p.dscales0, p.dbias0)
    e["dscales"], e["dbias"], e["dmean"], e["dvar"], e["dy"] = b["dscales"], b["db"], b["dmean"], b["dvar"], b["dy_out"]
    dw, dx, e["dx_prefix"] = conv_grads(p.x, p.w, e["dy"], g, F64)
    e["dw"], e["dx"] = p.dw0.astype(F64) + dw, dx
    return e


# ---- float32, one rounding per operation ------------------------------------------------------------------------------------
def chain32(shape, rc, act, seed=None):
    p = inputs(shape, seed)
    g = p.g
    rcc = min(rc, g.total)
    raw = conv(p.x, p.w, g, F32)
    r64 = raw.astype(F64)
    e = {"bn_workspace": raw}
    e["saved_mean"], e["saved_var"], e["run_mean"], e["run_var"] = B.stats_finalize32(
        r64.sum(axis=(0, 2)), (r64 * r64).sum(axis=(0, 2)), g.M, p.run_mean0, p.run_var0)
    pre = B.affine32(B.normalize32(raw, e["saved_mean"], e["saved_var"]), p.scales, p.bias).ravel()
    e["out"] = R.act_forward32(R.eltwise_sum32(pre, p.res, rcc), act)
    gg = B.act_grad32(p.dout, e["out"], act)
    e["dres"] = p.dres0.copy()
    e["dres"][:rcc] = p.dres0[:rcc] + gg[:rcc]
    g3 = gg.reshape(g.n, g.f, g.hw)
    d32 = (raw - B.chan(e["saved_mean"], g.f)).astype(F32)
    S1, S2 = B.channel_sums(g3, g.n, g.f, g.hw), B.channel_sums((g3 * d32).astype(F32), g.n, g.f, g.hw)
    e["dbias"], e["dscales"], e["dmean"], e["dvar"] = B.bwd_finalize32(S1, S2, p.scales, e["saved_var"], p.dscales0, p.dbias0)
    e["dy"] = B.bwd_apply32(g3, raw, e["saved_mean"], e["saved_var"], p.scales, e["dmean"], e["dvar"], g.M)
    dw, dx, e["dx_prefix"] = conv_grads(p.x, p.w, e["dy"], g, F32)
    e["dw"], e["dx"] = (p.dw0 + dw).astype(F32), dx
    return e


# ---- what makes the tests bite -----------------------------------------------------------------------------------------------
def _mask(v, act):
    """act' taken from act(v), v rounded to float32 as the kernels hold it"""
    return R.act_factor64(R.act_forward64(np.asarray(v, F64).astype(F32), act), act)


def preconditions(shape, rc, act, seed=None):
    """the reasons (strings) why this draw would let a wrong kernel pass; empty: the draw is good"""
    p = inputs(shape, seed)
    e = chain64(shape, rc, act, seed)
    total, rcc = p.g.total, min(rc, p.g.total)
    bad = []
    for kink in KINKS.get(act, ()):
        near = np.abs(e["v"] - kink).min()
        if near <= KINK_MARGIN * np.abs(e["v"]).max():
            bad.append("an element %.3g from the kink of act' at %g" % (near, kink))
    with_res = e["pre"] + p.res.astype(F64)
    value = lambda v: R.act_forward64(np.asarray(v, F64).astype(F32), act)
    # a sweep that stops one element short of rc, or runs one element past it, changes `out` there (not two values that the
    # activation maps to the same number)
    if rcc > 0 and value(with_res[rcc - 1]) == value(e["pre"][rcc - 1]):
        bad.append("out[rc - 1] does not depend on res")
    if rcc < total and value(with_res[rcc]) == value(e["pre"][rcc]):
        bad.append("out[rc] would not change if res were added there")
    if act not in MASK_ACTS:
        return bad
    differs = _mask(with_res, act) != _mask(e["pre"], act)      # would adding res here change act'?
    if rcc > 0:
        if not differs[:rcc].any():
            bad.append("no element of [0, rc) whose act' depends on res")
        if not differs[max(0, rcc - 4):rcc].any():
            bad.append("none of the last four elements before rc has an act' that depends on res")
    if rcc < total and not differs[rcc:min(rcc + 4, total)].any():
        bad.append("none of the four elements behind rc would change its act' if res were added there")
    return bad


def find_seed(shape, limit=2000):
    """the first seed whose draw passes preconditions() for every case of this shape (how SEEDS was filled)"""
    for seed in range(limit):
        if not any(preconditions(s, rc, act, seed) for s, rc, act in CASES if s == shape):
            return seed
    raise AssertionError("no seed below %d for shape %s" % (limit, shape))
