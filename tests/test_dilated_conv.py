"""The dilated-convolution kernels (bcnn_hip_dilated_conv_forward / _backward, conv_dilated.hip)
through bcnn_amd.ops, against torch.nn.functional.conv2d on the CPU in float64 with autograd for the gradients (the
reference project has no dilation: the same second-opinion use of torch that tests/test_deconv.py makes).

The bar is element-wise OP_TOL * max |reference| of the tensor, tests/test_deconv.py's bar for a stand-alone matrix-core
op: torch's own float32 results stay within 5.9e-7 of float64 on that measure over these shapes, so the bar leaves the fp32
formula about 17x room. On small-integer inputs every partial sum is an integer far below 2^24 and the results must equal
the float64 ones bit for bit, whatever the split or tile order."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = {"none": 0, "relu": 2, "lrelu": 5, "logistic": 9}
OP_TOL = 1e-5      # element-wise, times max |reference| of the tensor

# (n, c, h, w, f, k, s, p, d, g)
CASES = [
    (2, 3, 7, 9, 5, 3, 1, 2, 2, 1),      # H != W, few channels
    (1, 4, 5, 5, 6, 3, 1, 7, 7, 2),      # dilation larger than the plane: only the centre tap ever lands inside; groups
    (2, 20, 9, 8, 34, 3, 1, 3, 3, 1),    # C not a multiple of the K step; F straddles a tile
    (2, 6, 11, 10, 9, 3, 2, 2, 2, 3),    # stride 2 with even dilation: one parity of tap for every pixel; groups of 3
    (1, 5, 12, 13, 4, 3, 2, 3, 3, 1),    # stride 2 with odd dilation
    (2, 4, 8, 8, 4, 2, 1, 1, 2, 1),      # even kernel
    (1, 3, 10, 10, 70, 5, 1, 4, 2, 1),   # 5x5, F > 64
    (3, 40, 20, 20, 8, 3, 1, 4, 4, 1),   # several dW splits with a ragged last one, C > 32
    (2, 17, 6, 6, 3, 1, 1, 0, 3, 1),     # k = 1, where dilation is irrelevant
    (1, 2, 9, 9, 2, 3, 3, 4, 4, 2),      # stride 3, 3x3 output
    (2, 8, 33, 33, 16, 3, 1, 6, 6, 1),   # an ASPP-like plane
]
INT_CASES = [CASES[2], CASES[3]]
GRID = [(c, a) for c in CASES for a in ("none", "relu")] + [(CASES[2], "lrelu"), (CASES[4], "lrelu"),
                                                            (CASES[0], "logistic"), (CASES[3], "logistic")]


def _act(v, act):
    if act == ACTS["relu"]:
        return v * (v > 0)
    if act == ACTS["lrelu"]:
        return np.where(v > 0, v, 0.1 * v)
    if act == ACTS["logistic"]:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def _act_grad(y, act):
    if act == ACTS["relu"]:
        return (y > 0).astype(np.float64)
    if act == ACTS["lrelu"]:
        return np.where(y > 0, 1.0, 0.1)
    if act == ACTS["logistic"]:
        return (1 - y) * y
    return np.ones_like(y)


def _close(tag, got, want, tol=OP_TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), tag
    bound = tol * max(float(np.abs(want).max()), 1e-30)
    diff = float(np.abs(got - want).max())
    print("%s: max abs diff %.3g, bound %.3g" % (tag, diff, bound))
    assert diff <= bound, "%s: max abs diff %.3g > %.3g" % (tag, diff, bound)


@functools.lru_cache(maxsize=None)
def _inputs(case, seed, integer):
    """host inputs of a case (float32; read-only: shared between tests)"""
    from bcnn_amd import ops
    n, c, h, w, f, k, s, p, d, g = case
    rs = np.random.RandomState(seed)
    oh, ow = ops.dilated_conv_out_hw(h, w, k, s, p, d)
    if integer:
        draw = lambda lo, hi, shape: rs.randint(-3, 4, shape).astype(np.float32)  # noqa: E731
    else:
        draw = lambda lo, hi, shape: rs.uniform(lo, hi, shape).astype(np.float32)  # noqa: E731
    inp = dict(x=draw(-1, 1, (n, c, h, w)), wt=draw(-0.5, 0.5, (f, c // g, k, k)), b=draw(-0.5, 0.5, (f,)),
               dy=draw(-1, 1, (n, f, oh, ow)), dw0=draw(-0.1, 0.1, (f, c // g, k, k)), db0=draw(-0.1, 0.1, (f,)))
    for v in inp.values():
        v.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def _conv64(case, seed, integer):
    """the float64 pre-activation output of torch's conv2d on the CPU (computed once per case)"""
    n, c, h, w, f, k, s, p, d, g = case
    inp = _inputs(case, seed, integer)
    z = torch.nn.functional.conv2d(torch.tensor(inp["x"], dtype=torch.float64), torch.tensor(inp["wt"], dtype=torch.float64),
                                   torch.tensor(inp["b"], dtype=torch.float64), stride=s, padding=p, dilation=d, groups=g)
    z = z.numpy()
    z.setflags(write=False)
    return z


def _grads64(case, seed, integer, gout):
    """(dW, dx) of torch's conv2d for the output gradient gout (float64), by autograd"""
    n, c, h, w, f, k, s, p, d, g = case
    inp = _inputs(case, seed, integer)
    x = torch.tensor(inp["x"], dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(inp["wt"], dtype=torch.float64, requires_grad=True)
    z = torch.nn.functional.conv2d(x, wt, None, stride=s, padding=p, dilation=d, groups=g)
    z.backward(torch.tensor(np.asarray(gout, np.float64)))
    return wt.grad.numpy(), x.grad.numpy()


def _guarded(shape, guard):
    """a NaN-filled device tensor of `shape`; with guard > 0 inside a larger one with `guard` sentinels on both sides"""
    numel = int(np.prod(shape))
    if not guard:
        return torch.full(shape, float("nan"), device="cuda"), None
    big = torch.full((numel + 2 * guard,), 12345.0, device="cuda")
    inner = big[guard:guard + numel].view(shape)
    inner.fill_(float("nan"))
    return inner, big


def _run(case, act, seed=0, integer=False, with_dx=True, ws_elems=None, guard=0):
    """one forward + backward on the device; returns every result (numpy float32) and the guard-band tensors"""
    from bcnn_amd import ops
    n, c, h, w, f, k, s, p, d, g = case
    inp = _inputs(case, seed, integer)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    tx, tw, tb, tdy, tdb = map(dev, (inp["x"], inp["wt"], inp["b"], inp["dy"], inp["db0"]))
    ty, ybig = _guarded(inp["dy"].shape, guard)
    tdx, dxbig = _guarded(inp["x"].shape, guard) if with_dx else (None, None)
    tdw, dwbig = _guarded(inp["wt"].shape, guard)
    tdw.copy_(dev(inp["dw0"]))
    full = ops.dilated_conv_workspace_size(n, c, h, w, f, k, s, p, d, g)
    ws = torch.zeros(full if ws_elems is None else ws_elems, device="cuda")
    ops.dilated_conv_forward(tx, tw, tb, ty, k, s, p, d, g, act)
    y = ty.cpu().numpy()
    ops.dilated_conv_backward(tx, tw, ty, tdy, tdx, tdw, tdb, k, s, p, d, g, act, ws)
    torch.cuda.synchronize()
    got = dict(y=y, g=tdy.cpu().numpy(), dw=tdw.cpu().numpy(), db=tdb.cpu().numpy(),
               dx=tdx.cpu().numpy() if with_dx else None)
    bands = [b.cpu().numpy() for b in (ybig, dxbig, dwbig) if b is not None]
    return got, bands


def _check(case, act, got, seed=0, integer=False, exact=False, dx=True):
    inp = _inputs(case, seed, integer)
    cmp = (lambda tag, a, b: np.testing.assert_array_equal(np.asarray(a, np.float64), b, err_msg=tag)) if exact else _close
    y_ref = _act(_conv64(case, seed, integer), act)
    cmp("y", got["y"], y_ref)
    # the activation backward is evaluated at the output the forward wrote
    g_ref = inp["dy"].astype(np.float64) * _act_grad(got["y"].astype(np.float64), act)
    cmp("dy * act'(y)", got["g"], g_ref)
    dw_ref, dx_ref = _grads64(case, seed, integer, g_ref)
    cmp("dw", got["dw"], inp["dw0"].astype(np.float64) + dw_ref)
    cmp("db", got["db"], inp["db0"].astype(np.float64) + g_ref.sum(axis=(0, 2, 3)))
    if dx:
        cmp("dx", got["dx"], dx_ref)


@pytest.mark.parametrize("case,act", GRID, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_ops_match_torch_float64(case, act):
    got, _ = _run(case, ACTS[act])
    _check(case, ACTS[act], got)
    # without a data gradient nothing else changes
    nodx, _ = _run(case, ACTS[act], with_dx=False)
    for key in ("y", "g", "dw", "db"):
        assert np.array_equal(got[key], nodx[key]), key


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("case", INT_CASES, ids=lambda v: "-".join(map(str, v)))
def test_exact_on_small_integers(case, act):
    got, _ = _run(case, ACTS[act], seed=5, integer=True)
    _check(case, ACTS[act], got, seed=5, integer=True, exact=True)


def test_weight_gradient_is_deterministic_and_takes_a_one_split_workspace():
    from bcnn_amd import ops
    case = CASES[7]
    n, c, h, w, f, k, s, p, d, g = case
    per_split = k * k * (c // g) * f
    full = ops.dilated_conv_workspace_size(*case)
    assert full % per_split == 0 and full // per_split > 1   # the full workspace splits K several times
    runs = [_run(case, ACTS["relu"], seed=3)[0] for _ in range(2)]
    for key in ("y", "g", "dw", "db", "dx"):
        assert np.array_equal(runs[0][key], runs[1][key]), key
    one, _ = _run(case, ACTS["relu"], seed=3, ws_elems=per_split)
    _check(case, ACTS["relu"], one, seed=3)


@pytest.mark.parametrize("case", [CASES[2], CASES[3], CASES[6]], ids=lambda v: "-".join(map(str, v)))
def test_neighbours_are_untouched(case):
    guard = 256
    got, bands = _run(case, ACTS["none"], guard=guard)
    _check(case, ACTS["none"], got)
    assert len(bands) == 3
    for b in bands:
        assert (b[:guard] == 12345.0).all() and (b[-guard:] == 12345.0).all()


def test_dilation_one_agrees_with_the_convolution_entry_points():
    from bcnn_amd import ops
    case = (2, 20, 9, 8, 34, 3, 1, 1, 1, 1)
    n, c, h, w, f, k, s, p, d, g = case
    inp = _inputs(case, 11, False)
    got, _ = _run(case, ACTS["none"], seed=11)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    tx, tw, tb, tdy, tdw, tdb = map(dev, (inp["x"], inp["wt"], inp["b"], inp["dy"], inp["dw0"], inp["db0"]))
    ty = torch.full(inp["dy"].shape, float("nan"), device="cuda")
    tdx = torch.full(inp["x"].shape, float("nan"), device="cuda")
    ws = torch.zeros(max(ops.conv_workspace_size(n, c, h, w, f, k, s, p, g), 1), device="cuda")
    ops.conv_forward(tx, tw, tb, ty, k, s, p, g, ACTS["none"])
    ops.conv_backward(tx, tw, ty, tdy, tdx, tdw, tdb, k, s, p, g, ACTS["none"], ws)
    torch.cuda.synchronize()
    _close("y", got["y"], ty.cpu().numpy())
    _close("dy", got["g"], tdy.cpu().numpy())
    _close("dx", got["dx"], tdx.cpu().numpy())
    _close("dw", got["dw"], tdw.cpu().numpy())
    _close("db", got["db"], tdb.cpu().numpy())
