"""The dilated depthwise kernels (bcnn_hip_dilated_depthwise_forward / _backward, depthwise_dilated.hip; DESIGN.md section
29) through bcnn_amd.ops, against torch.nn.functional.conv2d(groups = c, dilation = d) on the CPU in float64 with autograd
for the gradients: the harness of tests/test_dilated_conv.py, restated.

The bar is element-wise OP_TOL * max |reference| of the tensor, the project's bar for a stand-alone op. torch's own float32
conv2d and autograd on the CPU stay inside it on every case below: the worst ratio of its error to the bar is 0.50 (dw of
the 131 x 257 plane, a sum of 33667 products; db 0.19, y 0.021, dx 0.016 and dy act'(y) 0.006 at their worst). On small-integer inputs every partial
sum is an integer below 2^24 and the results must equal the float64 ones bit for bit, whatever the band or plane split.

At dilation 1 the forward and the data gradient carry the bits of bcnn_hip_depthwise_forward / _backward (the rounding
rule of the file's header); the case list reaches every value bcnn_hip_dilated_depthwise_path defines, in both
directions, and both sides of each of its thresholds."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = {"none": 0, "relu": 2, "lrelu": 5, "logistic": 9}
OP_TOL = 1e-5      # element-wise, times max |reference| of the tensor
GUARD = 256

# (n, c, h, w, k, s, p, d)
CASES = [
    (2, 3, 7, 9, 3, 1, 2, 2),        # H != W, odd width: no 16-byte rows
    (1, 4, 5, 5, 3, 1, 7, 7),        # dilation larger than the plane: only the centre tap lands
    (2, 5, 33, 33, 3, 1, 6, 6),      # the ASPP plane
    (2, 3, 9, 9, 3, 1, 1, 3),        # pad < dilation: the output shrinks
    (1, 2, 6, 6, 3, 1, 5, 2),        # pad > dilation: the output is larger than the input, rows no tap of x reaches
    (2, 6, 11, 10, 3, 2, 2, 2),      # stride 2, even d: one tap parity per pixel
    (1, 3, 12, 13, 3, 2, 3, 3),      # stride 2, odd d
    (1, 2, 9, 9, 3, 3, 4, 4),        # stride 3
    (2, 4, 8, 8, 2, 1, 1, 2),        # even kernel
    (1, 3, 10, 10, 5, 1, 4, 2),      # 5x5
    (2, 17, 6, 6, 1, 1, 0, 3),       # k = 1
    (3, 70, 4, 4, 3, 1, 2, 2),       # more channels than a wave has lanes, tiny planes
    (9, 3, 5, 5, 3, 1, 2, 2),        # a ragged cross-image reduction
    (1, 2, 150, 260, 3, 1, 2, 2),    # planes no LDS path holds whole: bands and their halo
    (1, 1, 131, 257, 3, 1, 4, 4),
]
# either side of every threshold of bcnn_hip_dilated_depthwise_path: (forward path, backward path)
THRESHOLDS = {
    (1, 1, 96, 128, 3, 1, 2, 2): (1, 1),     # 12288 floats: the largest whole plane
    (1, 1, 97, 128, 3, 1, 2, 2): (2, 2),     # one row more: bands
    (1, 1, 100, 120, 3, 1, 6, 2): (1, 2),    # x fits (12000), the larger dy plane (108 x 128) does not
    (1, 1, 82, 151, 3, 1, 40, 40): (2, 2),   # 81 rows of 151 fit: bands of one row beside an 80-row halo
    (1, 1, 82, 152, 3, 1, 40, 40): (0, 0),   # 80 rows of 152: no band fits, the generic kernels
}
ALL_CASES = CASES + list(THRESHOLDS)
BANDED = CASES[13]
INT_CASES = [CASES[0], CASES[5], BANDED]
GRID = ([(c, a) for c in ALL_CASES for a in ("none", "relu")] +
        [(CASES[2], "lrelu"), (CASES[6], "lrelu"), (BANDED, "lrelu"), (CASES[0], "logistic"), (CASES[5], "logistic"),
         (CASES[14], "logistic")])
_ids = lambda v: v if isinstance(v, str) else "-".join(map(str, v))  # noqa: E731


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


def _out_hw(case):
    n, c, h, w, k, s, p, d = case
    return (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1


@functools.lru_cache(maxsize=None)
def _inputs(case, seed, integer):
    """host inputs of a case (float32; read-only: shared between tests)"""
    n, c, h, w, k, s, p, d = case
    rs = np.random.RandomState(seed)
    oh, ow = _out_hw(case)
    if integer:
        draw = lambda lo, hi, shape: rs.randint(-3, 4, shape).astype(np.float32)  # noqa: E731
    else:
        draw = lambda lo, hi, shape: rs.uniform(lo, hi, shape).astype(np.float32)  # noqa: E731
    inp = dict(x=draw(-1, 1, (n, c, h, w)), wt=draw(-0.5, 0.5, (c, 1, k, k)), b=draw(-0.5, 0.5, (c,)),
               dy=draw(-1, 1, (n, c, oh, ow)), dw0=draw(-0.1, 0.1, (c, 1, k, k)), db0=draw(-0.1, 0.1, (c,)),
               dx0=draw(-1, 1, (n, c, h, w)))
    for v in inp.values():
        v.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def _conv64(case, seed, integer):
    """the float64 pre-activation output of torch's conv2d on the CPU (computed once per case)"""
    n, c, h, w, k, s, p, d = case
    inp = _inputs(case, seed, integer)
    z = torch.nn.functional.conv2d(torch.tensor(inp["x"], dtype=torch.float64), torch.tensor(inp["wt"], dtype=torch.float64),
                                   torch.tensor(inp["b"], dtype=torch.float64), stride=s, padding=p, dilation=d, groups=c)
    z = z.numpy()
    z.setflags(write=False)
    return z


def _grads(case, seed, integer, gout, dtype=torch.float64):
    """(dW, dx) of torch's conv2d for the output gradient gout, by autograd"""
    n, c, h, w, k, s, p, d = case
    inp = _inputs(case, seed, integer)
    x = torch.tensor(inp["x"], dtype=dtype, requires_grad=True)
    wt = torch.tensor(inp["wt"], dtype=dtype, requires_grad=True)
    z = torch.nn.functional.conv2d(x, wt, None, stride=s, padding=p, dilation=d, groups=c)
    z.backward(torch.tensor(np.asarray(gout), dtype=dtype))
    return wt.grad.numpy(), x.grad.numpy()


def _guarded(shape, guard, fill=float("nan")):
    """a device tensor of `shape` filled with `fill`; with guard > 0 inside a larger one with sentinels on both sides"""
    numel = int(np.prod(shape))
    if not guard:
        return torch.full(shape, fill, device="cuda"), None
    big = torch.full((numel + 2 * guard,), 12345.0, device="cuda")
    inner = big[guard:guard + numel].view(shape)
    inner.fill_(fill)
    return inner, big


def _run(case, act, seed=0, integer=False, dx="overwrite", guard=0):
    """one forward + backward on the device; returns every result (numpy float32) and the guard-band tensors.
    dx: "overwrite" (overwrite = 1 into NaNs), "zeros" (overwrite = 0 onto zeros), "add" (overwrite = 0 onto dx0), None."""
    from bcnn_amd import ops
    n, c, h, w, k, s, p, d = case
    inp = _inputs(case, seed, integer)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    tx, tw, tb = map(dev, (inp["x"], inp["wt"], inp["b"]))
    ty, ybig = _guarded(inp["dy"].shape, guard)
    tdy, dybig = _guarded(inp["dy"].shape, guard)
    tdy.copy_(dev(inp["dy"]))
    tdx, dxbig = (None, None)
    if dx is not None:
        tdx, dxbig = _guarded(inp["x"].shape, guard, float("nan") if dx == "overwrite" else 0.0)
        if dx == "add":
            tdx.copy_(dev(inp["dx0"]))
    tdw, dwbig = _guarded(inp["wt"].shape, guard)
    tdw.copy_(dev(inp["dw0"]))
    tdb, dbbig = _guarded(inp["b"].shape, guard)
    tdb.copy_(dev(inp["db0"]))
    # exactly the size the query names, full of NaNs: every partial the finalize kernel reads has been written
    ws = torch.full((ops.dilated_depthwise_workspace_size(*case),), float("nan"), device="cuda")
    ops.dilated_depthwise_forward(tx, tw, tb, ty, k, s, p, d, act)
    y = ty.cpu().numpy()
    ops.dilated_depthwise_backward(tx, tw, ty, tdy, tdx, tdw, tdb, k, s, p, d, act, dx == "overwrite", ws)
    torch.cuda.synchronize()
    got = dict(y=y, g=tdy.cpu().numpy(), dw=tdw.cpu().numpy(), db=tdb.cpu().numpy(),
               dx=tdx.cpu().numpy() if dx is not None else None)
    bands = [b.cpu().numpy() for b in (ybig, dybig, dxbig, dwbig, dbbig) if b is not None]
    return got, bands


def _check(case, act, got, seed=0, integer=False, exact=False, dx="overwrite"):
    inp = _inputs(case, seed, integer)
    cmp = (lambda tag, a, b: np.testing.assert_array_equal(np.asarray(a, np.float64), b, err_msg=tag)) if exact else _close
    y_ref = _act(_conv64(case, seed, integer), act)
    cmp("y", got["y"], y_ref)
    # the activation backward is evaluated at the output the forward wrote
    g_ref = inp["dy"].astype(np.float64) * _act_grad(got["y"].astype(np.float64), act)
    cmp("dy * act'(y)", got["g"], g_ref)
    dw_ref, dx_ref = _grads(case, seed, integer, g_ref)
    cmp("dw", got["dw"], inp["dw0"].astype(np.float64) + dw_ref)
    cmp("db", got["db"], inp["db0"].astype(np.float64) + g_ref.sum(axis=(0, 2, 3)))
    if dx is not None:
        cmp("dx", got["dx"], dx_ref + (inp["dx0"].astype(np.float64) if dx == "add" else 0.0))


@pytest.mark.parametrize("case,act", GRID, ids=_ids)
def test_ops_match_torch_float64(case, act):
    got, _ = _run(case, ACTS[act])
    _check(case, ACTS[act], got)
    # without a data gradient nothing else changes
    nodx, _ = _run(case, ACTS[act], dx=None)
    for key in ("y", "g", "dw", "db"):
        assert np.array_equal(got[key], nodx[key]), key
    # assigning into NaNs is accumulating onto zeros
    zeros, _ = _run(case, ACTS[act], dx="zeros")
    for key in ("y", "g", "dw", "db", "dx"):
        assert np.array_equal(got[key], zeros[key]), key


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[5], CASES[9], BANDED, (1, 1, 82, 152, 3, 1, 40, 40)], ids=_ids)
def test_data_gradient_accumulates_without_overwrite(case):
    got, _ = _run(case, ACTS["relu"], dx="add")
    _check(case, ACTS["relu"], got, dx="add")


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("case", INT_CASES, ids=_ids)
def test_exact_on_small_integers(case, act):
    for dx in ("overwrite", "add"):
        got, _ = _run(case, ACTS[act], seed=5, integer=True, dx=dx)
        _check(case, ACTS[act], got, seed=5, integer=True, exact=True, dx=dx)


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("case", [(2, 5, 14, 14, 3, 1, 1, 1), (2, 3, 9, 11, 3, 2, 1, 1), (1, 70, 7, 7, 3, 1, 1, 1)], ids=_ids)
def test_dilation_one_has_the_bits_of_the_depthwise_entry_points(case, act):
    from bcnn_amd import ops
    n, c, h, w, k, s, p, d = case
    inp = _inputs(case, 11, False)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    for mode in ("overwrite", "add"):
        got, _ = _run(case, ACTS[act], seed=11, dx=mode)
        tx, tw, tb, tdy, tdw, tdb = map(dev, (inp["x"], inp["wt"], inp["b"], inp["dy"], inp["dw0"], inp["db0"]))
        ty = torch.full(inp["dy"].shape, float("nan"), device="cuda")
        tdx = torch.full(inp["x"].shape, float("nan"), device="cuda") if mode == "overwrite" else dev(inp["dx0"])
        ops.depthwise_forward(tx, tw, tb, ty, k, s, p, ACTS[act])
        ops.depthwise_backward(tx, tw, ty, tdy, tdx, tdw, tdb, k, s, p, ACTS[act], overwrite=mode == "overwrite")
        torch.cuda.synchronize()
        assert np.array_equal(got["y"], ty.cpu().numpy())
        assert np.array_equal(got["g"], tdy.cpu().numpy())
        assert np.array_equal(got["dx"], tdx.cpu().numpy()), mode
        _close("dw", got["dw"], tdw.cpu().numpy())
        _close("db", got["db"], tdb.cpu().numpy())


@pytest.mark.parametrize("case", [CASES[2], CASES[5]], ids=_ids)
def test_agrees_with_the_dilated_convolution_kernels_at_groups_c(case):
    """the same weights buffer is [c][k][k] here and [c][1][k][k] there"""
    from bcnn_amd import ops
    n, c, h, w, k, s, p, d = case
    inp = _inputs(case, 7, False)
    got, _ = _run(case, ACTS["none"], seed=7)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    tx, tw, tb, tdy, tdw, tdb = map(dev, (inp["x"], inp["wt"], inp["b"], inp["dy"], inp["dw0"], inp["db0"]))
    ty = torch.full(inp["dy"].shape, float("nan"), device="cuda")
    tdx = torch.full(inp["x"].shape, float("nan"), device="cuda")
    ws = torch.zeros(ops.dilated_conv_workspace_size(n, c, h, w, c, k, s, p, d, c), device="cuda")
    ops.dilated_conv_forward(tx, tw, tb, ty, k, s, p, d, c, ACTS["none"])
    ops.dilated_conv_backward(tx, tw, ty, tdy, tdx, tdw, tdb, k, s, p, d, c, ACTS["none"], ws)
    torch.cuda.synchronize()
    _close("y", got["y"], ty.cpu().numpy())
    _close("dy", got["g"], tdy.cpu().numpy())
    _close("dx", got["dx"], tdx.cpu().numpy())
    _close("dw", got["dw"], tdw.cpu().numpy())
    _close("db", got["db"], tdb.cpu().numpy())


@pytest.mark.parametrize("case", [CASES[11], CASES[12], BANDED, CASES[6]], ids=_ids)
def test_two_runs_give_the_same_bits(case):
    runs = [_run(case, ACTS["relu"], seed=3)[0] for _ in range(2)]
    for key in ("y", "g", "dw", "db", "dx"):
        assert np.array_equal(runs[0][key], runs[1][key]), key
    _check(case, ACTS["relu"], runs[0], seed=3)


@pytest.mark.parametrize("case", [CASES[0], CASES[9], BANDED, CASES[4]], ids=_ids)
def test_neighbours_are_untouched(case):
    got, bands = _run(case, ACTS["relu"], guard=GUARD)
    _check(case, ACTS["relu"], got)
    assert len(bands) == 5
    for b in bands:
        assert (b[:GUARD] == 12345.0).all() and (b[-GUARD:] == 12345.0).all()


def test_the_cases_reach_every_path_and_both_sides_of_every_threshold():
    from bcnn_amd import ops
    assert len(ops.DILATED_DEPTHWISE_PATHS) == 3
    for backward in (False, True):
        paths = {ops.dilated_depthwise_path(*case, backward=backward) for case in ALL_CASES}
        assert paths == {0, 1, 2}, (backward, paths)
    for case, (fwd, bwd) in THRESHOLDS.items():
        assert ops.dilated_depthwise_path(*case, backward=False) == fwd, case
        assert ops.dilated_depthwise_path(*case, backward=True) == bwd, case
    assert ops.dilated_depthwise_path(*BANDED) == 2 and ops.dilated_depthwise_path(*CASES[14], backward=True) == 2
    assert ops.dilated_depthwise_path(*CASES[5]) == 0 and ops.dilated_depthwise_path(*CASES[9], backward=True) == 0
