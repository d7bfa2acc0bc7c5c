"""The weight-gradient ladder kDwFamilies (bcnn_amd/csrc/conv.hip), row by row and branch by branch: which family and which
host-chosen sub-branch takes a layer (dispatch trace), and what it computes -- EXACTLY, on small integers.

Every product conv kernel multiplies and accumulates in fp32 (v_mfma_f32_32x32x2f32 / 16x16x4f32, nothing rounds an operand
below fp32), and the Winograd F(2x2,3x3) transforms of conv_winograd.hip (wino_dy_transform_kernel, wino_dw_finish_kernel) and
of the fused weight gradient (wino_dw_fused_kernel, wino_dw_fused_finalize_kernel) use the constants 1, 1/2 and 1/4 only. On
integer inputs whose absolute-value convolutions stay below 2^24 / 64 every partial sum, in any order and under any split
plan, is a float32 number (the factor 64 is the growth of the F(2x2,3x3) input and gradient transforms, 16 x 4, with the two
fractional bits of the 1/4), so the results must EQUAL the float64 reference: no tolerance, and one dropped or doubled term
is a failure. The precondition is asserted on the reference alone, before the comparison.

Reference: torch conv2d in float64 and its autograd on the same integers. Two conventions of the node are restated here and
are not the subject of this file: a bias of exactly 1.0f is not added (bcnn_add_scalar of the reference's AVX build,
bcnn_mat.c:381-383; every forward epilogue reproduces it) and the bias gradient is the plain sum of dy * act'(y).

The expected names come from a port of the families' shape rules at kCUs = 256 (plan_dw_dma, plan_dw_small_c and plan_dw,
all three on split_k of conv_common.h, dw_direct_plan, wino_dw_fused_plan, wino_dw_applicable); the trace assertion is the
check. The rows, stem, direct, large and register-staged rows all end in conv_dw_tiles_finalize (conv_bwd.hip), which writes
no name of its own: only conv_backward_weights names its branch (conv_dw_finalize:4 / :16)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NONE, RELU, PRELU = 0, 2, 8
SENTINEL = -777.25
LIMIT = 2.0 ** 24 / 64

# one name per row of kDwFamilies, in row order (the direct and the register-staged row by their first instantiation)
ROWS = ["conv_dw_rows_kernel", "conv_dw_stem_kernel", "conv_dw_direct_kernel", "wino43_dw_kernel", "wino_dw_fused_kernel",
        "wino_unfused:dw", "conv_dw_dma_kernel", "conv_small_c:dw", "conv_large_dw_kernel", "conv_dw_kernel"]
# every name a weight-gradient launcher writes: families and their host-chosen sub-branches
DW_NAMES = {"conv_dw_rows_kernel", "conv_dw_stem_kernel", "conv_dw_direct_kernel<1>", "conv_dw_direct_kernel<2>",
            "wino43_dw_kernel", "wino_dw_fused_kernel", "wino_unfused:dw", "conv_dw_dma_kernel", "conv_dw_dma_finalize:x4",
            "conv_dw_dma_finalize:16", "conv_dw_dma_finalize:4", "conv_small_c:dw", "conv_large_dw_kernel",
            "conv_dw_kernel<1,1>", "conv_dw_kernel<1,2>", "conv_dw_kernel<2,1>", "conv_dw_kernel<2,2>", "conv_dw_kernel:biascol",
            "conv_dw_finalize:4", "conv_dw_finalize:16", "bnfold:dw"}


def _direct(tm):
    return {"conv_dw_direct_kernel<%d>" % tm}


def _dma(fin):
    return {"conv_dw_dma_kernel", "conv_dw_dma_finalize:" + fin}


def _small_c(fin="4"):
    return {"conv_small_c:dw", "conv_dw_dma_finalize:" + fin}


def _staged(tm, tn, biascol=True, fin="16"):
    return {"conv_dw_kernel<%d,%d>" % (tm, tn), "conv_dw_finalize:" + fin} | ({"conv_dw_kernel:biascol"} if biascol else set())


FUSED = {"wino_dw_fused_kernel"}
UNFUSED = {"wino_unfused:dw"} | _dma("4")  # its 16 grouped GEMMs are one launch of the LDS-DMA kernel, one split

# (n, c, h, w, f, k, stride, pad, groups) -> the dW names the trace must hold, and no other of DW_NAMES
CASES = [
    # direct row (LDS-free): a floor of 16 windows per workgroup
    ((1, 1, 21, 20, 8, 5, 1, 0, 1), _direct(1)),      # 17 windows: a full block of 16 and a block of one; 5x5 on one channel
    ((2, 3, 17, 18, 40, 3, 1, 0, 1), _direct(2)),     # W % 4 != 0 keeps it off the window row; 40 filters: ragged second block
    ((1, 6, 9, 33, 48, 2, 1, 0, 2), _direct(1)),      # two groups, a 2x2 filter, odd W
    ((3, 2, 10, 34, 64, 3, 1, 0, 1), _direct(2)),     # three blocks, two input channels
    # fused and unfused F(2x2,3x3)
    ((15, 256, 7, 7, 256, 3, 1, 1, 1), FUSED),        # odd plane: the tiles hang over; 16 channel blocks, 8 splits
    ((21, 128, 14, 14, 128, 3, 1, 1, 1), FUSED),      # 33 splits, the last short
    ((3, 128, 14, 14, 128, 3, 1, 1, 1), UNFUSED),     # 147 tiles
    ((3, 128, 13, 15, 130, 3, 1, 1, 1), UNFUSED),     # odd plane, ragged filter block
    ((3, 130, 13, 15, 128, 3, 1, 1, 1), UNFUSED),     # odd plane, ragged channel block
    ((2, 128, 14, 14, 128, 3, 1, 1, 1), _dma("4")),   # 98 tiles < 128: the grouped GEMM is refused, nine taps on the LDS-DMA row
    # LDS-DMA row
    ((4, 64, 14, 14, 128, 1, 1, 0, 1), _dma("4")),    # 128 x 64 tile; last split 112 of 224
    ((4, 34, 14, 14, 130, 1, 1, 0, 1), _dma("4")),    # two ragged row tiles, 34 channels in a 64-wide tile
    ((6, 18, 28, 28, 64, 1, 1, 0, 1), _dma("16")),    # 19 splits; Cg % 4 != 0 bars the x4 form; last split 96 of 256
    ((6, 20, 28, 28, 64, 1, 1, 0, 1), _dma("x4")),    # the same with the x4 form
    ((6, 16, 28, 28, 32, 3, 1, 1, 1), _dma("16")),    # nine taps, 19 splits; Mg = 32 and Cg = 16: the row's lower edges
    ((4, 32, 12, 12, 72, 3, 2, 1, 2), _dma("4")),     # two groups, stride 2
    ((4, 48, 9, 7, 66, 3, 1, 0, 1), _dma("4")),       # 128-row tile, H != W, no padding
    ((5, 16, 8, 8, 32, 5, 1, 2, 1), _dma("4")),       # 25 taps
    # lower edges of the LDS-DMA row: the register-staged row instead
    ((1, 16, 4, 8, 32, 1, 1, 0, 1), _staged(1, 1)),   # total_q = 32 < 128
    ((4, 16, 4, 8, 32, 1, 1, 0, 1), _dma("4")),       # ... and the same layer at N = 4
    ((2, 64, 8, 8, 33, 1, 1, 0, 1), _staged(2, 2, biascol=False)),  # odd Mg; K = 64 fills the tile
    ((2, 16, 10, 10, 33, 3, 1, 1, 1), _staged(2, 2)),
    # few-channel row
    ((2, 3, 16, 16, 64, 5, 1, 2, 1), _small_c()),     # K = 75: two column tiles
    ((2, 3, 30, 30, 40, 7, 2, 3, 1), _small_c()),     # OW = 15 keeps it off the stem row; K = 147: three tiles; last split 194
    ((9, 4, 24, 24, 64, 5, 1, 0, 1), _small_c()),     # 15 splits, the last of 16 columns
    ((1, 7, 12, 12, 34, 5, 1, 2, 1), _small_c()),     # seven channels; Mg = 34: the lower edge
    ((2, 3, 16, 16, 35, 5, 1, 2, 1), _staged(2, 2)),  # ... odd Mg
    # register-staged row
    ((2, 8, 96, 96, 8, 1, 1, 0, 1), _staged(1, 1, fin="4")),  # 72 splits
    ((2, 40, 9, 9, 20, 1, 1, 0, 1), _staged(1, 2)),
    ((2, 64, 9, 9, 16, 1, 1, 0, 1), _staged(1, 2, biascol=False)),  # K = 64 fills the tile: db from bcnn_hip_grad_bias
    ((2, 32, 8, 8, 24, 1, 1, 0, 1), _staged(1, 2)),   # K = 32: the second column tile exists for the bias column alone
    ((2, 3, 32, 32, 33, 3, 1, 5, 1), _staged(2, 1)),  # pad 5 is beyond the window rule; 13 splits
    ((5, 8, 21, 21, 40, 3, 1, 0, 1), _staged(2, 2)),  # 8 splits, the last of 13 columns: three of its four waves see none
    ((3, 8, 20, 20, 100, 3, 2, 1, 1), _staged(2, 2)),  # two row tiles, the second ragged
    ((2, 12, 11, 11, 70, 3, 2, 0, 2), _staged(2, 2)),  # two groups
    ((1, 4, 5, 5, 6, 3, 1, 1, 1), _staged(1, 2)),     # 25 columns in one 64-column step
]
IDS = ["x".join(map(str, s)) for s, _ in CASES]
BN_LAYER = (2, 32, 8, 8, 24, 1, 1, 0, 1)
UNALIGNED_LAYER = (2, 3, 17, 18, 40, 3, 1, 0, 1)
# the four rows with files of their own (test_window_conv.py, test_winograd43_dw.py, test_conv_large_kernel.py): one shape each
OTHER_ROWS = [((2, 3, 16, 16, 64, 3, 1, 1, 1), "conv_dw_rows_kernel"), ((2, 3, 32, 32, 64, 7, 2, 3, 1), "conv_dw_stem_kernel"),
              ((16, 64, 56, 56, 64, 3, 1, 1, 1), "wino43_dw_kernel"), ((2, 3, 23, 23, 16, 11, 4, 0, 1), "conv_large_dw_kernel")]


def _trace_start():
    from bcnn_amd import _lib
    _lib.load().bcnn_hip_trace_enable(1)


def _trace_stop():
    from bcnn_amd import _lib
    L = _lib.load()
    n = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return set(buf.value.decode().split())


def _out_hw(layer):
    n, c, h, w, f, k, st, pad, g = layer
    return (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1


def _integers(layer):
    """x in -2..2, w in -1..1, bias in -3..3, dy in -1..1, carries in -8..8: float32 CPU tensors from a fixed seed"""
    n, c, h, w, f, k, st, pad, g = layer
    oh, ow = _out_hw(layer)
    rs = np.random.RandomState(sum(layer) * 131 + c)
    T = lambda lo, hi, *sh: torch.from_numpy(rs.randint(lo, hi + 1, sh).astype(np.float32))
    return dict(x=T(-2, 2, n, c, h, w), w=T(-1, 1, f, c // g, k, k), b=T(-3, 3, f), dy=T(-1, 1, n, f, oh, ow),
                dw0=T(-8, 8, f, c // g, k, k), db0=T(-8, 8, f))


def _reference(t, layer, act, slopes=None):
    """float64: y, dx, dw, db and the largest value of the same convolutions on the absolute values; z: the convolution
    plus bias in front of the activation (tests/test_conv_fwd_dx_ladder.py applies the other cheap activations to it).
    act: NONE, RELU or PRELU with one float32 slope per filter"""
    n, c, h, w, f, k, st, pad, g = layer
    x, wt, dy = t["x"].double().requires_grad_(), t["w"].double().requires_grad_(), t["dy"].double()
    b = t["b"].double()
    b = torch.where(b == 1.0, torch.zeros_like(b), b)                    # bcnn_add_scalar adds nothing for exactly 1.0f
    z = F.conv2d(x, wt, None, st, pad, 1, g) + b.view(1, f, 1, 1)
    y = z
    if act == RELU:
        y = torch.relu(z)
    elif act == PRELU:
        y = torch.where(z > 0, z, z * slopes.double().view(1, f, 1, 1))
    else:
        assert act == NONE, act
    y.backward(dy)
    gy = dy * (y > 0) if act == RELU else dy
    if act == PRELU:
        gy = dy * torch.where(y > 0, torch.ones_like(y), slopes.double().view(1, f, 1, 1).expand_as(y))
    ref = dict(y=y.detach(), dx=x.grad, dw=wt.grad, db=gy.sum(dim=(0, 2, 3)), z=z.detach())
    xa, wa = t["x"].double().abs().requires_grad_(), t["w"].double().abs().requires_grad_()
    ya = F.conv2d(xa, wa, None, st, pad, 1, g) + t["b"].double().abs().view(1, f, 1, 1)
    ya.backward(dy.abs())
    largest = max(float(v.max()) for v in (ya.detach(), xa.grad, wa.grad, dy.abs().sum(dim=(0, 2, 3))))
    return ref, largest


def _workspace(ops, layer):
    """exactly conv_workspace_size floats at the front of a larger tensor that holds the sentinel everywhere"""
    need = ops.conv_workspace_size(*layer)
    assert need > 0, layer
    whole = torch.full((need + 4096,), SENTINEL, device=DEV)
    return whole, whole[:need]


def _run_hip(t, layer, act, dy=None, with_dx=True):
    """forward, then backward twice from the same carry; y and dx start as NaN, the workspace as the sentinel"""
    from bcnn_amd import ops
    n, c, h, w, f, k, st, pad, g = layer
    oh, ow = _out_hw(layer)
    d = {key: v.to(DEV) for key, v in t.items()}
    y = torch.full((n, f, oh, ow), float("nan"), device=DEV)
    ops.conv_forward(d["x"], d["w"], d["b"], y, k, st, pad, g, act)
    whole, ws = _workspace(ops, layer)
    out = []
    for rep in range(2):
        if dy is None:
            g_in = d["dy"].clone()
        else:
            g_in = dy
            g_in.copy_(d["dy"])
        dx = torch.full_like(d["x"], float("nan")) if with_dx else None
        dw, db = d["dw0"].clone(), d["db0"].clone()
        if rep == 0:
            _trace_start()
        ops.conv_backward(d["x"], d["w"], y, g_in, dx, dw, db, k, st, pad, g, act, ws)
        if rep == 0:
            trace = _trace_stop()
        out.append((dx, dw, db))
    torch.cuda.synchronize()
    (dx, dw, db), (_, dw2, _) = out
    got = dict(y=y.cpu(), dw=(dw - d["dw0"]).cpu(), db=(db - d["db0"]).cpu())
    if with_dx:
        got["dx"] = dx.cpu()
    return dict(trace=trace, got=got, repeat=torch.equal(dw, dw2), sentinel=bool((whole[ws.numel():] == SENTINEL).all()))


@functools.lru_cache(maxsize=None)
def _ran(i):
    """case i once: shared by its own test and by the row coverage"""
    layer = CASES[i][0]
    act = RELU if i % 2 else NONE
    t = _integers(layer)
    ref, largest = _reference(t, layer, act)
    r = _run_hip(t, layer, act)
    r.update(ref=ref, largest=largest, act=act)
    return r


def _assert_exact(r, layer, keys=("y", "dx", "dw", "db"), limit=LIMIT):
    assert r["largest"] < limit, (layer, r["largest"])            # the reference alone: what makes equality legitimate
    for key in keys:
        want = r["ref"][key].float()
        assert torch.equal(want.double(), r["ref"][key]), (layer, key)
        got = r["got"][key]
        bad = int((got != want).sum())
        assert torch.equal(got, want), "%s %s: %d of %d elements differ, by up to %g" % (
            layer, key, bad, want.numel(), float((got - want).abs().nan_to_num(nan=float("inf")).max()))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_family_takes_the_layer_and_is_exact_on_integers(i):
    layer, expected = CASES[i]
    r = _ran(i)
    print("dW of %s, act %d, ran on: %s" % (layer, r["act"], ", ".join(sorted(r["trace"] & DW_NAMES))))
    assert r["trace"] & DW_NAMES == expected, (layer, sorted(r["trace"]))
    _assert_exact(r, layer)
    assert r["repeat"], (layer, "a second run gave another dw")
    assert r["sentinel"], (layer, "written behind conv_workspace_size floats")


def _float_case(layer, seed):
    n, c, h, w, f, k, st, pad, g = layer
    oh, ow = _out_hw(layer)
    rs = np.random.RandomState(seed)
    U = lambda scale, *sh: torch.from_numpy((rs.uniform(-1, 1, sh) * scale).astype(np.float32))
    return dict(x=U(1, n, c, h, w), w=U((3.0 / (c // g * k * k)) ** 0.5, f, c // g, k, k), b=U(0.3, f), dy=U(0.1, n, f, oh, ow))


@functools.lru_cache(maxsize=None)
def _ran_other(j):
    """a shape of a row that has a file of its own: float data, dw against float64 (activation NONE, no carry)"""
    from bcnn_amd import ops
    layer, _ = OTHER_ROWS[j]
    n, c, h, w, f, k, st, pad, g = layer
    t = _float_case(layer, 17 + j)
    d = {key: v.to(DEV) for key, v in t.items()}
    y = torch.empty(t["dy"].shape, device=DEV)
    dw, db, dx = torch.zeros_like(d["w"]), torch.zeros_like(d["b"]), torch.empty_like(d["x"])
    whole, ws = _workspace(ops, layer)
    _trace_start()
    ops.conv_backward(d["x"], d["w"], y, d["dy"].clone(), dx, dw, db, k, st, pad, g, NONE, ws)
    trace = _trace_stop()
    torch.cuda.synchronize()
    wt = t["w"].double().requires_grad_()
    F.conv2d(t["x"].double(), wt, None, st, pad, 1, g).backward(t["dy"].double())
    return dict(trace=trace, got=dw.cpu().double(), ref=wt.grad, sentinel=bool((whole[ws.numel():] == SENTINEL).all()))


def test_every_row_of_the_dw_table_is_hit():
    seen = set()
    for i in range(len(CASES)):
        seen |= _ran(i)["trace"]
    for j, (layer, name) in enumerate(OTHER_ROWS):
        r = _ran_other(j)
        assert r["trace"] & DW_NAMES == {name}, (layer, sorted(r["trace"]))
        assert r["sentinel"], layer
        err, scale = (r["got"] - r["ref"]).abs(), float(r["ref"].abs().max())
        assert float(err.max()) <= 1e-4 * scale, (layer, float(err.max()) / scale)      # the bar of the rows' own files
        if name == "wino43_dw_kernel":                                                   # ... and of test_winograd43_dw.py
            assert float(err.max()) <= 3e-5 * scale, (layer, float(err.max()) / scale)
            assert float((err / (1e-4 * r["ref"].abs() + 1e-5 * scale)).max()) <= 1.0, layer
        seen |= r["trace"]
    # (the instantiations of the direct and the register-staged row count as their row)
    rows = {k.split("<")[0] for k in seen}
    assert [k for k in ROWS if k not in rows] == [], sorted(seen)
    assert len(ROWS) == 10


def test_a_fused_batch_norm_launches_the_narrower_tile():
    """K = 32 with a fused batch-norm: the conv has no bias gradient, plan_dw(s, false) launches <1,1> where the workspace
    was sized by plan_dw(s, true) for <1,2>. Float data (the batch-norm divides): dw against float64 autograd through
    conv + batch-norm (biased variance, eps 1e-6) at 1e-4 |ref| + 1e-5 max|ref| elementwise, the bound of
    test_winograd43_dw.py. The node's backward uses eps 1e-5 where autograd has 1e-6 (bcnn_batchnorm_layer.c:263-296):
    with w in (-2, 2) the variances are about 14 and that is a relative 3e-7, far inside the bound."""
    from bcnn_amd import ops
    layer = BN_LAYER
    n, c, h, w, f, k, st, pad, g = layer
    rs = np.random.RandomState(5)
    U = lambda scale, *sh: torch.from_numpy((rs.uniform(-1, 1, sh) * scale).astype(np.float32))
    t = dict(x=U(1, n, c, h, w), w=U(2, f, c, k, k), b=U(0.3, f), dy=U(0.1, n, f, h, w), sc=U(0.5, f) + 1.0)
    d = {key: v.to(DEV) for key, v in t.items()}
    Z = lambda: torch.zeros(f, device=DEV)
    y = torch.empty((n, f, h, w), device=DEV)
    bn = dict(run_mean=Z(), run_var=Z(), scales=d["sc"], saved_mean=Z(), saved_var=Z(), workspace=torch.empty_like(y),
              dscales=Z(), dmean=Z(), dvar=Z())
    ops.conv_forward(d["x"], d["w"], d["b"], y, k, st, pad, g, NONE, None, bn, ops.MODE_TRAIN)
    whole, ws = _workspace(ops, layer)
    dw, db, dx = torch.zeros_like(d["w"]), Z(), torch.empty_like(d["x"])
    _trace_start()
    ops.conv_backward(d["x"], d["w"], y, d["dy"].clone(), dx, dw, db, k, st, pad, g, NONE, ws, bn=bn, bias=d["b"])
    trace = _trace_stop()
    torch.cuda.synchronize()
    assert trace & DW_NAMES == {"conv_dw_kernel<1,1>", "conv_dw_finalize:16"}, sorted(trace)
    assert bool((whole[ws.numel():] == SENTINEL).all())
    wt = t["w"].double().requires_grad_()
    z = F.conv2d(t["x"].double(), wt)
    mean = z.mean(dim=(0, 2, 3), keepdim=True)
    var = (z * z).mean(dim=(0, 2, 3), keepdim=True) - mean * mean
    out = (z - mean) / torch.sqrt(var + 1e-6) * t["sc"].double().view(1, f, 1, 1) + t["b"].double().view(1, f, 1, 1)
    out.backward(t["dy"].double())
    ref, got = wt.grad, dw.cpu().double()
    worst = float(((got - ref).abs() / (1e-4 * ref.abs() + 1e-5 * float(ref.abs().max()))).max())
    print("dW behind a fused batch-norm on %s: worst element %.3f of its bound" % (", ".join(sorted(trace & DW_NAMES)), worst))
    assert worst <= 1.0, worst


def test_an_unaligned_dy_falls_through_the_direct_row():
    """conv_backward_weights_direct loads dy 16 bytes at a time and refuses a dy that starts 4 bytes into its buffer; the
    layer then runs on conv_dw_kernel<2,1>, which reads dy four bytes at a time, as does the activation backward for an
    unaligned tensor (ActBwdBody). Same integers, same exact results. (No dx here: the data-gradient kernels' loads of dy are
    not the subject.)"""
    layer = UNALIGNED_LAYER
    t = _integers(layer)
    ref, largest = _reference(t, layer, RELU)
    buf = torch.empty(t["dy"].numel() + 1, device=DEV)
    dy = buf[1:].view(t["dy"].shape)
    assert dy.data_ptr() % 16 == 4 and dy.is_contiguous()
    r = _run_hip(t, layer, RELU, dy=dy, with_dx=False)
    r.update(ref=ref, largest=largest)
    assert r["trace"] & DW_NAMES == _staged(2, 1), sorted(r["trace"])
    _assert_exact(r, layer, keys=("y", "dw", "db"))
    assert r["repeat"] and r["sentinel"]


def test_grad_bias_of_an_unaligned_tensor():
    """bcnn_hip_grad_bias (what a register-staged dW without a free bias column leaves the bias gradient to) sums planes of
    HW % 4 == 0 in groups of four: an unaligned tensor takes 4-byte loads, in the same order -- the same integers"""
    from bcnn_amd import _lib
    L = _lib.load()
    n, c, hw = 3, 5, 36
    rs = np.random.RandomState(2)
    g = torch.from_numpy(rs.randint(-3, 4, (n, c, hw)).astype(np.float32))
    carry = torch.from_numpy(rs.randint(-8, 9, c).astype(np.float32))
    buf = torch.empty(g.numel() + 1, device=DEV)
    gu = buf[1:].view(g.shape)
    gu.copy_(g)
    assert gu.data_ptr() % 16 == 4
    db = carry.to(DEV)
    L.bcnn_hip_grad_bias(db.data_ptr(), gu.data_ptr(), n, c, hw)
    torch.cuda.synchronize()
    assert torch.equal(db.cpu(), carry + g.sum(dim=(0, 2)))
