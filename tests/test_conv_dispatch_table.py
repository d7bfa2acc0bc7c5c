"""Which kernel family takes which convolution, pinned with the dispatch trace (bcnn_hip_trace_*): one shape per row of
kConvFwdFamilies / kConvDxFamilies (bcnn_amd/csrc/conv.hip), every row hit at least once; bcnn_hip_conv_prepack plans for the
family that then runs (no `pack:self` left behind a prepack call, bit-identical outputs where nothing is packed); and a layer
without output or input pixels launches nothing.

The expectations are read off the families' shape rules (window_ok, stem_ok, wino43_wanted, wino_fused_wanted, dma_supported,
...), 256 compute units: e.g. (16, 64, 64, 64) has 4096 tiles of 4 x 4 = 128 blocks of 32 x 2 filter blocks = 256 units, enough
for F(4x4,3x3); (32, 64, 32, 64) has 128 of them, too few, and 8192 tiles of 2 x 2, enough for the fused F(2x2,3x3) kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_product_dispatch_parity import _trace_start, _trace_stop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RELU = 2

# (n, c, h = w, f, k, stride, pad), one group -> the family of the forward with bias + activation, of the raw forward (a
# batch-norm follows, TRAIN mode) and of the data gradient; None: not pinned here. The Winograd rows depend on the number
# of compute units the rules are written for (kCUs = 256, common.h)
CASES = {
    "window": ((2, 3, 16, 32, 3, 1, 1), "conv_fwd_window_kernel", "conv_fwd_window_kernel", "conv_small_c:dx"),  # dX: K = 27, Mg = 32
    "stem": ((2, 3, 32, 64, 7, 2, 3), "conv_fwd_stem_kernel", "conv_fwd_stem_kernel", None),
    "direct": ((2, 3, 16, 32, 3, 2, 1), "conv_fwd_direct_kernel", "conv_fwd_direct_kernel", None),  # stride 2: not the window's
    "winograd43": ((16, 64, 64, 64, 3, 1, 1), "wino_fused_kernel:fwd", "wino43b_kernel:fwd", "wino43b_kernel:dx"),
    "winograd_fused": ((32, 64, 32, 64, 3, 1, 1), "wino_fused_kernel:fwd", "wino_fused_kernel:fwd", "wino_fused_kernel:dx"),
    "winograd": ((2, 128, 14, 128, 3, 1, 1), "wino_unfused:fwd", "wino_unfused:fwd", "wino_unfused:dx"),
    "large": ((2, 3, 23, 16, 11, 4, 0), "conv_large_gemm_kernel:fwd", "conv_large_gemm_kernel:fwd", "conv_large_gemm_kernel:dx"),
    "dma_1x1": ((4, 64, 14, 128, 1, 1, 0), "conv_igemm_dma_kernel:fwd", "conv_igemm_dma_kernel:fwd", "conv_igemm_dma_kernel:dx"),
    "dma_3x3s2": ((4, 64, 28, 128, 3, 2, 1), "conv_igemm_dma_kernel:fwd", "conv_igemm_dma_kernel:fwd", "conv_igemm_dma_kernel:dx"),
    "small_c": ((2, 3, 16, 64, 5, 1, 2), "conv_small_c:fwd", "conv_small_c:fwd", None),  # K = 75
    "register_staged": ((2, 16, 8, 16, 1, 1, 0), "conv_igemm_kernel:fwd", "conv_igemm_kernel:fwd", "conv_igemm_kernel:dx"),
}
# every row of the two tables, in their order (the first form of F(4x4,3x3) exists in the experiment build only)
FWD_FAMILIES = ["conv_fwd_window_kernel", "conv_fwd_stem_kernel", "conv_fwd_direct_kernel", "wino43b_kernel:fwd",
                "wino_fused_kernel:fwd", "wino_unfused:fwd", "conv_large_gemm_kernel:fwd", "conv_igemm_dma_kernel:fwd",
                "conv_small_c:fwd", "conv_igemm_kernel:fwd"]
DX_FAMILIES = ["wino43b_kernel:dx", "wino_fused_kernel:dx", "wino_unfused:dx", "conv_large_gemm_kernel:dx", "conv_small_c:dx",
               "conv_igemm_dma_kernel:dx", "conv_igemm_kernel:dx"]
PACKING = ["winograd43", "winograd_fused", "dma_1x1", "dma_3x3s2"]
NOT_PACKING = ["window", "large", "winograd", "small_c"]


class Desc(C.Structure):
    _fields_ = [("w_d", C.c_void_p)] + [(k, C.c_int) for k in ("n", "c", "h", "w", "f", "k", "stride", "pad", "groups")]


def _make(name):
    n, c, hw, f, k, st, pad = CASES[name][0]
    rs = np.random.RandomState(len(name) + 7 * n + c)
    T = lambda *sh: torch.from_numpy(rs.uniform(-1, 1, sh).astype(np.float32)).to(DEV)
    oh = (hw + 2 * pad - k) // st + 1
    return dict(layer=CASES[name][0], x=T(n, c, hw, hw), w=T(f, c, k, k) * 0.1, b=T(f) * 0.1, dy=T(n, f, oh, oh) * 0.01, oh=oh)


def _forward(ops, it):
    n, c, hw, f, k, st, pad = it["layer"]
    y = torch.empty((n, f, it["oh"], it["oh"]), device=DEV)
    ops.conv_forward(it["x"], it["w"], it["b"], y, k, st, pad, 1, RELU)
    return y


def _forward_raw(ops, it):
    """batch_norm = 1, TRAIN: the bare convolution goes to the batch-norm workspace, its normalised form to y"""
    n, c, hw, f, k, st, pad = it["layer"]
    Z = lambda *sh: torch.zeros(*sh, device=DEV)
    y = torch.empty((n, f, it["oh"], it["oh"]), device=DEV)
    bn = dict(run_mean=Z(f), run_var=Z(f), scales=torch.ones(f, device=DEV), saved_mean=Z(f), saved_var=Z(f),
              workspace=torch.empty_like(y))
    ops.conv_forward(it["x"], it["w"], it["b"], y, k, st, pad, 1, RELU, None, bn, ops.MODE_TRAIN)
    return bn["workspace"], y


def _backward(ops, it, y):
    n, c, hw, f, k, st, pad = it["layer"]
    dy, dx = it["dy"].clone(), torch.zeros_like(it["x"])
    dw, db = torch.zeros_like(it["w"]), torch.zeros_like(it["b"])
    ws = torch.zeros(max(1, ops.conv_workspace_size(n, c, hw, hw, f, k, st, pad, 1)), device=DEV)
    ops.conv_backward(it["x"], it["w"], y, dy, dx, dw, db, k, st, pad, 1, RELU, ws)
    return dx, dw


def _traced(fn, *args):
    _trace_start()
    out = fn(*args)
    return out, _trace_stop()


@pytest.fixture(scope="module")
def runs():
    """every case once, without prepack: the traces of the three calls and their outputs"""
    from bcnn_amd import _lib, ops
    _lib.load().bcnn_hip_conv_prepack_reset()
    out = {}
    for name in CASES:
        it = _make(name)
        y, t_act = _traced(_forward, ops, it)
        raw, t_raw = _traced(_forward_raw, ops, it)
        grads, t_bwd = _traced(_backward, ops, it, y)
        out[name] = dict(it=it, y=y, raw=raw, grads=grads, trace=dict(act=t_act, raw=t_raw, bwd=t_bwd))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(CASES), ids=["%s-%s" % (k, v[1]) for k, v in CASES.items()])
def test_the_family_that_takes_the_shape(runs, name):
    _, fwd_act, fwd_raw, dx = CASES[name]
    tr = runs[name]["trace"]
    assert tr["act"].get(fwd_act, 0) > 0, ("forward with bias + activation", CASES[name][0], tr["act"])
    assert tr["raw"].get(fwd_raw, 0) > 0, ("raw forward", CASES[name][0], tr["raw"])
    if dx is not None:
        assert tr["bwd"].get(dx, 0) > 0, ("data gradient", CASES[name][0], tr["bwd"])
    if name.startswith("dma"):  # the few-channel forward ends in the same launcher: told apart by its own name
        assert "conv_small_c:fwd" not in tr["act"] and "conv_small_c:fwd" not in tr["raw"], tr


def test_every_row_of_both_tables_is_hit(runs):
    fwd, bwd = set(), set()
    for r in runs.values():
        fwd |= set(r["trace"]["act"]) | set(r["trace"]["raw"])
        bwd |= set(r["trace"]["bwd"])
    assert [k for k in FWD_FAMILIES if k not in fwd] == [], sorted(fwd)
    assert [k for k in DX_FAMILIES if k not in bwd] == [], sorted(bwd)


def _descs(items):
    arr = (Desc * len(items))()
    for d, it in zip(arr, items):
        n, c, hw, f, k, st, pad = it["layer"]
        d.w_d = it["w"].data_ptr()
        d.n, d.c, d.h, d.w, d.f, d.k, d.stride, d.pad, d.groups = n, c, hw, hw, f, k, st, pad, 1
    return arr


def test_prepack_plans_for_the_family_that_runs(runs):
    from bcnn_amd import _lib, ops
    L = _lib.load()
    names = PACKING + NOT_PACKING
    items = [runs[k]["it"] for k in names]
    arr = _descs(items)
    try:
        L.bcnn_hip_conv_prepack(C.cast(arr, C.c_void_p), len(items), 0)
        for k in names:
            (raw, y), tr = _traced(_forward_raw, ops, runs[k]["it"])
            if k in PACKING:
                assert "pack:self" not in tr, (k, "raw forward behind a forward prepack", tr)
            else:
                assert torch.equal(raw, runs[k]["raw"][0]) and torch.equal(y, runs[k]["raw"][1]), k
        L.bcnn_hip_conv_prepack(C.cast(arr, C.c_void_p), len(items), 1)
        for k in names:
            (dx, dw), tr = _traced(_backward, ops, runs[k]["it"], runs[k]["y"])
            if k in PACKING:
                assert "pack:self" not in tr, (k, "data gradient behind a data-gradient prepack", tr)
            else:
                assert torch.equal(dx, runs[k]["grads"][0]) and torch.equal(dw, runs[k]["grads"][1]), k
    finally:
        L.bcnn_hip_conv_prepack_reset()
    for k in PACKING:  # nothing packed ahead: each family packs for itself (the fixture ran behind a reset too)
        _, tr = _traced(_forward_raw, ops, runs[k]["it"])
        assert tr.get("pack:self", 0) > 0, (k, "raw forward", tr)
        assert runs[k]["trace"]["raw"].get("pack:self", 0) > 0, (k, runs[k]["trace"]["raw"])
        _, tr = _traced(_backward, ops, runs[k]["it"], runs[k]["y"])
        assert tr.get("pack:self", 0) > 0, (k, "data gradient", tr)


# n >= 1 (tests/test_edge_cases.py has the empty batch; F = 0 is refused upstream). A 3x3 filter on a 2 x 2 plane without
# padding has no output pixel: nothing to compute forward, no weight gradient; its input gradient is all zeros, which is a
# launch, so that call carries no dx. A plane without rows has no input pixel either: the data gradient returns as well.
@pytest.mark.parametrize("n,c,h,w,f,k,with_dx", [(1, 16, 2, 2, 16, 3, False), (1, 16, 0, 4, 16, 1, True)],
                         ids=["no_output_pixels", "no_input_pixels"])
def test_a_layer_without_pixels_launches_nothing(n, c, h, w, f, k, with_dx):
    from bcnn_amd import ops
    oh, ow = ops.conv_out_hw(h, w, k, 1, 0)
    assert n * f * oh * ow == 0
    x = torch.zeros((n, c, h, w), device=DEV)
    wt, b = torch.ones((f, c, k, k), device=DEV), torch.zeros(f, device=DEV)
    y = torch.empty((n, f, oh, ow), device=DEV)
    dw, db = torch.full_like(wt, 2.0), torch.full_like(b, 3.0)
    ws = torch.zeros(16, device=DEV)
    _trace_start()
    ops.conv_forward(x, wt, b, y, k, 1, 0, 1, RELU)
    ops.conv_backward(x, wt, y, torch.empty_like(y), torch.empty_like(x) if with_dx else None, dw, db, k, 1, 0, 1, RELU, ws)
    assert _trace_stop() == {}
    torch.cuda.synchronize()
    assert float(dw.min()) == 2.0 and float(db.max()) == 3.0  # gradients untouched
