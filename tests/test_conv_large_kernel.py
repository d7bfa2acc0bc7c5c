"""Convolutions with kernels larger than 7x7 (bcnn_amd/csrc/conv_large.hip): a fixed list of shapes
around the AlexNet stem (11x11 / s4), every kernel size 8 .. 16 and one 31x31, groups with ragged channel counts, planes
smaller than the kernel, strides next to the kernel size (stride-parity classes of one tap), every activation of the fused
epilogue. Forward, dW - dW0, dbias - dbias0 and dX are checked against torch's float64 convolution at 1e-4 of the
reference tensor's maximum (the bar of tests/test_conv_dispatch_sweep.py); dW and dbias accumulate onto a random carry and
dX is pre-filled with garbage (it is overwritten). Then, on the scaled-down stem inside a net: the weight gradient is
bit-identical between two passes, and does not depend on the stream it is computed on (the bar of
tests/test_side_stream.py). Before this family every one of these shapes ended the process at its first forward, so the
first case also runs in a child process: there it fails as a test instead of taking pytest down."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, c, h, w, f, k, s, p, g)
STEM = (3, 3, 67, 67, 96, 11, 4, 0, 1)      # the AlexNet stem geometry, scaled down
SHAPES = [
    STEM,
    (2, 3, 67, 67, 64, 11, 4, 2, 1),        # torchvision's variant
    (2, 1, 20, 20, 16, 9, 1, 4, 1),
    (2, 64, 14, 14, 64, 9, 1, 4, 1),
    # every k = 8 .. 16 once, s in {1 .. 5}, p in {0, 1, k/2, k-1}
    (2, 4, 24, 21, 20, 8, 1, 0, 1),
    (2, 4, 24, 21, 20, 9, 2, 1, 1),
    (2, 4, 24, 21, 20, 10, 3, 5, 1),
    (2, 4, 24, 21, 20, 11, 4, 10, 1),
    (2, 4, 24, 21, 20, 12, 5, 0, 1),
    (2, 4, 24, 21, 20, 13, 1, 1, 1),
    (2, 4, 24, 21, 20, 14, 2, 7, 1),
    (2, 4, 24, 21, 20, 15, 3, 14, 1),
    (2, 4, 24, 21, 20, 16, 4, 8, 1),
    (1, 2, 40, 33, 8, 31, 1, 15, 1),        # 961 taps
    (2, 10, 18, 17, 66, 9, 2, 4, 2),        # groups: C/g = 5, F/g = 33
    (2, 15, 16, 19, 99, 8, 1, 3, 3),
    (2, 4, 5, 9, 12, 9, 1, 2, 1),           # plane smaller than the kernel: OH = 1
    (2, 6, 23, 26, 40, 8, 5, 3, 1),         # stride next to the kernel size: parity classes of one tap
    (2, 5, 30, 25, 24, 9, 7, 4, 1),
    (1, 3, 19, 27, 130, 9, 1, 0, 1),        # more than one 128-row tile
]


def _rel(a, r):
    return float((a.double() - r).abs().max() / max(float(r.abs().max()), 1e-30))


def _inputs(shape):
    import torch
    dev = "cuda:0"
    n, c, h, w, f, k, s, p, g = shape
    gen = torch.Generator(device=dev).manual_seed(sum(shape))
    x = torch.rand((n, c, h, w), device=dev, generator=gen) * 2 - 1
    wt = (torch.rand((f, c // g, k, k), device=dev, generator=gen) * 2 - 1) * (3.0 / ((c // g) * k * k)) ** 0.5
    b = torch.rand(f, device=dev, generator=gen) - 0.5
    return gen, x, wt, b


def _run_case(shape):
    import torch
    import torch.nn.functional as F
    from bcnn_amd import ops
    dev = "cuda:0"
    n, c, h, w, f, k, s, p, g = shape
    gen, x, wt, b = _inputs(shape)
    oh, ow = ops.conv_out_hw(h, w, k, s, p)
    assert oh >= 1 and ow >= 1, shape
    y = torch.full((n, f, oh, ow), 3.0, device=dev)
    ops.conv_forward(x, wt, b, y, k, s, p, g, 0)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, b.double(), stride=s, padding=p, groups=g)
    dy = (torch.rand(y.shape, device=dev, generator=gen) * 2 - 1) * 0.1
    yr.backward(dy.double())
    dx = torch.full_like(x, 7.0)                               # garbage: dX overwrites
    dw0 = torch.rand(wt.shape, device=dev, generator=gen)      # beta = 1: gradients accumulate onto a carry
    db0 = torch.rand(f, device=dev, generator=gen)
    dw, db = dw0.clone(), db0.clone()
    ws = torch.zeros(max(1, ops.conv_workspace_size(n, c, h, w, f, k, s, p, g)), device=dev)
    ops.conv_backward(x, wt, y, dy.clone(), dx, dw, db, k, s, p, g, 0, ws)
    torch.cuda.synchronize()
    errs = dict(y=_rel(y, yr.detach()), dw=_rel(dw - dw0, wr.grad), db=_rel(db - db0, dy.double().sum((0, 2, 3))),
                dx=_rel(dx, xr.grad))
    print("conv_large %s: %s" % (shape, " ".join("%s %.2e" % kv for kv in errs.items())))
    for key, err in errs.items():
        assert err <= 1e-4, (shape, key, err)


def test_alexnet_stem_in_a_child_process():
    code = "from tests.test_conv_large_kernel import _run_case, STEM; _run_case(STEM)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_matches_torch_float64(shape):
    _run_case(shape)


def _act_ref(v, act, slopes):
    import torch
    if act == 1:
        return torch.tanh(v)
    if act == 2:
        return torch.relu(v)
    if act == 3:
        return torch.relu(v) + 0.1 * v
    if act == 4:
        return torch.nn.functional.softplus(v)
    if act == 5:
        return torch.where(v > 0, v, 0.1 * v)
    if act == 6:
        return v.abs()
    if act == 7:
        return v.clamp(0, 1)
    if act == 8:
        return torch.where(v > 0, v, slopes.double().view(1, -1, 1, 1) * v)
    if act == 9:
        return torch.sigmoid(v)
    return v


@pytest.mark.parametrize("act", sorted(__import__("bcnn_amd.ops", fromlist=["ACT"]).ACT.items(), key=lambda kv: kv[1]),
                         ids=lambda kv: kv[0])
def test_every_activation_of_the_forward(act):
    """bias, then the activation (PReLU with per-filter slopes), on a 9x9 / s2 layer with two groups"""
    import torch
    import torch.nn.functional as F
    from bcnn_amd import ops
    shape = (2, 6, 21, 18, 40, 9, 2, 3, 2)
    n, c, h, w, f, k, s, p, g = shape
    gen, x, wt, b = _inputs(shape)
    b[3] = 1.0  # quirk 2: a bias of exactly 1 is not added
    slopes = torch.rand(f, device="cuda:0", generator=gen) * 0.4 + 0.05
    oh, ow = ops.conv_out_hw(h, w, k, s, p)
    y = torch.full((n, f, oh, ow), 3.0, device="cuda:0")
    ops.conv_forward(x, wt, b, y, k, s, p, g, act[1], slopes=slopes if act[0] == "prelu" else None)
    torch.cuda.synchronize()
    bq = b.double().clone()
    bq[3] = 0.0
    yr = _act_ref(F.conv2d(x.double(), wt.double(), bq, stride=s, padding=p, groups=g), act[1], slopes)
    err = _rel(y, yr)
    print("conv_large act %s: y %.2e" % (act[0], err))
    assert err <= 1e-4, (act, err)


# ---- inside a net: determinism and the weight-gradient side stream ------------------------------------------------------
def _stem_net(seed):
    from bcnn_amd import capi
    n, c, h, w, f, k, s, p, g = STEM
    ctypes.CDLL(None).srand(5)
    net = capi.Net(mode=capi.MODE_TRAIN, n=n, w=w, h=h, c=c, input_grad=True)
    net.conv(f, k, s, p, 1, 0, capi.ACT_RELU, "input", "stem")
    net.conv(32, 9, 1, 4, 2, 1, capi.ACT_RELU, "stem", "c2")  # 9x9, two groups, fused batch-norm: the raw = 1 epilogue
    net.avgpool("c2", "gap")
    net.fullc(10, capi.ACT_NONE, "gap", "fc")
    net.softmax("fc", "sm")
    net.cost("sm", "label", "cost", 1.0)
    net.compile()
    rs = np.random.RandomState(seed)
    net.data(0)[...] = rs.uniform(-1, 1, net.shape(0)).astype(np.float32)
    lab = np.zeros(net.shape(1), np.float32)
    for b in range(n):
        lab[b, rs.randint(10)] = 1.0
    net.data(1)[...] = lab
    net.upload(0)
    net.upload(1)
    return net


def test_weight_gradient_is_deterministic_and_independent_of_its_stream():
    from tests.test_side_stream import _pass, _trace
    net = _stem_net(seed=11)
    _trace(True)
    main = _pass(net, 0)
    kernels = _trace(False)
    assert {"conv_large_gemm_kernel:fwd", "conv_large_gemm_kernel:dx", "conv_large_dw_kernel"} <= kernels, kernels
    again = _pass(net, 0)
    side = _pass(net, 1)
    side_again = _pass(net, 1)
    dw = net.index("input_w")  # a conv node names its weights after its source
    assert float(np.abs(main[dw]).max()) > 0
    assert main.keys() == side.keys() and dw in main
    for i in main:
        assert np.array_equal(main[i].view(np.uint32), again[i].view(np.uint32)), "tensor %d differs between two passes" % i
        assert np.array_equal(side[i].view(np.uint32), side_again[i].view(np.uint32)), "tensor %d, side stream" % i
        ref = np.abs(main[i]).max()
        err = np.abs(side[i] - main[i]).max()
        assert err <= 2e-6 * ref + 1e-12, "tensor %d: %g of %g between the two stream arrangements" % (i, err, ref)
    net.close()
