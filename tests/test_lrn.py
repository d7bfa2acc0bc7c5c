"""The local response normalisation node, bcnn_add_lrn_layer (reference bcnn_lrn_layer.c):
  - the kernels (bcnn_hip_lrn_forward / _backward) against an fp64 NumPy model of the formulas in include/bcnn_hip.h
    over even and odd window sizes, ragged H*W and large batches, and against torch.nn.functional.local_response_norm
    (CPU, float64) for odd sizes, forward and through autograd;
  - overwrite 0 / 1, and a column split into channel chunks gives the same bits as one march;
  - the reference's deviations pinned one at a time, k honoured, the refusals, and an INI [lrn]
    section whose fractional alpha is parsed."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_bind as rb


def np_lrn(x, n, alpha, beta, k):
    """fp64: returns y and s; window of c = [c - (n-1)/2, c + n/2] clipped"""
    x = x.astype(np.float64)
    cc = x.shape[1]
    sq = x * x
    s = np.empty_like(x)
    for c in range(cc):
        lo, hi = max(0, c - (n - 1) // 2), min(cc - 1, c + n // 2)
        s[:, c] = k + alpha / n * sq[:, lo:hi + 1].sum(axis=1)
    return x * s ** -beta, s


def np_lrn_backward(x, dy, n, alpha, beta, k):
    y, s = np_lrn(x, n, alpha, beta, k)
    x, dy = x.astype(np.float64), dy.astype(np.float64)
    t = dy * y / s
    cc = x.shape[1]
    acc = np.empty_like(x)
    for j in range(cc):
        lo, hi = max(0, j - n // 2), min(cc - 1, j + (n - 1) // 2)
        acc[:, j] = t[:, lo:hi + 1].sum(axis=1)
    return dy * s ** -beta - 2 * alpha * beta / n * x * acc


def _run(x, dy, n, alpha, beta, k, dx0=None, overwrite=1):
    import torch
    from bcnn_amd import ops
    tx = torch.from_numpy(x).cuda()
    ty = torch.empty_like(tx)
    ops.lrn_forward(tx, ty, n, alpha, beta, k)
    tdx = torch.from_numpy(dx0).cuda() if dx0 is not None else torch.full_like(tx, float("nan"))
    ops.lrn_backward(tx, torch.from_numpy(dy).cuda(), tdx, n, alpha, beta, k, overwrite)
    return ty.cpu().numpy(), tdx.cpu().numpy()


CASES = [  # (window, N, C, H, W)
    (1, 4, 2, 13, 13), (2, 3, 3, 1, 1), (3, 2, 7, 13, 13), (4, 2, 9, 8, 8), (5, 128, 16, 1, 1), (5, 2, 96, 55, 55),
    (5, 3, 256, 13, 13), (7, 3, 20, 4, 6), (15, 2, 16, 4, 4), (15, 5, 31, 3, 5), (16, 2, 40, 3, 5), (16, 1, 17, 2, 2),
    (2, 64, 5, 2, 2), (3, 1, 4, 55, 55)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,N,C,H,W", CASES)
def test_kernels_match_fp64_model(n, N, C, H, W):
    rs = np.random.RandomState(n * 1000 + C)
    x = rs.uniform(-2, 2, (N, C, H, W)).astype(np.float32)
    dy = rs.uniform(-1, 1, x.shape).astype(np.float32)
    alpha, beta, k = 0.7, 0.75, 1.3
    y, dx = _run(x, dy, n, alpha, beta, k)
    y64, _ = np_lrn(x, n, alpha, beta, k)
    assert np.all(np.abs(y - y64) <= 1e-5 * np.abs(y64) + 1e-30)
    dx64 = np_lrn_backward(x, dy, n, alpha, beta, k)
    assert np.max(np.abs(dx - dx64)) <= 1e-5 * np.max(np.abs(dx64))


@pytest.mark.gpu
@pytest.mark.parametrize("n,C,HW", [(1, 3, (5, 5)), (3, 8, (13, 13)), (5, 12, (4, 4)), (9, 20, (3, 7))])
def test_odd_sizes_match_torch_forward_and_autograd(n, C, HW):
    import torch
    rs = np.random.RandomState(n)
    x = rs.uniform(-2, 2, (3, C) + HW).astype(np.float32)
    dy = rs.uniform(-1, 1, x.shape).astype(np.float32)
    alpha, beta, k = 2e-2 * n, 0.75, 2.0
    y, dx = _run(x, dy, n, alpha, beta, k)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    yt = torch.nn.functional.local_response_norm(xt, n, alpha=alpha, beta=beta, k=k)
    yt.backward(torch.from_numpy(dy.astype(np.float64)))
    np.testing.assert_allclose(y, yt.detach().numpy(), rtol=1e-5, atol=0)
    g = xt.grad.numpy()
    assert np.max(np.abs(dx - g)) <= 1e-5 * np.max(np.abs(g))


@pytest.mark.gpu
@pytest.mark.parametrize("n,hw", [(3, (6, 6)), (5, (5, 5)), (11, (4, 4))])
def test_overwrite_flag(n, hw):
    rs = np.random.RandomState(1)
    x = rs.uniform(-1, 1, (2, 14) + hw).astype(np.float32)
    dy = rs.uniform(-1, 1, x.shape).astype(np.float32)
    dx0 = rs.uniform(-1, 1, x.shape).astype(np.float32)
    _, assigned = _run(x, dy, n, 0.5, 0.75, 1.0, dx0=dx0.copy(), overwrite=1)
    _, added = _run(x, dy, n, 0.5, 0.75, 1.0, dx0=dx0.copy(), overwrite=0)
    assert np.array_equal(added, dx0 + assigned)


@pytest.mark.gpu
@pytest.mark.parametrize("n,C,hw", [(5, 64, (55, 55)), (4, 16, (12, 12))])
def test_channel_chunks_give_the_same_bits(n, C, hw):
    """one image is few columns, so its channels are split into chunks; in a batch that fills the chip they are not"""
    rs = np.random.RandomState(2)
    N = 128 if hw == (55, 55) else 7400
    x = rs.uniform(-2, 2, (N, C) + hw).astype(np.float32)
    dy = rs.uniform(-1, 1, x.shape).astype(np.float32)
    y_all, dx_all = _run(x, dy, n, 0.9, 0.75, 1.0)
    for i in (0, N - 1):
        y1, dx1 = _run(x[i:i + 1].copy(), dy[i:i + 1].copy(), n, 0.9, 0.75, 1.0)
        assert np.array_equal(y1.view(np.uint32), y_all[i:i + 1].view(np.uint32))
        assert np.array_equal(dx1.view(np.uint32), dx_all[i:i + 1].view(np.uint32))


def _bind_ref():
    L = rb.lib()
    L.bcnn_add_lrn_layer.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_char_p, C.c_char_p]
    L.bcnn_add_lrn_layer.restype = C.c_int
    return L


def _ref_lrn(L, n, alpha, beta, k, x, dx0):
    """the reference's CPU workers on input x (1 image); returns y and dx for dy = 1 onto a dx prefilled with dx0"""
    c = x.shape[1]
    ref = rb.RefNet(mode=rb.MODE_TRAIN, w=1, h=1, c=c, n=1, input_grad=True)
    assert L.bcnn_add_lrn_layer(ref.net, n, alpha, beta, k, b"input", b"lrn") == 0
    ref.compile()
    ref.data(0)[...] = x
    ref.L.ref_forward_node(ref.net, 0)
    li = ref.index("lrn")
    y = ref.data(li).copy()
    ref.grad(li)[...] = 1.0
    ref.grad(0)[...] = dx0
    ref.L.ref_backward_node(ref.net, 0)
    dx = ref.grad(0).copy()
    ref.close()
    return y, dx


def _hip_lrn(n, alpha, beta, k, x, dx0):
    """the same through this build's node workers (bcnn_backward_node: the node accumulates)"""
    from bcnn_amd import capi
    c = x.shape[1]
    hip = capi.Net(mode=capi.MODE_TRAIN, w=1, h=1, c=c, n=1, input_grad=True)
    hip.lrn(n, alpha, beta, k, src="input", dst="lrn")
    hip.compile()
    hip.data(0)[...] = x
    hip.upload(0)
    hi = hip.index("lrn")
    hip.forward_node(0)
    hip.download(hi)
    y = hip.data(hi).copy()
    hip.grad(hi)[...] = 1.0
    hip.upload(hi, with_grad=True)
    hip.grad(0)[...] = dx0
    hip.upload(0, with_grad=True)
    hip.backward_node(0)
    hip.download(0)
    dx = hip.grad(0).copy()
    hip.close()
    return y, dx


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 4, 5])
def test_reference_deviations_one_at_a_time(n):
    """INTEGRATION.md, LRN deviations, each on its own (positive inputs, so no window sum is zero):
      - window sums: with k = 0 on both sides, the reference's channel 0 sums channels 0 .. n/2 - 1 and leaves n/2 out;
      - k: the reference's builder never stores it (alpha = 0: its scale is 0^-beta = inf, this build's k^-beta);
      - dx: the reference overwrites the source gradient, this build adds to it."""
    L = _bind_ref()
    c, alpha, beta = 8, 1.0, 1.0
    x = np.random.RandomState(n).uniform(0.5, 1.5, (1, c, 1, 1)).astype(np.float32)
    xs = x[0, :, 0, 0].astype(np.float64)
    # window sums (k = 0 given to both; the reference ignores k anyway)
    ref_y, _ = _ref_lrn(L, n, alpha, beta, 0.0, x, 0.0)
    ref_s0 = alpha / n * np.sum(xs[:n // 2] ** 2)
    np.testing.assert_allclose(ref_y[0, 0, 0, 0], xs[0] * ref_s0 ** -beta, rtol=1e-5)
    y64, _ = np_lrn(x, n, alpha, beta, 0.0)
    assert abs(ref_y[0, 0, 0, 0] - y64[0, 0, 0, 0]) > 1e-3 * abs(y64[0, 0, 0, 0])
    hip_y, _ = _hip_lrn(n, alpha, beta, 0.0, x, 0.0)
    np.testing.assert_allclose(hip_y, y64, rtol=1e-5)
    # k
    ref_y, _ = _ref_lrn(L, n, 0.0, 1.0, 2.0, x, 0.0)
    assert np.isinf(ref_y).all()
    hip_y, _ = _hip_lrn(n, 0.0, 1.0, 2.0, x, 0.0)
    np.testing.assert_allclose(hip_y, x / 2.0, rtol=1e-6)
    # the source gradient: overwritten by the reference, accumulated here
    _, ref_dx0 = _ref_lrn(L, n, 0.5, 0.75, 1.0, x, 0.0)
    _, ref_dx5 = _ref_lrn(L, n, 0.5, 0.75, 1.0, x, 5.0)
    assert np.array_equal(ref_dx0, ref_dx5, equal_nan=True)
    _, hip_dx0 = _hip_lrn(n, 0.5, 0.75, 1.0, x, 0.0)
    _, hip_dx5 = _hip_lrn(n, 0.5, 0.75, 1.0, x, 5.0)
    np.testing.assert_allclose(hip_dx0, np_lrn_backward(x, np.ones_like(x), n, 0.5, 0.75, 1.0), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(hip_dx5, hip_dx0 + 5.0, rtol=1e-6)


@pytest.mark.gpu
def test_k_is_honoured_and_refusals_leave_the_net_unchanged():
    import torch
    from bcnn_amd import capi, ops
    rs = np.random.RandomState(4)
    x = rs.uniform(-1, 1, (2, 6, 3, 3)).astype(np.float32)
    outs = []
    for k in (0.5, 2.0):
        tx = torch.from_numpy(x).cuda()
        ty = torch.empty_like(tx)
        ops.lrn_forward(tx, ty, 3, 0.4, 0.75, k)
        np.testing.assert_allclose(ty.cpu().numpy(), np_lrn(x, 3, 0.4, 0.75, k)[0], rtol=1e-5)
        outs.append(ty.cpu().numpy())
    assert not np.allclose(outs[0], outs[1])
    net = capi.Net(mode=capi.MODE_TRAIN, w=4, h=3, c=5, n=2)
    net.conv(6, 3, 1, 1, act=capi.ACT_RELU, src="input", dst="c1")
    nodes, tensors = net.L.bcnn_get_num_nodes(net.net), net.index("c1")
    for ls, a, b, k in [(0, 1e-4, 0.75, 1.0), (6, 1e-4, 0.75, 1.0), (7, 1e-4, 0.75, 1.0), (3, -1e-4, 0.75, 1.0),
                        (3, 1e-4, -0.75, 1.0), (3, 1e-4, 0.75, -1.0)]:
        assert net.L.bcnn_add_lrn_layer(net.net, ls, a, b, k, b"c1", b"lrn") != 0, (ls, a, b, k)
        assert net.L.bcnn_get_num_nodes(net.net) == nodes
        assert net.index("lrn") < 0
    net.lrn(5, 1e-4, 0.75, 1.0, src="c1", dst="lrn")
    assert net.index("lrn") > tensors
    net.close()


CAFFE_CFG = """
[network]
input_width=3
input_height=2
input_channels=12
batch_size=2

[lrn]
size=5
alpha=0.0001
beta=0.75
src=input
dst=norm1
"""


@pytest.mark.gpu
def test_ini_lrn_section_normalises(tmp_path):
    from bcnn_amd import capi
    cfg = tmp_path / "lrn.conf"
    cfg.write_text(CAFFE_CFG)
    net = capi.Net.load_net(str(cfg), mode=capi.MODE_PREDICT)
    assert net.num_nodes == 1
    assert net.L.bcnn_compile_net(net.net) == 0
    rs = np.random.RandomState(5)
    x = rs.uniform(-30, 30, net.shape(0)).astype(np.float32)
    net.data(0)[...] = x
    net.upload(0)
    net.forward()
    i = net.index("norm1")
    net.download(i)
    y = net.data(i)
    assert not np.allclose(y, x, rtol=1e-3)
    np.testing.assert_allclose(y, np_lrn(x, 5, 1e-4, 0.75, 1.0)[0], rtol=1e-5)
    net.close()
