"""The transposed-convolution (deconvolution) node, bcnn_add_deconvolutional_layer (reference bcnn_deconv_layer.c):
  - the kernels (bcnn_hip_deconv_forward / _backward) against an fp64 NumPy restatement of the reference's math over a
    grid of kernel sizes, strides (s > size included) and pads, and against torch.nn.functional.conv_transpose2d (CPU,
    float64) for pad > 0, where this build computes the standard cropped transposed convolution;
  - the node in a TRAIN graph against the unmodified reference (oracle/_ref/libbcnn_ref.so) through the public C API:
    the filler, two SGD steps with momentum, Adam from an INI config with a [deconv] section, the model file;
  - the refusals (PReLU, non-positive extent, bcnn_resize_net) and bit-identical weight gradients from run to run."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import ref_bind as rb
from tests import _detect_ref as D
from tests.test_load_net import load_both, same_graph

pytestmark = pytest.mark.gpu

ACTS = {"none": 0, "relu": 2, "lrelu": 5, "logistic": 9}
OP_TOL = 1e-5      # element-wise, times max |reference| of the tensor
NET_TOL = 1e-4     # tests/test_net_parity.py


# ---- fp64 restatement -------------------------------------------------------------------------------------------------
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


def np_forward(x, wt, b, k, s, p, act):
    """y = act(crop_p(sum over taps of x scattered at stride s) + b); wt [c][f][k][k]"""
    n, c, h, w = x.shape
    f = wt.shape[1]
    hf, wf = s * (h - 1) + k, s * (w - 1) + k
    full = np.zeros((n, f, hf, wf))
    for ky in range(k):
        for kx in range(k):
            full[:, :, ky:ky + s * (h - 1) + 1:s, kx:kx + s * (w - 1) + 1:s] += np.einsum("nchw,cf->nfhw", x,
                                                                                        wt[:, :, ky, kx])
    y = full[:, :, p:hf - p, p:wf - p] + b[None, :, None, None]
    return _act(y, act)


def np_backward(x, wt, g, k, s, p):
    """(dW (without the 1/N), dx) for the output gradient g (already multiplied by act'(y))"""
    n, c, h, w = x.shape
    f = wt.shape[1]
    gf = np.zeros((n, f, s * (h - 1) + k, s * (w - 1) + k))
    gf[:, :, p:gf.shape[2] - p, p:gf.shape[3] - p] = g
    dw = np.zeros(wt.shape)
    dx = np.zeros(x.shape)
    for ky in range(k):
        for kx in range(k):
            gs = gf[:, :, ky:ky + s * (h - 1) + 1:s, kx:kx + s * (w - 1) + 1:s]
            dw[:, :, ky, kx] = np.einsum("nchw,nfhw->cf", x, gs)
            dx += np.einsum("nfhw,cf->nchw", gs, wt[:, :, ky, kx])
    return dw, dx


def _close(tag, got, want, tol=OP_TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bound = tol * max(float(np.abs(want).max()), 1e-30)
    diff = float(np.abs(got - want).max())
    assert diff <= bound, "%s: max abs diff %.3g > %.3g" % (tag, diff, bound)


# ---- the kernels ------------------------------------------------------------------------------------------------------
def _run_op(n, c, h, w, f, k, s, p, act, seed, with_dx=True, ws_elems=None):
    """one forward + backward on the device; returns the inputs and every result (float64 numpy). ws_elems: floats of
    workspace handed to the backward pass (default: what bcnn_hip_deconv_workspace_size asks for)"""
    from bcnn_amd import ops
    rs = np.random.RandomState(seed)
    ho, wo = ops.deconv_out_hw(h, w, k, s, p)
    x = rs.uniform(-1, 1, (n, c, h, w)).astype(np.float32)
    wt = rs.uniform(-0.5, 0.5, (c, f, k, k)).astype(np.float32)
    b = rs.uniform(-0.5, 0.5, (f,)).astype(np.float32)
    dy = rs.uniform(-1, 1, (n, f, ho, wo)).astype(np.float32)
    dw0 = rs.uniform(-0.1, 0.1, wt.shape).astype(np.float32)
    db0 = rs.uniform(-0.1, 0.1, b.shape).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    tx, tw, tb, tdy, tdw, tdb = map(dev, (x, wt, b, dy, dw0, db0))
    ty = torch.full((n, f, ho, wo), float("nan"), device="cuda")
    tdx = torch.full(x.shape, float("nan"), device="cuda") if with_dx else None
    full = ops.deconv_workspace_size(n, c, h, w, f, k, s, p)
    ws = torch.zeros(full if ws_elems is None else ws_elems, device="cuda")
    ops.deconv_forward(tx, tw, tb, ty, k, s, p, act)
    y = ty.cpu().numpy().astype(np.float64)
    ops.deconv_backward(tx, tw, ty, tdy, tdx, tdw, tdb, k, s, p, act, ws)
    torch.cuda.synchronize()
    got = dict(y=y, g=tdy.cpu().numpy(), dw=tdw.cpu().numpy(), db=tdb.cpu().numpy(),
               dx=tdx.cpu().numpy() if with_dx else None)
    inp = dict(x=x.astype(np.float64), wt=wt.astype(np.float64), b=b.astype(np.float64), dy=dy.astype(np.float64),
               dw0=dw0.astype(np.float64), db0=db0.astype(np.float64))
    return inp, got


def _grid():
    cases = []
    chans = [(3, 2), (5, 6), (7, 9), (17, 13), (20, 19)]
    for idx, (k, s, p) in enumerate(itertools.product(range(1, 6), range(1, 4), range(3))):
        h, w = 5, 4
        if s * (h - 1) + k - 2 * p <= 0 or s * (w - 1) + k - 2 * p <= 0:
            continue
        c, f = chans[idx % len(chans)]
        act = list(ACTS.values())[idx % 4]
        cases.append((1 + 2 * (idx % 2), c, h, w, f, k, s, p, act))
    # 128-wide tiles (more than 64 channels / pixels), several channel blocks, s > k with a crop
    cases += [(2, 70, 9, 11, 130, 3, 2, 1, ACTS["relu"]), (3, 129, 6, 6, 66, 4, 2, 1, ACTS["logistic"]),
              (1, 64, 12, 10, 64, 2, 2, 0, ACTS["none"]), (2, 33, 7, 5, 40, 2, 3, 1, ACTS["lrelu"])]
    return cases


@pytest.mark.parametrize("n,c,h,w,f,k,s,p,act", _grid())
def test_ops_match_fp64_restatement(n, c, h, w, f, k, s, p, act):
    inp, got = _run_op(n, c, h, w, f, k, s, p, act, seed=n * 1000 + k * 100 + s * 10 + p)
    y_ref = np_forward(inp["x"], inp["wt"], inp["b"], k, s, p, act)
    _close("y", got["y"], y_ref)
    # the activation backward is evaluated at the output the forward wrote (reference :203-206)
    g_ref = inp["dy"] * _act_grad(got["y"], act)
    _close("dy * act'(y)", got["g"], g_ref)
    dw_ref, dx_ref = np_backward(inp["x"], inp["wt"], g_ref, k, s, p)
    _close("dw", got["dw"], inp["dw0"] + dw_ref / n)
    _close("db", got["db"], inp["db0"] + g_ref.sum(axis=(0, 2, 3)))
    _close("dx", got["dx"], dx_ref)


@pytest.mark.parametrize("k,s,p", [(4, 2, 1), (3, 2, 1), (5, 3, 2), (3, 1, 1), (2, 3, 1), (5, 1, 2)])
def test_padded_matches_torch_conv_transpose2d(k, s, p):
    n, c, h, w, f = 3, 6, 5, 7, 10
    inp, got = _run_op(n, c, h, w, f, k, s, p, ACTS["none"], seed=17 + k + s + p)
    x = torch.tensor(inp["x"], requires_grad=True)
    wt = torch.tensor(inp["wt"], requires_grad=True)
    b = torch.tensor(inp["b"], requires_grad=True)
    y = torch.nn.functional.conv_transpose2d(x, wt, b, stride=s, padding=p)
    _close("y", got["y"], y.detach().numpy())
    y.backward(torch.tensor(inp["dy"]))
    _close("dx", got["dx"], x.grad.numpy())
    _close("dw", got["dw"], inp["dw0"] + wt.grad.numpy() / n)
    _close("db", got["db"], inp["db0"] + b.grad.numpy())


def test_weight_gradient_is_bit_identical_across_runs():
    shape = (8, 48, 16, 16, 40, 4, 2, 1)  # K = 2048 pixels per tap: split into several chunks
    from bcnn_amd import ops
    assert ops.deconv_workspace_size(*shape) > 48 * 40 * 16
    runs = [_run_op(*shape, act=ACTS["relu"], seed=3)[1] for _ in range(2)]
    for key in ("y", "g", "dw", "db", "dx"):
        assert np.array_equal(runs[0][key], runs[1][key]), key


def test_weight_gradient_takes_a_one_split_workspace():
    """K = 2 * 9 * 11 = 198 pixels per tap: the full workspace splits it four ways (chunks of 64, the last one 6 long); a
    workspace of one split clamps the plan to a single chunk of 208, and the result is the same sum"""
    from bcnn_amd import ops
    n, c, h, w, f, k, s, p = shape = (2, 70, 9, 11, 130, 3, 2, 1)
    act = ACTS["relu"]
    per_split = k * k * c * f
    assert ops.deconv_workspace_size(*shape) == 4 * per_split
    inp, got = _run_op(*shape, act=act, seed=21, ws_elems=per_split)
    _close("y", got["y"], np_forward(inp["x"], inp["wt"], inp["b"], k, s, p, act))
    g_ref = inp["dy"] * _act_grad(got["y"], act)
    _close("dy * act'(y)", got["g"], g_ref)
    dw_ref, dx_ref = np_backward(inp["x"], inp["wt"], g_ref, k, s, p)
    _close("dw", got["dw"], inp["dw0"] + dw_ref / n)
    _close("db", got["db"], inp["db0"] + g_ref.sum(axis=(0, 2, 3)))
    _close("dx", got["dx"], dx_ref)


def test_backward_without_data_gradient():
    inp, got = _run_op(2, 5, 6, 6, 7, 3, 2, 0, ACTS["none"], seed=9, with_dx=False)
    dw_ref, _ = np_backward(inp["x"], inp["wt"], inp["dy"], 3, 2, 0)
    _close("dw", got["dw"], inp["dw0"] + dw_ref / 2)


# ---- the node against the reference -------------------------------------------------------------------------------
def _ref_deconv(ref, f, k, s, p, act, src, dst, init=rb.FILLER_XAVIER):
    st = ref.L.bcnn_add_deconvolutional_layer(ref.net, f, k, s, p, init, act, src.encode(), dst.encode())
    assert st == 0, st
    return ref.num_nodes() - 1


def _bind_ref():
    D.need_ref()
    L = D.ref_lib()
    vp, i, cp = C.c_void_p, C.c_int, C.c_char_p
    L.bcnn_add_deconvolutional_layer.argtypes = [vp, i, i, i, i, i, i, cp, cp]
    L.bcnn_add_deconvolutional_layer.restype = i
    L.bcnn_add_cost_layer.argtypes = [vp, i, i, C.c_float, cp, cp, cp]
    return L


def _graph(net, deconv):
    """conv -> deconv k4 s2 -> deconv k2 s3 (phases without taps) -> euclidean cost"""
    net.conv(6, 3, 1, 1, 1, 0, rb.ACT_RELU, "input", "c1")
    deconv(net, 5, 4, 2, 0, rb.ACT_LRELU, "c1", "d1")
    deconv(net, 4, 2, 3, 0, rb.ACT_LOGISTIC, "d1", "d2")
    net.cost("d2", "label", "cost", 1.0)


def _compare(tag, a, b, tol=NET_TOL, floor=1e-7):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a64.shape == b64.shape, (tag, a64.shape, b64.shape)
    diff = float(np.max(np.abs(a64 - b64)))
    bound = tol * float(np.max(np.abs(b64))) + floor
    assert diff <= bound, "%s: max abs diff %.3g > %.3g" % (tag, diff, bound)


def test_net_sgd_steps_and_model_file_match_reference(tmp_path):
    from bcnn_amd import capi
    _bind_ref()
    shp = dict(w=7, h=6, c=3, n=3)
    C.CDLL(None).srand(20240611)
    ref = rb.RefNet(mode=rb.MODE_TRAIN, **shp)
    ref.L.ref_set_threads(ref.net, 4)
    _graph(ref, lambda net, *a: _ref_deconv(net, *a))
    C.CDLL(None).srand(20240611)
    hip = capi.Net(mode=capi.MODE_TRAIN, **shp)
    _graph(hip, lambda net, f, k, s, p, act, src, dst: net.deconv(f, k, s, p, act=act, src=src, dst=dst))
    ref.compile()
    hip.compile()
    nt = ref.L.ref_num_tensors(ref.net)
    names = [ref.L.ref_tensor_name(ref.net, i).decode() for i in range(nt)]
    assert ref.shape(ref.index("d2")) == hip.shape(hip.index("d2")) == (3, 4, 41, 47)
    # the filler: same srand, same draws (weights [c_in][f][k][k] as one vector)
    for name in ("c1_w", "d1_w"):
        i = ref.index(name)
        assert hip.shape(i) == ref.shape(i) == (1, 1, 1, {"c1_w": 6 * 5 * 16, "d1_w": 5 * 4 * 4}[name])
        hip.download(i)
        np.testing.assert_allclose(hip.data(i), ref.data(i), rtol=1e-6, atol=0, err_msg=name)
    ref.L.bcnn_set_sgd_optimizer(ref.net, 0.01, 0.9)
    ref.L.bcnn_set_weight_regularizer(ref.net, 5e-4)
    hip.set_sgd(0.01, 0.9, 5e-4)
    rs = np.random.RandomState(7)
    for i in range(2, nt):
        d = ref.data(i)
        if names[i].endswith("_b"):
            d[...] = rs.uniform(-0.2, 0.2, d.shape)
        hip.data(i)[...] = d
        hip.upload(i)
    for idx in (0, 1):
        v = rs.uniform(-1, 1, ref.shape(idx)).astype(np.float32) if idx == 0 else \
            rs.uniform(0, 1, ref.shape(idx)).astype(np.float32)
        ref.data(idx)[...] = v
        hip.data(idx)[...] = v
        hip.upload(idx)
    for it in range(2):  # the second step runs on updated weights and the momentum carry
        ref.forward()
        hip.forward()
        ref.backward()
        hip.backward()
        for i in range(nt):
            hip.download(i)
            _compare("it%d %s data" % (it, names[i]), hip.data(i), ref.data(i))
            if ref.grad(i) is not None and i != 1:
                _compare("it%d %s grad" % (it, names[i]), hip.grad(i), ref.grad(i))
        ref.L.bcnn_update(ref.net)
        hip.update()
        for i in range(2, nt):
            hip.download(i)
            _compare("it%d %s data after update" % (it, names[i]), hip.data(i), ref.data(i))
    # model file: with the same parameter values both libraries write the same bytes
    for i in range(2, nt):
        if names[i].endswith(("_w", "_b")):
            hip.download(i)
            ref.data(i)[...] = hip.data(i)
    pr, ph = str(tmp_path / "ref.bcnnmodel"), str(tmp_path / "hip.bcnnmodel")
    assert ref.save_weights(pr) == 0 and hip.save_weights(ph) == 0
    assert open(pr, "rb").read() == open(ph, "rb").read()
    # ... and loading it restores them in a fresh net
    fresh = capi.Net(mode=capi.MODE_TRAIN, **shp)
    _graph(fresh, lambda net, f, k, s, p, act, src, dst: net.deconv(f, k, s, p, act=act, src=src, dst=dst))
    fresh.compile()
    assert fresh.load_weights(ph) == 0
    for i in range(2, nt):
        if names[i].endswith(("_w", "_b")):
            fresh.download(i)
            assert np.array_equal(fresh.data(i), hip.data(i)), names[i]
    fresh.close()
    ref.close()
    hip.close()


ADAM_CFG = """
[network]
input_width=6
input_height=5
input_channels=3
batch_size=2
optimizer=adam
learning_rate=0.01
momentum=0.9
decay=0.0005
beta1=0.9
beta2=0.999

[convolutional]
filters=4
size=3
stride=1
pad=1
function=relu
src=input
dst=conv1

[deconv]
filters=5
size=3
stride=2
pad=0
function=relu
src=conv1
dst=up1

[cost]
src=up1
dst=out
loss=euclidean
metric=error
"""


def test_ini_deconv_section_and_adam_match_reference(tmp_path):
    from bcnn_amd import capi
    _bind_ref()
    cfg = tmp_path / "deconv.conf"
    cfg.write_text(ADAM_CFG)
    C.CDLL(None).srand(20240612)
    ref, st_ref, raw, st = load_both(str(cfg), None, rb.MODE_TRAIN)
    assert st_ref == 0 and st == 0
    nt = same_graph(ref, raw)
    assert ref.shape(ref.index("up1")) == (2, 5, 11, 13)
    assert ref.L.bcnn_compile_net(ref.net) == 0 and raw.L.bcnn_compile_net(raw.net) == 0
    hip = capi.Net.__new__(capi.Net)
    hip.L, hip.net = raw.L, raw.net
    names = [ref.L.ref_tensor_name(ref.net, i).decode() for i in range(nt)]
    params = [i for i in range(2, nt) if names[i].endswith(("_w", "_b"))]
    assert len(params) == 4
    rs = np.random.RandomState(11)
    for i in params:
        if names[i].endswith("_b"):
            ref.data(i)[...] = rs.uniform(-0.2, 0.2, ref.shape(i))
        hip.data(i)[...] = ref.data(i)
        hip.upload(i)
    for step in range(3):
        for idx in (0, 1):
            v = rs.uniform(-1, 1, ref.shape(idx)).astype(np.float32)
            ref.data(idx)[...] = v
            hip.data(idx)[...] = v
            hip.upload(idx)
        ref.forward()
        hip.forward()
        ref.backward()
        hip.backward()
        ref.L.bcnn_update(ref.net)
        hip.update()
        for i in params:
            hip.download(i)
            _compare("step%d %s" % (step, names[i]), hip.data(i), ref.data(i))
            if names[i].endswith("_w"):  # Adam leaves the weight gradient zeroed (no momentum carry)
                assert not hip.grad(i).any() and not ref.grad(i).any(), names[i]
    hip.close()
    ref.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_net_unchanged():
    from bcnn_amd import capi
    hip = capi.Net(mode=capi.MODE_TRAIN, w=4, h=3, c=2, n=2)
    hip.conv(3, 3, 1, 1, act=capi.ACT_RELU, src="input", dst="c1")
    L = hip.L
    nodes = L.bcnn_get_num_nodes(hip.net)
    bad = [(4, 3, 2, 0, capi.ACT_PRELU),   # the reference passes NULL slopes
           (4, 2, 1, 2, capi.ACT_NONE),    # output height 1 * (3 - 1) + 2 - 4 = 0
           (4, 1, 1, 3, capi.ACT_NONE),    # output height 2 + 1 - 6 < 0
           (4, 0, 1, 0, capi.ACT_NONE),    # size < 1
           (4, 3, 0, 0, capi.ACT_NONE),    # stride < 1
           (0, 3, 1, 0, capi.ACT_NONE)]    # no filters
    for f, k, s, p, act in bad:
        st = L.bcnn_add_deconvolutional_layer(hip.net, f, k, s, p, capi.FILLER_XAVIER, act, b"c1", b"d")
        assert st != 0, (f, k, s, p, act)
        assert L.bcnn_get_num_nodes(hip.net) == nodes
        assert hip.index("d") < 0
    hip.deconv(4, 3, 2, 1, act=capi.ACT_RELU, src="c1", dst="d")
    hip.compile()
    assert hip.shape(hip.index("d")) == (2, 4, 5, 7)
    before = [hip.shape(i) for i in range(hip.index("d") + 1)]
    assert hip.resize(8, 6, 2) != 0
    assert [hip.shape(i) for i in range(hip.index("d") + 1)] == before
    hip.close()
