"""The bilinear interpolation node inside nets (bcnn_amd.capi): a small segmentation head, built by builder calls and from
an INI string,

    input 2x3x17x17 -> conv 3x3 (8) -> dilated conv 3x3 d2 (8, groups 2, ReLU) -> conv 1x1 (5)
                    -> interp zoom 4, align_corners (65x65) -> softmax over the channels of every pixel
                    -> Euclidean cost on a dense one-hot label,

against the same graph in torch float64 on the net's own weights, at the project's parity bar (1e-4 of the tensor's
maximum, tests/test_net_parity.py): the interp output, the softmax output and the gradient arriving at the first
convolution's output. The softmax node passes its gradient through and the cost node leaves p - y (bcnn_layers_next.c),
so p - y is what arrives at the interp output.

Then: the add form against the overwrite form when the interp's source has a second consumer, PREDICT == TRAIN forward,
bcnn_resize_net through the scale and the fixed form (and still refused next to a dilated node), the node type, and a
model file round trip with the node in the graph."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
NET_TOL = 1e-4  # tests/test_net_parity.py
SEED = 20261020
SHP = dict(w=17, h=17, c=3, n=2)
CLASSES = 5


def _trace(on):
    from bcnn_amd import _lib
    L = _lib.load()
    if on:
        L.bcnn_hip_trace_enable(1)
        return None
    n = L.bcnn_hip_trace_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return buf.value.decode().split()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def _compare(tag, a, b, tol=NET_TOL):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a64.shape == b64.shape, (tag, a64.shape, b64.shape)
    assert np.isfinite(a64).all(), tag
    diff = float(np.max(np.abs(a64 - b64)))
    print("%s: max abs diff %.3g of max %.3g" % (tag, diff, float(np.max(np.abs(b64)))))
    assert diff <= tol * float(np.max(np.abs(b64))) + 1e-7, "%s: max abs diff %.3g" % (tag, diff)


def _data(net, idx):
    net.download(idx, False)
    return net.data(idx).copy()


def _grad(net, idx):
    net.download(idx, True)
    return net.grad(idx).copy()


def _head(mode, side=False, seed=SEED):
    """the segmentation head by builder calls; side: a second consumer of the interp's source, outside the loss"""
    from bcnn_amd import capi
    C.CDLL(None).srand(seed)   # the fillers draw from rand()
    net = capi.Net(mode=mode, **SHP)
    net.conv(8, 3, 1, 1, act=capi.ACT_NONE, src="input", dst="c1")
    net.dilated_conv(8, 3, 1, 2, 2, g=2, act=capi.ACT_RELU, src="c1", dst="dc")
    net.conv(CLASSES, 1, 1, 0, act=capi.ACT_NONE, src="dc", dst="c3")
    node = net.interp("c3", "up", zoom=4, align_corners=True)
    if side:
        net.pool2d("avg", 2, 2, 0, src="c3", dst="side")
    net.softmax("up", "sm")
    net.cost("sm", "label", "cost")
    net.compile()
    return net, node


HEAD_CFG = """
[net]
input_width=17
input_height=17
input_channels=3
batch_size=2

[conv]
filters=8
size=3
stride=1
pad=1
activation=linear
src=input
dst=c1

[conv]
filters=8
size=3
stride=1
pad=2
dilation=2
groups=2
activation=relu
src=c1
dst=dc

[conv]
filters=5
size=1
stride=1
pad=0
activation=linear
src=dc
dst=c3

[%s]
zoom=4
align_corners=1
src=c3
dst=up

[softmax]
src=up
dst=sm

[cost]
src=sm
dst=cost
"""


def _feed(net, seed=7):
    rs = np.random.RandomState(seed)
    for node in range(3):   # non-trivial biases (the builders fill 0)
        i = net.node_src(node, 2)
        net.data(i)[...] = rs.uniform(-0.5, 0.5, net.shape(i))
        net.upload(i)
    net.data(0)[...] = rs.uniform(-1, 1, net.shape(0))
    net.upload(0)
    if net.tensor(1).data:
        n, k, h, w = net.shape(1)
        lab = np.zeros((n, k, h, w), np.float32)
        cls = rs.randint(0, k, (n, h, w))
        np.put_along_axis(lab, cls[:, None], 1.0, axis=1)   # a dense one-hot label: one class per pixel
        net.data(1)[...] = lab
        net.upload(1)


def _torch_head(net):
    """the same graph in float64 on the net's weights: (up, softmax, gradient at c1)"""
    t = lambda i: torch.tensor(_data(net, i), dtype=torch.float64)
    w = [t(net.node_src(k, 1)) for k in range(3)]
    b = [t(net.node_src(k, 2)).reshape(-1) for k in range(3)]
    x, label = t(0), t(1)
    c1 = F.conv2d(x, w[0].reshape(8, 3, 3, 3), b[0], padding=1).requires_grad_(True)
    dc = F.relu(F.conv2d(c1, w[1].reshape(8, 4, 3, 3), b[1], padding=2, dilation=2, groups=2))
    c3 = F.conv2d(dc, w[2].reshape(CLASSES, 8, 1, 1), b[2])
    up = F.interpolate(c3, size=(65, 65), mode="bilinear", align_corners=True)
    p = F.softmax(up, dim=1)
    up.backward((p - label).detach())
    return up.detach().numpy(), p.detach().numpy(), c1.grad.numpy()


@pytest.mark.parametrize("how", ["builders", "ini-interp", "ini-bilinear"])
def test_segmentation_head_against_torch(tmp_path, how):
    from bcnn_amd import capi
    if how == "builders":
        net, node = _head(capi.MODE_TRAIN)
    else:
        cfg = tmp_path / "head.cfg"
        cfg.write_text(HEAD_CFG % how[4:])
        C.CDLL(None).srand(SEED)
        net, node = capi.Net.load_net(str(cfg), None, mode=capi.MODE_TRAIN), 3
        net.compile()
    assert net.num_nodes == 6 and net.node_type(node) == capi.LAYER_INTERP == 21
    up, sm, c1 = net.index("up"), net.index("sm"), net.index("c1")
    assert net.node_src(node, 0) == net.index("c3") and net.node_dst(node) == up
    assert net.shape(up) == (2, CLASSES, 65, 65) == net.shape(1)
    from bcnn_amd import ops
    assert ops.interp_out_hw(17, 17, zoom=4) == (65, 65)   # the Python restatement of the extent rule follows the builder
    _feed(net)
    _trace(True)
    net.forward()
    net.backward()
    net.sync()
    ran = _trace(False)
    assert "interp_fwd_kernel" in ran, ran                 # 65 columns: scalar stores
    assert "interp_bwd_kernel:overwrite" in ran, ran       # the node is the only writer of c3's gradient
    assert "interp_bwd_kernel" not in ran, ran
    want_up, want_sm, want_c1 = _torch_head(net)
    _compare("interp output", _data(net, up), want_up)
    _compare("softmax output", _data(net, sm), want_sm)
    _compare("gradient at the first convolution's output", _grad(net, c1), want_c1)
    if how != "builders":   # the file builds the graph the builder calls build: the same bits on the same weights
        twin, _ = _head(capi.MODE_TRAIN)
        _feed(twin)
        twin.forward()
        twin.backward()
        twin.sync()
        assert np.array_equal(_bits(_data(net, up)), _bits(_data(twin, up)))
        assert np.array_equal(_bits(_grad(net, c1)), _bits(_grad(twin, c1)))
        twin.close()
    net.close()


def test_second_consumer_selects_the_add_form():
    """with a second node reading c3 the interp node is not the only writer of c3's gradient: the executor zero-fills it
    and the node adds. The side branch is outside the loss, so its gradient is zero and both forms must give the same
    gradient at c3 and below, bit for bit (0 + g and g + 0 are exact)."""
    from bcnn_amd import capi
    got = {}
    for side in (False, True):
        net, node = _head(capi.MODE_TRAIN, side=side)
        _feed(net)
        _trace(True)
        net.forward()
        net.backward()
        net.sync()
        ran = _trace(False)
        assert ("interp_bwd_kernel" in ran) == side and ("interp_bwd_kernel:overwrite" in ran) == (not side), ran
        got[side] = (_grad(net, net.index("c3")), _grad(net, net.index("c1")))
        net.close()
    assert np.abs(got[False][0]).max() > 0
    for a, b in zip(got[False], got[True]):
        assert np.array_equal(_bits(a), _bits(b))


def test_predict_forward_is_the_train_forward():
    from bcnn_amd import capi
    outs = {}
    for mode in (capi.MODE_TRAIN, capi.MODE_PREDICT):
        net, node = _head(mode)
        _feed(net)
        net.forward()
        net.sync()
        outs[mode] = _data(net, net.index("up"))
        net.close()
    assert np.abs(outs[capi.MODE_TRAIN]).max() > 0
    assert np.array_equal(_bits(outs[capi.MODE_TRAIN]), _bits(outs[capi.MODE_PREDICT]))


def _tail(w, h, n):
    """conv -> interp scale 2, and the same conv -> interp fixed 40 x 40"""
    from bcnn_amd import capi
    C.CDLL(None).srand(SEED)
    net = capi.Net(mode=capi.MODE_TRAIN, w=w, h=h, c=3, n=n)
    net.conv(4, 3, 1, 1, act=capi.ACT_RELU, src="input", dst="c1")
    net.interp("c1", "u2", scale=2)
    net.interp("c1", "uf", out_w=40, out_h=40, align_corners=True)
    net.compile()
    return net


def test_resize_follows_the_scale_form_and_keeps_the_fixed_form():
    from bcnn_amd import capi
    net = _tail(17, 17, 2)
    assert net.shape(net.index("u2")) == (2, 4, 34, 34) and net.shape(net.index("uf")) == (2, 4, 40, 40)
    assert net.resize(21, 21, 3, need_realloc=True) == 0
    fresh = _tail(21, 21, 1)
    x = np.random.RandomState(3).uniform(-1, 1, (1, 3, 21, 21))
    from bcnn_amd import ops
    for t in (net, fresh):
        assert t.shape(t.index("u2")) == (1, 4, 42, 42) and t.shape(t.index("uf")) == (1, 4, 40, 40)
        assert t.shape(t.index("u2"))[2:] == ops.interp_out_hw(21, 21, scale=2)   # the Python restatement follows
        assert t.shape(t.index("uf"))[2:] == ops.interp_out_hw(21, 21, out_h=40, out_w=40)
        t.data(0)[...] = x
        t.upload(0)
        t.forward()
        t.backward()   # in bounds on the re-allocated tensors
        t.sync()
    for name in ("u2", "uf"):
        a, b = _data(net, net.index(name)), _data(fresh, fresh.index(name))
        assert np.abs(b).max() > 0 and np.array_equal(_bits(a), _bits(b)), name
    net.close()
    fresh.close()
    # a graph that holds a dilated node is refused as before, and left as it was
    head, node = _head(capi.MODE_TRAIN)
    assert head.resize(21, 21, 3, need_realloc=True) == 1   # BCNN_INVALID_PARAMETER
    assert head.shape(0) == (2, 3, 17, 17) and head.shape(head.index("up")) == (2, CLASSES, 65, 65)
    head.close()


def test_model_file_round_trip_with_the_node_in_the_graph(tmp_path):
    from bcnn_amd import capi
    a, _ = _head(capi.MODE_TRAIN)
    _feed(a)
    a.forward()
    a.sync()
    path = str(tmp_path / "head.bcnnmodel")
    assert a.save_weights(path) == 0
    b, node = _head(capi.MODE_TRAIN, seed=SEED + 1)   # other weights, until the file is loaded
    assert b.node_type(node) == capi.LAYER_INTERP
    assert b.load_weights(path) == 0
    b.data(0)[...] = a.data(0)   # the input alone: weights and biases came from the file
    b.upload(0)
    b.forward()
    b.sync()
    for name in ("c3", "up"):
        assert np.array_equal(_bits(_data(a, a.index(name))), _bits(_data(b, b.index(name)))), name
    a.close()
    b.close()
