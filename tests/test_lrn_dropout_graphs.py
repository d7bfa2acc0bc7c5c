"""LRN and dropout nodes inside TRAIN graphs, against the unmodified reference (oracle/_ref/libbcnn_ref.so):
  - an AlexNet-shaped net (conv -> LRN -> maxpool -> conv+BN -> dropout -> fc -> dropout -> fc -> softmax -> cost) at
    dropout rate 0: filler, SGD steps and the model file. LRN runs with alpha = beta = 0, where it is the identity; the
    reference graph leaves the LRN node out, because its LRN backward divides by its never-stored k = 0 (NaN);
  - rate 0.5: every node but dropout is the reference's own worker, the reference tensor is masked with this build's
    mask (NumPy), node by node. This pins the in-place contract: a producer's backward sees the post-dropout output
    (logistic conv+BN and fc producers), and no fusion link fires across a dropout node (maxpool, eltwise, depthwise);
  - bcnn_resize_net on a net holding both nodes, and the model file skipping them."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_bind as rb
from tests.test_dropout import dropout_key, np_dropout
from tests.test_lrn import np_lrn, np_lrn_backward

pytestmark = pytest.mark.gpu
NET_TOL = 1e-4  # tests/test_net_parity.py


def _bind_ref():
    L = rb.lib()
    L.bcnn_add_dropout_layer.argtypes = [C.c_void_p, C.c_float, C.c_char_p]
    L.bcnn_add_dropout_layer.restype = C.c_int
    return L


def _compare(tag, a, b, tol=NET_TOL):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a64.shape == b64.shape, (tag, a64.shape, b64.shape)
    assert np.isfinite(a64).all(), tag
    diff = float(np.max(np.abs(a64 - b64))) if a64.size else 0.0
    assert diff <= tol * float(np.max(np.abs(b64))) + 1e-7, "%s: max abs diff %.3g" % (tag, diff)


def _alexnet(net, is_ref, rate, act2=rb.ACT_RELU, act_f1=rb.ACT_RELU, tail="pool"):
    """returns the node index of each dropout node in `net`"""
    drops = []
    net.conv(6, 3, 1, 1, act=rb.ACT_RELU, src="input", dst="c1")
    if is_ref:
        first = "c1"
    else:
        net.lrn(3, 0.0, 0.0, 1.0, src="c1", dst="n1")
        first = "n1"
    net.maxpool(2, 2, src=first, dst="p1")
    net.conv(8, 3, 1, 1, bn=1, act=act2 if tail != "elt" else rb.ACT_NONE, src="p1", dst="c2")
    drops.append(_dropout(net, is_ref, rate, "c2"))
    if tail == "pool":
        net.maxpool(2, 2, src="c2", dst="t1")
    elif tail == "elt":
        net.conv(8, 1, 1, 0, act=rb.ACT_RELU, src="p1", dst="c3")
        net.eltwise(rb.ACT_RELU, "c2", "c3", "t1")
    else:
        net.depthwise(3, 1, 1, act=rb.ACT_RELU, src="c2", dst="t1")
    net.fullc(24, act=act_f1, src="t1", dst="f1")
    drops.append(_dropout(net, is_ref, rate, "f1"))
    net.fullc(5, src="f1", dst="f2")
    net.softmax("f2", "sm")
    net.cost("sm", "label", "cost")
    return drops


def _dropout(net, is_ref, rate, src):
    if is_ref:
        assert net.L.bcnn_add_dropout_layer(net.net, rate, src.encode()) == 0
        return net.L.ref_num_nodes(net.net) - 1
    return net.dropout(rate, src)


def _pair(rate, seed, shp, **kw):
    from bcnn_amd import capi
    _bind_ref()
    C.CDLL(None).srand(seed)
    ref = rb.RefNet(mode=rb.MODE_TRAIN, **shp)
    ref.L.ref_set_threads(ref.net, 4)
    ref_drops = _alexnet(ref, True, rate, **kw)
    C.CDLL(None).srand(seed)
    hip = capi.Net(mode=capi.MODE_TRAIN, **shp)
    hip_drops = _alexnet(hip, False, rate, **kw)
    hip.L.bcnn_set_dropout_seed(hip.net, seed)
    ref.compile()
    hip.compile()
    rnames = [ref.L.ref_tensor_name(ref.net, i).decode() for i in range(ref.L.ref_num_tensors(ref.net))]
    assert hip.index("n1") == ref.index("c1") + 1
    return ref, hip, rnames, ref_drops, hip_drops


def _hip_idx(ref, i):
    """this build's tensor for reference tensor i: the same list with the LRN output inserted behind c1"""
    return i if i <= ref.index("c1") else i + 1


def _feed(ref, hip, rnames, rs):
    for i, name in enumerate(rnames):
        if name.endswith("_b"):
            ref.data(i)[...] = rs.uniform(-0.2, 0.2, ref.shape(i))
        if name.endswith(("_w", "_b", "_scales")) or i <= 1:
            if i == 0:
                ref.data(i)[...] = rs.uniform(-1, 1, ref.shape(i))
            elif i == 1:
                lab = np.zeros(ref.shape(i), np.float32)
                lab.reshape(lab.shape[0], -1)[np.arange(lab.shape[0]), rs.randint(0, 5, lab.shape[0])] = 1
                ref.data(i)[...] = lab
            j = _hip_idx(ref, i)
            hip.data(j)[...] = ref.data(i)
            hip.upload(j)


def test_alexnet_rate0_matches_reference(tmp_path):
    shp = dict(w=12, h=12, c=3, n=4)
    ref, hip, rnames, _, _ = _pair(0.0, 20260101, shp)
    for i, name in enumerate(rnames):  # the filler: LRN and dropout draw nothing
        if name.endswith("_w"):
            j = _hip_idx(ref, i)
            hip.download(j)
            np.testing.assert_allclose(hip.data(j), ref.data(i), rtol=1e-6, atol=0, err_msg=name)
    ref.L.bcnn_set_sgd_optimizer(ref.net, 0.01, 0.9)
    ref.L.bcnn_set_weight_regularizer(ref.net, 5e-4)
    hip.set_sgd(0.01, 0.9, 5e-4)
    rs = np.random.RandomState(3)
    _feed(ref, hip, rnames, rs)
    for it in range(3):
        ref.forward()
        hip.forward()
        ref.backward()
        hip.backward()
        for i, name in enumerate(rnames):
            j = _hip_idx(ref, i)
            hip.download(j)
            _compare("it%d %s" % (it, name), hip.data(j), ref.data(i))
            if ref.grad(i) is not None and i > 1:
                _compare("it%d d%s" % (it, name), hip.grad(j), ref.grad(i))
        ref.L.bcnn_update(ref.net)
        hip.update()
    outputs = {ref.node_dst(k) for k in range(ref.L.ref_num_nodes(ref.net))}
    for i, name in enumerate(rnames):  # parameters and batch-norm running statistics
        if i > 1 and i not in outputs:
            j = _hip_idx(ref, i)
            hip.download(j)
            _compare("final %s" % name, hip.data(j), ref.data(i))
            ref.data(i)[...] = hip.data(j)
    pr, ph = str(tmp_path / "ref.bcnnmodel"), str(tmp_path / "hip.bcnnmodel")
    assert ref.save_weights(pr) == 0 and hip.save_weights(ph) == 0
    assert open(pr, "rb").read() == open(ph, "rb").read()
    assert hip.load_weights(ph) == 0
    ref.close()
    hip.close()


def _teacher_forced_ref(ref, rnames, hip_drops, ref_drops, seed, step, rate):
    """one reference TRAIN forward + backward, node by node, its dropout nodes replaced by this build's mask"""
    L = ref.L
    nn = L.ref_num_nodes(ref.net)
    key = {r: dropout_key(seed, h) for r, h in zip(ref_drops, hip_drops)}
    for i in range(nn):
        t = L.ref_node_dst(ref.net, i, 0)  # bcnn_reset_gradients (reference bcnn_net.c:413-415)
        if ref.grad(t) is not None:
            ref.grad(t)[...] = 0
        if i in key:
            t = L.ref_node_src(ref.net, i, 0)
            ref.data(t)[...] = np_dropout(ref.data(t).copy(), rate, key[i], step)
        else:
            L.ref_forward_node(ref.net, i)
    for i in reversed(range(nn)):
        if i in key:
            t = L.ref_node_src(ref.net, i, 0)
            ref.grad(t)[...] = np_dropout(ref.grad(t).copy(), rate, key[i], step)
        else:
            L.ref_backward_node(ref.net, i)


@pytest.mark.parametrize("act2,act_f1,tail", [(rb.ACT_RELU, rb.ACT_RELU, "pool"),
                                              (rb.ACT_LOGISTIC, rb.ACT_LOGISTIC, "pool"),
                                              (rb.ACT_RELU, rb.ACT_LOGISTIC, "elt"),
                                              (rb.ACT_LRELU, rb.ACT_RELU, "dw"),
                                              (rb.ACT_TANH, rb.ACT_TANH, "dw")])
def test_rate_half_teacher_forced_against_reference(act2, act_f1, tail):
    shp = dict(w=12, h=12, c=3, n=4)
    seed, rate = 77, 0.5
    ref, hip, rnames, ref_drops, hip_drops = _pair(rate, seed, shp, act2=act2, act_f1=act_f1, tail=tail)
    rs = np.random.RandomState(5)
    _feed(ref, hip, rnames, rs)
    for step in range(2):
        _teacher_forced_ref(ref, rnames, hip_drops, ref_drops, seed, step, rate)
        hip.forward()
        hip.backward()
        for i, name in enumerate(rnames):
            j = _hip_idx(ref, i)
            hip.download(j)
            _compare("step%d %s" % (step, name), hip.data(j), ref.data(i))
            if ref.grad(i) is not None and i > 1:
                _compare("step%d d%s" % (step, name), hip.grad(j), ref.grad(i))
        for i, name in enumerate(rnames):  # the parameter gradients accumulate: start the next step from zero
            if ref.grad(i) is not None and i > 1:
                j = _hip_idx(ref, i)
                ref.grad(i)[...] = 0
                hip.grad(j)[...] = 0
                hip.upload(j, with_grad=True)
    ref.close()
    hip.close()


def test_resize_net_with_lrn_and_dropout():
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=6, h=5, c=7, n=1)
    net.conv(7, 1, 1, 0, src="input", dst="c0")
    net.lrn(5, 0.3, 0.75, 1.5, src="c0", dst="n1")
    net.dropout(0.25, "n1")
    net.L.bcnn_set_dropout_seed(net.net, 9)
    net.compile()
    assert net.resize(11, 9, 7) == 0
    c0, i = net.index("c0"), net.index("n1")
    assert net.shape(i) == net.shape(c0) == (1, 7, 9, 11)
    rs = np.random.RandomState(8)
    net.data(0)[...] = rs.uniform(-2, 2, net.shape(0))
    net.upload(0)
    net.forward()
    net.download(c0)
    net.download(i)
    x = net.data(c0).copy()
    y = np_dropout(np_lrn(x, 5, 0.3, 0.75, 1.5)[0].astype(np.float32), 0.25, dropout_key(9, 2), 0)
    dropped = y == 0
    np.testing.assert_allclose(net.data(i), y, rtol=1e-5, atol=1e-6)
    dy = rs.uniform(-1, 1, x.shape).astype(np.float32)
    net.grad(i)[...] = dy
    net.upload(i, with_grad=True)
    net.backward()
    net.download(c0)
    want = np_lrn_backward(x, np.where(dropped, 0, dy / np.float32(0.75)), 5, 0.3, 0.75, 1.5)
    assert np.max(np.abs(net.grad(c0) - want)) <= 1e-5 * np.max(np.abs(want))
    net.close()
