"""Concat ([route]) and nearest-neighbour upsample against the unmodified reference (oracle/_ref/libbcnn_ref.so):
node-level forward and backward bit-exact (both are copies or single float adds in the reference CPU order), and a
TRAIN graph through forward / backward / SGD at the net-parity tolerance, in which concat also reads the output of a
convolution that a max-pooling node consumes -- the conv -> max-pool fusion link must not be taken for it."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from oracle import ref_bind as rb
from tests import _detect_ref as D

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4


def _pair(mode, shp, input_grad):
    from bcnn_amd import capi
    D.need_ref()
    D.ref_lib()
    ctypes.CDLL(None).srand(1234)
    ref = rb.RefNet(mode=mode, input_grad=input_grad, **shp)
    hip = capi.Net(mode=mode, input_grad=input_grad, **shp)
    return ref, hip


def _set(ref, hip, idx, rs, grad=False):
    """same random data (and gradient) in tensor idx on both sides"""
    d = rs.uniform(-1, 1, ref.shape(idx)).astype(np.float32)
    ref.data(idx)[...] = d
    hip.data(idx)[...] = d
    if grad and ref.grad(idx) is not None:
        g = rs.uniform(-1, 1, ref.shape(idx)).astype(np.float32)
        ref.grad(idx)[...] = g
        hip.grad(idx)[...] = g
    hip.upload(idx, with_grad=grad)


@pytest.mark.parametrize("hw", [(5, 7), (8, 8)])   # c*h*w % 4 != 0 (unaligned slices) and the 16-byte path
def test_concat_node_matches_reference_bit_exact(hw):
    h, w = hw
    shp = dict(w=w, h=h, c=3, n=3)
    ref, hip = _pair(rb.MODE_TRAIN, shp, input_grad=False)   # the input has no gradient: skipped by backward
    for net in (ref, hip):
        net.conv(5, 3, 1, 1, 1, 0, rb.ACT_NONE, "input", "c1")
        net.conv(2, 1, 1, 0, 1, 0, rb.ACT_NONE, "input", "c2")
    cats = [(["c1"], "cat1"), (["c1", "c2"], "cat2"), (["input", "c1", "c2"], "cat3"), (["c2", "input"], "cat4")]
    nodes = []
    for srcs, dst in cats:
        nodes.append(D.ref_concat(ref, srcs, dst))
        assert hip.concat(srcs, dst) == nodes[-1]
    ref.compile()
    hip.compile()
    rs = np.random.RandomState(5)
    for name in ("input", "c1", "c2"):
        _set(ref, hip, ref.index(name), rs, grad=True)
    assert ref.grad(ref.index("input")) is None and hip.grad(hip.index("input")) is None
    for node, (srcs, dst) in zip(nodes, cats):
        o = ref.index(dst)
        assert hip.shape(o) == ref.shape(o) == (3, sum(ref.shape(ref.index(s))[1] for s in srcs), h, w)
        ref.forward_node(node)
        hip.forward_node(node)
        hip.download(o, with_grad=False)
        np.testing.assert_array_equal(hip.data(o), ref.data(o), err_msg=dst)
        # backward from a non-zero source gradient: the add must be the reference's one float add per element
        _set(ref, hip, o, rs, grad=True)
        for s in ("c1", "c2"):
            _set(ref, hip, ref.index(s), rs, grad=True)
        ref.backward_node(node)
        hip.backward_node(node)
        for s in ("c1", "c2"):
            i = ref.index(s)
            hip.download(i)
            np.testing.assert_array_equal(hip.grad(i), ref.grad(i), err_msg="%s <- %s" % (s, dst))
    ref.close()
    hip.close()


@pytest.mark.parametrize("size,w", [(2, 8), (2, 7), (3, 7), (1, 5)])
def test_upsample_node_matches_reference_bit_exact(size, w):
    shp = dict(w=w, h=5, c=3, n=2)
    ref, hip = _pair(rb.MODE_TRAIN, shp, input_grad=False)
    for net in (ref, hip):
        net.conv(4, 3, 1, 1, 1, 0, rb.ACT_NONE, "input", "c1")
    node = D.ref_upsample(ref, size, "c1", "up")
    assert hip.upsample(size, "c1", "up") == node
    ref.compile()
    hip.compile()
    rs = np.random.RandomState(11)
    x, y = ref.index("c1"), ref.index("up")
    assert hip.shape(y) == ref.shape(y) == (2, 4, 5 * size, w * size)
    _set(ref, hip, x, rs, grad=True)   # non-zero dx: the gather starts from it
    ref.forward_node(node)
    hip.forward_node(node)
    hip.download(y, with_grad=False)
    np.testing.assert_array_equal(hip.data(y), ref.data(y))
    _set(ref, hip, y, rs, grad=True)
    ref.backward_node(node)
    hip.backward_node(node)
    hip.download(x)
    np.testing.assert_array_equal(hip.grad(x), ref.grad(x))
    ref.close()
    hip.close()


def _fpn_graph(net, concat):
    """conv+BN -> maxpool -> conv+BN -> upsample x2 -> concat with the first conv's output -> conv -> avgpool -> fc ->
    softmax -> cost (concat=False: the first conv's output goes straight on instead -- the control graph)"""
    net.conv(8, 3, 1, 1, 1, 1, rb.ACT_RELU, "input", "c1")
    net.maxpool(3, 2, rb.PADDING_SAME, "c1", "p1")
    net.conv(8, 3, 1, 1, 1, 1, rb.ACT_RELU, "p1", "c2")
    if concat:
        if isinstance(net, rb.RefNet):
            D.ref_upsample(net, 2, "c2", "u2")
            D.ref_concat(net, ["u2", "c1"], "cat")
        else:
            net.upsample(2, "c2", "u2")
            net.concat(["u2", "c1"], "cat")
        net.conv(8, 3, 1, 1, 1, 0, rb.ACT_RELU, "cat", "c3")
    else:
        net.conv(8, 3, 1, 1, 1, 0, rb.ACT_RELU, "c2", "c3")
    net.avgpool("c3", "avg")
    net.fullc(10, rb.ACT_NONE, "avg", "fc")
    net.softmax("fc", "sm")
    net.cost("sm", "label", "cost", 1.0)


def _compare(tag, a, b, tol=REL_TOL, floor=1e-7):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    diff = float(np.max(np.abs(a64 - b64)))
    bound = tol * float(np.max(np.abs(b64))) + floor
    assert diff <= bound, "%s: max abs diff %.3g > %.3g" % (tag, diff, bound)


def _trace(fn):
    from bcnn_amd import _lib
    L = _lib.load()
    L.bcnn_hip_trace_enable(1)  # clears the log
    fn()
    n = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return set(buf.value.decode().split())


def test_control_graph_takes_the_conv_maxpool_link():
    """without the concat the first conv's output has one consumer: the fused pooling kernel runs (so that the test
    below, which expects it NOT to run, is not vacuous)"""
    from bcnn_amd import capi
    hip = capi.Net(mode=capi.MODE_TRAIN, w=16, h=16, c=3, n=4)
    _fpn_graph(hip, concat=False)
    hip.compile()
    hip.data(0)[...] = np.random.RandomState(0).uniform(-1, 1, hip.shape(0)).astype(np.float32)
    hip.upload(0)
    ran = _trace(hip.forward)
    assert "maxpool_fwd_s2_bn_kernel" in ran, sorted(ran)
    hip.close()


def test_fpn_graph_matches_reference_and_blocks_the_link():
    shp = dict(w=16, h=16, c=3, n=4)
    ref, hip = _pair(rb.MODE_TRAIN, shp, input_grad=False)
    ref.L.ref_set_threads(ref.net, 4)
    _fpn_graph(ref, concat=True)
    _fpn_graph(hip, concat=True)
    ref.compile()
    hip.compile()
    ref.L.bcnn_set_sgd_optimizer(ref.net, 0.01, 0.9)
    ref.L.bcnn_set_weight_regularizer(ref.net, 5e-4)
    hip.set_sgd(0.01, 0.9, 5e-4)
    rs = np.random.RandomState(7)
    nt = ref.L.ref_num_tensors(ref.net)
    names = [ref.L.ref_tensor_name(ref.net, i).decode() for i in range(nt)]
    for i in range(2, nt):
        d = ref.data(i)
        if names[i].endswith("_scales") or names[i].endswith("_run_var"):
            d[...] = rs.uniform(0.5, 1.5, d.shape)
        elif names[i].endswith("_b"):
            d[...] = rs.uniform(-0.2, 0.2, d.shape)
        assert hip.shape(i) == ref.shape(i), names[i]
        hip.data(i)[...] = d
        hip.upload(i)
    x = rs.uniform(-1, 1, ref.shape(0)).astype(np.float32)
    ref.data(0)[...] = x
    hip.data(0)[...] = x
    hip.upload(0)
    lab = np.zeros(ref.shape(1), np.float32)
    for b in range(lab.shape[0]):
        lab[b, rs.randint(lab.shape[1])] = 1.0
    ref.data(1)[...] = lab
    hip.data(1)[...] = lab
    hip.upload(1)
    ran = set()
    for it in range(2):
        ref.forward()
        ref.backward()
        ran |= _trace(lambda: (hip.forward(), hip.backward()))
        for i in range(nt):
            if not ref.tensor(i).data:
                continue
            hip.download(i)
            _compare("it%d %s data" % (it, names[i]), hip.data(i), ref.data(i))
            if ref.grad(i) is not None and i != 1:
                _compare("it%d %s grad" % (it, names[i]), hip.grad(i), ref.grad(i))
        ref.L.bcnn_update(ref.net)
        hip.update()
        for i in range(2, nt):
            hip.download(i)
            _compare("it%d %s data after update" % (it, names[i]), hip.data(i), ref.data(i))
    # c1 feeds the max-pooling node AND the concat: the pooling kernel must not normalise c1 on the fly (c1 would stay
    # unwritten for the concat), and the pooling backward must not own c1's gradient alone
    assert "maxpool_fwd_s2_bn_kernel" not in ran and "maxpool_bwd_pair_bn_kernel" not in ran, sorted(ran)
    ref.close()
    hip.close()
