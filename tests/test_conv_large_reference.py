"""AlexNet's first two stages against the unmodified reference (oracle/_ref/libbcnn_ref.so, oracle/ref_bind.RefNet):
conv 11x11 / s4 + ReLU -> LRN -> maxpool 3 / s2 -> conv 5x5 p2 groups 2 -> fc -> softmax -> cost on a 67 x 67 input,
N = 4, the same parameters on both sides; one bcnn_forward + bcnn_backward + bcnn_update, every tensor and every
parameter after the update compared at the bar of tests/test_net_parity.py. As in tests/test_lrn_dropout_graphs.py the
LRN node runs with alpha = beta = 0, where it is the identity, and the reference graph leaves it out: the reference's LRN
backward divides by its never-stored k = 0 (NaN). Then the 11x11 node alone, teacher-forced through ref_forward_node /
ref_backward_node as tests/test_teacher_forced.py does, and a 9x9 layer with a fused batch-norm (the raw epilogue)."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from oracle import ref_bind as rb
from tests.test_net_parity import REL_TOL, _compare

pytestmark = pytest.mark.gpu

SHAPE = dict(w=67, h=67, c=3, n=4)


def _alexnet_stages(net, is_ref):
    net.conv(96, 11, 4, 0, 1, 0, rb.ACT_RELU, "input", "c1")
    first = "c1"
    if not is_ref:
        net.lrn(5, 0.0, 0.0, 1.0, src="c1", dst="n1")
        first = "n1"
    net.maxpool(3, 2, rb.PADDING_SAME, first, "p1")
    net.conv(256, 5, 1, 2, 2, 0, rb.ACT_RELU, "p1", "c2")
    net.fullc(10, rb.ACT_NONE, "c2", "fc")
    net.softmax("fc", "sm")
    net.cost("sm", "label", "cost", 1.0)


def _bn_graph(net, is_ref):
    net.conv(40, 9, 2, 4, 1, 1, rb.ACT_RELU, "input", "c1")
    net.conv(24, 8, 1, 3, 2, 1, rb.ACT_LRELU, "c1", "c2")
    net.avgpool("c2", "gap")
    net.fullc(10, rb.ACT_NONE, "gap", "fc")
    net.softmax("fc", "sm")
    net.cost("sm", "label", "cost", 1.0)


def _pair(graph, shape):
    from bcnn_amd import capi
    if not rb.available():
        pytest.skip("oracle/_ref/libbcnn_ref.so not present (built from the reference tree by oracle/Makefile)")
    ctypes.CDLL(None).srand(20240607)
    ref = rb.RefNet(mode=rb.MODE_TRAIN, input_grad=True, **shape)
    ref.L.ref_set_threads(ref.net, 4)
    hip = capi.Net(mode=capi.MODE_TRAIN, input_grad=True, **shape)
    graph(ref, True)
    graph(hip, False)
    ref.compile()
    hip.compile()
    nt = ref.L.ref_num_tensors(ref.net)
    names = [ref.L.ref_tensor_name(ref.net, i).decode() for i in range(nt)]
    to_hip = [hip.index(nm) for nm in names]
    assert all(j >= 0 for j in to_hip), list(zip(names, to_hip))
    rs = np.random.RandomState(7)
    for i in range(2, nt):  # the reference's (rand()-initialised) parameters on both sides
        if not ref.tensor(i).data:
            continue
        d = ref.data(i)
        if names[i].endswith("_scales"):
            d[...] = rs.uniform(0.5, 1.5, d.shape)
        elif names[i].endswith("_b"):
            d[...] = rs.uniform(-0.2, 0.2, d.shape)
        j = to_hip[i]
        assert hip.shape(j) == ref.shape(i), names[i]
        hip.data(j)[...] = d
        hip.upload(j)
    x = rs.uniform(-1, 1, ref.shape(0)).astype(np.float32)
    lab = np.zeros(ref.shape(1), np.float32)
    for b in range(lab.shape[0]):
        lab[b, rs.randint(lab.shape[1])] = 1.0
    for i, v in ((0, x), (1, lab)):
        ref.data(i)[...] = v
        hip.data(i)[...] = v
        hip.upload(i)
    return ref, hip, names, to_hip, rs


def _trace_set(L):
    n = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return set(buf.value.decode().split())


@pytest.mark.parametrize("gname", ["alexnet_stages", "fused_batchnorm"])
def test_one_training_step_matches_the_reference(gname):
    from bcnn_amd import _lib
    graph, shape = (_alexnet_stages, SHAPE) if gname == "alexnet_stages" else (_bn_graph, dict(w=31, h=26, c=3, n=6))
    ref, hip, names, to_hip, _ = _pair(graph, shape)
    ref.L.bcnn_set_sgd_optimizer(ref.net, 0.01, 0.9)
    ref.L.bcnn_set_weight_regularizer(ref.net, 5e-4)
    hip.set_sgd(0.01, 0.9, 5e-4)
    _lib.load().bcnn_hip_trace_enable(1)
    ref.forward()
    hip.forward()
    ref.backward()
    hip.backward()
    ran = _trace_set(_lib.load())
    assert {"conv_large_gemm_kernel:fwd", "conv_large_gemm_kernel:dx", "conv_large_dw_kernel"} <= ran, sorted(ran)
    for i, nm in enumerate(names):
        if not ref.tensor(i).data:
            continue
        hip.download(to_hip[i])
        _compare("%s %s data" % (gname, nm), hip.data(to_hip[i]), ref.data(i), REL_TOL)
        if ref.grad(i) is not None and i != 1:
            _compare("%s %s grad" % (gname, nm), hip.grad(to_hip[i]), ref.grad(i), REL_TOL)
    ref.L.bcnn_update(ref.net)
    hip.update()
    for i in range(2, len(names)):
        if not ref.tensor(i).data:
            continue
        hip.download(to_hip[i])
        _compare("%s %s data after update" % (gname, names[i]), hip.data(to_hip[i]), ref.data(i), REL_TOL)
    ref.close()
    hip.close()


def test_the_11x11_node_alone_teacher_forced():
    """node 0 of both nets on the same inputs; its backward from a random output gradient onto random carries in dw and
    db (both sides accumulate) and garbage in dx (both sides overwrite)"""
    ref, hip, names, to_hip, rs = _pair(_alexnet_stages, SHAPE)
    node = 0
    src = [ref.node_src(node, k) for k in range(ref.node_num_src(node))]
    dst = ref.node_dst(node, 0)
    assert [hip.node_src(node, k) for k in range(len(src))] == [to_hip[t] for t in src] and hip.node_dst(node) == to_hip[dst]
    ref.forward_node(node)
    hip.forward_node(node)
    hip.download(to_hip[dst], False)
    _compare("teacher-forced c1", hip.data(to_hip[dst]), ref.data(dst), REL_TOL)
    hip.data(to_hip[dst])[...] = ref.data(dst)
    ref.grad(dst)[...] = (rs.uniform(-1, 1, ref.shape(dst)) * 0.1).astype(np.float32)
    hip.grad(to_hip[dst])[...] = ref.grad(dst)
    hip.upload(to_hip[dst], with_grad=True)
    for t in src:
        if ref.grad(t) is None:
            continue
        ref.grad(t)[...] = rs.uniform(-1, 1, ref.shape(t)).astype(np.float32)
        hip.grad(to_hip[t])[...] = ref.grad(t)
        hip.upload(to_hip[t], with_grad=True)
    ref.backward_node(node)
    hip.backward_node(node)
    checked = 0
    for t in src + [dst]:
        if ref.grad(t) is None:
            continue
        hip.download(to_hip[t], True)
        _compare("teacher-forced d(%s)" % names[t], hip.grad(to_hip[t]), ref.grad(t), REL_TOL)
        checked += 1
    assert checked >= 4  # dx, dw, db and the rewritten dy
    ref.close()
    hip.close()
