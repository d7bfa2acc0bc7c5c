"""One training step of the yolov3-tiny pattern at toy size against the unmodified reference (oracle/_ref/libbcnn_ref.so):
input 32x32x3, N = 2, SGD;

    c1 -> pool -> c2 -> pool -> c3 -> c4 -> 1x1 h1 -> yolo1 (8x8, anchors 3, 4)
    [route] c3 -> 1x1 c5 -> upsample x2 -> concat with c2 -> c6 -> 1x1 h2 -> yolo2 (16x16, anchors 0, 1, 2)

c3 is read by a convolution and by the later route, c2 by a max-pooling node and the later concat. Identical weights on
both sides, set as tests/test_concat_upsample.py sets them; after forward + backward every tensor's data and gradient,
after the update every weight, at that file's rule (1e-4 of the tensor's maximum plus its floor). The thresholds of the
heads' loss are comparisons, so the precondition of tests/test_yolo_train_head.py is asserted on the reference's heads in
both steps (the seed of input and labels is searched on reference nets alone).

Second step: the loss of a second forward (the mean of the heads' costs, as bcnn_train_on_batch returns it) within 1e-3
relative of the reference's. Measured on an MI355X: 93.596642 against the reference's 93.596657, a relative difference
of 1.6e-7. The oracle builds one variant of the reference (its in-tree gemm, no BLAS), so no spread between builds of
the reference enters the bound."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from oracle import ref_bind as rb
from tests import _detect_ref as D
from tests import _yolo_train as Y
from tests.test_concat_upsample import _compare

pytestmark = pytest.mark.gpu

SIDE, N, CLASSES = 32, 2, 2
ANCHORS = [3, 4, 5, 3, 6, 7, 10, 12, 16, 11]   # input pixels
HEADS = [Y.Head(8, 8, [3, 4], CLASSES, SIDE, SIDE, ANCHORS), Y.Head(16, 16, [0, 1, 2], CLASSES, SIDE, SIDE, ANCHORS)]


def _graph(net):
    is_ref = isinstance(net, rb.RefNet)
    if not is_ref:
        assert net.set_detector_training(True) == 0
    lrelu = rb.ACT_LRELU
    net.conv(8, 3, 1, 1, 1, 1, lrelu, "input", "c1")
    net.maxpool(2, 2, rb.PADDING_SAME, "c1", "p1")
    net.conv(16, 3, 1, 1, 1, 1, lrelu, "p1", "c2")
    net.maxpool(2, 2, rb.PADDING_SAME, "c2", "p2")
    net.conv(16, 3, 1, 1, 1, 1, lrelu, "p2", "c3")
    net.conv(16, 3, 1, 1, 1, 1, lrelu, "c3", "c4")
    net.conv(HEADS[0].channels, 1, 1, 0, 1, 0, rb.ACT_NONE, "c4", "h1")
    nodes = []
    if is_ref:
        nodes.append(D.ref_yolo(net, HEADS[0].num, CLASSES, HEADS[0].mask, ANCHORS, "h1", "yolo1"))
        D.ref_concat(net, ["c3"], "r1")
    else:
        nodes.append(net.yolo(HEADS[0].num, CLASSES, HEADS[0].mask, ANCHORS, "h1", "yolo1"))
        net.concat(["c3"], "r1")
    net.conv(8, 1, 1, 0, 1, 1, lrelu, "r1", "c5")
    if is_ref:
        D.ref_upsample(net, 2, "c5", "up")
        D.ref_concat(net, ["up", "c2"], "cat")
    else:
        net.upsample(2, "c5", "up")
        net.concat(["up", "c2"], "cat")
    net.conv(16, 3, 1, 1, 1, 1, lrelu, "cat", "c6")
    net.conv(HEADS[1].channels, 1, 1, 0, 1, 0, rb.ACT_NONE, "c6", "h2")
    if is_ref:
        nodes.append(D.ref_yolo(net, HEADS[1].num, CLASSES, HEADS[1].mask, ANCHORS, "h2", "yolo2"))
    else:
        nodes.append(net.yolo(HEADS[1].num, CLASSES, HEADS[1].mask, ANCHORS, "h2", "yolo2"))
    net.compile()
    return nodes


def _ref_net():
    """a fresh reference net with the weights every run of this file uses; (net, nodes, tensor names)"""
    D.need_ref()
    D.ref_lib()
    ctypes.CDLL(None).srand(1234)
    ref = rb.RefNet(mode=rb.MODE_TRAIN, w=SIDE, h=SIDE, c=3, n=N)
    nodes = _graph(ref)
    ref.L.bcnn_set_sgd_optimizer(ref.net, 0.01, 0.9)
    ref.L.bcnn_set_weight_regularizer(ref.net, 5e-4)
    rs = np.random.RandomState(7)
    nt = ref.L.ref_num_tensors(ref.net)
    names = [ref.L.ref_tensor_name(ref.net, i).decode() for i in range(nt)]
    for i in range(2, nt):
        d = ref.data(i)
        if names[i].endswith("_scales") or names[i].endswith("_run_var"):
            d[...] = rs.uniform(0.5, 1.5, d.shape)
        elif names[i].endswith("_b"):
            d[...] = rs.uniform(-0.2, 0.2, d.shape)
    return ref, nodes, names


def _batch(seed):
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1, 1, (N, 3, SIDE, SIDE)).astype(np.float32)
    rows = []
    for _ in range(N):   # a dozen truths per image, the size of any of the five anchors: both heads take some
        rows.append(Y._row([Y.random_truth(rs, HEADS[k % 2]) for k in range(12)]))
    return x, np.stack(rows)


def _heads_clear(ref, nodes, labels):
    return all(Y.thresholds_clear(hd, ref.data(ref.node_dst(node)), labels) for hd, node in zip(HEADS, nodes))


def _ref_loss(ref, nodes):
    """bcnn_get_loss over the heads (bcnn_net.c:431-449): the mean of cost = |grad|^2, in float like there"""
    costs = [np.float32(np.sum(ref.grad(ref.node_dst(node)).astype(np.float64) ** 2)) for node in nodes]
    return float(np.float32(sum(costs)) / np.float32(len(costs)))


def _reference_step(seed):
    """step 1 (forward, backward, update) and the forward of step 2 on a fresh reference net; None when a head's
    threshold is within 1e-3 in either forward"""
    ref, nodes, names = _ref_net()
    x, labels = _batch(seed)
    nt = len(names)
    start = {i: ref.data(i).copy() for i in range(2, nt) if ref.tensor(i).data}
    ref.data(0)[...] = x
    ref.data(1)[...] = labels.reshape(ref.shape(1))
    ref.forward()
    clear = _heads_clear(ref, nodes, labels)
    ref.backward()
    after = {i: (ref.data(i).copy(), None if ref.grad(i) is None else ref.grad(i).copy())
             for i in range(nt) if ref.tensor(i).data}
    ref.L.bcnn_update(ref.net)
    updated = {i: ref.data(i).copy() for i in range(2, nt) if ref.tensor(i).data}
    ref.forward()
    clear = clear and _heads_clear(ref, nodes, labels)
    out = dict(x=x, labels=labels, names=names, nodes=nodes, start=start, after=after, updated=updated,
               loss2=_ref_loss(ref, nodes), shapes=[ref.shape(i) for i in range(nt)])
    ref.close()
    return out if clear else None


_CACHE = {}


def _reference():
    if "ref" not in _CACHE:
        _CACHE["ref"] = next(r for r in (_reference_step(seed) for seed in range(40)) if r is not None)
    return _CACHE["ref"]


def _hip_net(want):
    from bcnn_amd import capi
    ctypes.CDLL(None).srand(1234)
    hip = capi.Net(mode=capi.MODE_TRAIN, w=SIDE, h=SIDE, c=3, n=N)
    assert _graph(hip) == want["nodes"]
    hip.set_sgd(0.01, 0.9, 5e-4)
    for i, d in want["start"].items():
        assert hip.shape(i) == want["shapes"][i], want["names"][i]
        hip.data(i)[...] = d
        hip.upload(i)
    hip.data(0)[...] = want["x"]
    hip.upload(0)
    hip.data(1)[...] = want["labels"].reshape(hip.shape(1))
    hip.upload(1)
    return hip


def test_one_training_step_matches_reference():
    want = _reference()
    hip = _hip_net(want)
    names = want["names"]
    hip.forward()
    hip.backward()
    for i, (data, grad) in want["after"].items():
        hip.download(i)
        _compare("%s data" % names[i], hip.data(i), data)
        if grad is not None and i != 1:
            _compare("%s grad" % names[i], hip.grad(i), grad)
    hip.update()
    for i, data in want["updated"].items():
        hip.download(i)
        _compare("%s data after update" % names[i], hip.data(i), data)
    hip.close()


def test_second_step_loss():
    """measured on an MI355X: 1.6e-7 relative (device 93.596642, reference 93.596657); the bound is 1e-3"""
    want = _reference()
    hip = _hip_net(want)
    hip.forward()
    hip.backward()
    hip.update()
    hip.forward()
    costs = [np.float32(hip.yolo_train_stats(node)["cost"]) for node in want["nodes"]]
    loss = float(np.float32(sum(costs)) / np.float32(len(costs)))
    rel = abs(loss - want["loss2"]) / abs(want["loss2"])
    print("second-step loss: device %.6f reference %.6f relative difference %.3g" % (loss, want["loss2"], rel))
    assert rel <= 1e-3, (loss, want["loss2"])
    hip.close()
