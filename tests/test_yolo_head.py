"""The YOLOv3 head and bcnn_yolo_get_detections against the unmodified reference (oracle/_ref/libbcnn_ref.so) on
`input -> concat(input) -> yolo` (an identity upsample first: neither concat nor the head may be a net's first node),
and the refusals of what this build does not do: the head in TRAIN nets (its loss is not built), and resizing a net
that holds a concat / upsample / YOLO node."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from oracle import ref_bind as rb
from tests import _detect_ref as D

pytestmark = pytest.mark.gpu

NUM, CLASSES, COORDS = 3, 4, 4
MASK = [1, 2, 4]
ANCHORS = [1.5, 2.0, 2.5, 1.0, 3.0, 3.5, 4.0, 2.5, 1.2, 1.7]   # total = 5 anchors, in input pixels
H, W, N = 9, 11, 2
THRESH = 0.5
NMS = 0.45


def _graph(net, is_ref):
    if is_ref:
        D.ref_upsample(net, 1, "input", "u0")
        D.ref_concat(net, ["input"], "cat")
        return D.ref_yolo(net, NUM, CLASSES, MASK, ANCHORS, "cat", "yolo")
    net.upsample(1, "input", "u0")
    net.concat(["input"], "cat")
    return net.yolo(NUM, CLASSES, MASK, ANCHORS, "cat", "yolo")


def _sig(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def _input(seed):
    """head input whose objectness and class probabilities keep >= 1e-3 from the threshold, and whose candidate boxes
    (decoded here in double) have no pairwise IoU within 1e-3 of the NMS threshold; None if this seed fails the latter"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-3, 3, (N, NUM, COORDS + 1 + CLASSES, H, W))
    for _ in range(20):
        obj = _sig(x[:, :, COORDS])
        near = np.abs(obj - THRESH) < 1e-3
        prob = obj[:, :, None] * _sig(x[:, :, COORDS + 1:])
        near_p = np.abs(prob - THRESH) < 1e-3
        if not near.any() and not near_p.any():
            break
        x[:, :, COORDS][near] += 0.05
        x[:, :, COORDS + 1:][near_p] += 0.05
    else:
        return None
    for b in range(N):
        boxes = []
        for n in range(NUM):
            for i in range(H):
                for j in range(W):
                    if _sig(x[b, n, COORDS, i, j]) <= THRESH:
                        continue
                    a = ANCHORS[2 * MASK[n]:2 * MASK[n] + 2]
                    boxes.append(((j + _sig(x[b, n, 0, i, j])) / W, (i + _sig(x[b, n, 1, i, j])) / H,
                                  np.exp(x[b, n, 2, i, j]) * a[0] / W, np.exp(x[b, n, 3, i, j]) * a[1] / H))
        bx = np.array(boxes)
        l = np.maximum(bx[:, None, 0] - bx[:, None, 2] / 2, bx[None, :, 0] - bx[None, :, 2] / 2)
        r = np.minimum(bx[:, None, 0] + bx[:, None, 2] / 2, bx[None, :, 0] + bx[None, :, 2] / 2)
        t = np.maximum(bx[:, None, 1] - bx[:, None, 3] / 2, bx[None, :, 1] - bx[None, :, 3] / 2)
        u = np.minimum(bx[:, None, 1] + bx[:, None, 3] / 2, bx[None, :, 1] + bx[None, :, 3] / 2)
        iw, ih = r - l, u - t
        inter = np.where((iw < 0) | (ih < 0), 0.0, iw * ih)
        area = bx[:, 2] * bx[:, 3]
        iou = inter / (area[:, None] + area[None, :] - inter)
        if (np.abs(iou - NMS) < 1e-3).any():
            return None
    return x.reshape(N, NUM * (COORDS + 1 + CLASSES), H, W).astype(np.float32)


def _nets():
    from bcnn_amd import capi
    D.need_ref()
    D.ref_lib()
    x = next(v for v in (_input(s) for s in range(40)) if v is not None)
    shp = dict(w=W, h=H, c=x.shape[1], n=N)
    ref = rb.RefNet(mode=rb.MODE_PREDICT, **shp)
    hip = capi.Net(mode=capi.MODE_PREDICT, **shp)
    node = _graph(ref, True)
    assert _graph(hip, False) == node
    ref.compile()
    hip.compile()
    ref.data(0)[...] = x
    hip.data(0)[...] = x
    hip.upload(0)
    ref.forward()
    hip.forward()
    return ref, hip, node


def test_head_output_matches_reference():
    ref, hip, node = _nets()
    y = ref.node_dst(node)
    hip.download(y, with_grad=False)
    err = np.max(np.abs(hip.data(y).astype(np.float64) - ref.data(y)) / np.maximum(np.abs(ref.data(y)), 1e-30))
    assert err <= 2e-6, err
    # entries 2, 3 (w, h) are copied raw
    c = np.arange(hip.shape(y)[1]) % (COORDS + 1 + CLASSES)
    np.testing.assert_array_equal(hip.data(y)[:, (c == 2) | (c == 3)], hip.data(0)[:, (c == 2) | (c == 3)])
    ref.close()
    hip.close()


@pytest.mark.parametrize("batch", [0, 1])
@pytest.mark.parametrize("relative", [0, 1])
def test_detections_match_reference(batch, relative):
    ref, hip, _ = _nets()
    args = (batch, 640, 480, 416, 416, THRESH, relative)
    want = D.ref_detections(ref, *args)
    got = hip.get_detections(*args)
    assert len(want) > 5 and any(d["objectness"] == 0 for d in want)  # NMS suppressed something: the count includes it
    D.assert_same_detections(got, want, 1e-5)
    for d in got:
        assert d["prob"].shape == (CLASSES,)
    ref.close()
    hip.close()


def test_no_detection_returns_null():
    ref, hip, _ = _nets()
    assert hip.get_detections(0, 416, 416, 416, 416, 1.5, 1) == []
    n = ctypes.c_int(-1)
    assert not hip.L.bcnn_yolo_get_detections(hip.net, 0, 416, 416, 416, 416, 1.5, 1, ctypes.byref(n))
    assert n.value == 0
    ref.close()
    hip.close()


def _status_net(mode, c=NUM * (COORDS + 1 + CLASSES)):
    from bcnn_amd import capi
    net = capi.Net(mode=mode, w=W, h=H, c=c, n=1)
    net.upsample(1, "input", "u0")
    return net


def _yolo_status(net, classes=CLASSES):
    m = (ctypes.c_int * NUM)(*MASK)
    a = (ctypes.c_float * len(ANCHORS))(*ANCHORS)
    return net.L.bcnn_add_yolo_layer(net.net, NUM, classes, COORDS, len(ANCHORS) // 2, m, a, b"u0", b"yolo")


def test_yolo_refused_on_a_train_net():
    from bcnn_amd import capi
    net = _status_net(capi.MODE_TRAIN)
    assert _yolo_status(net) == 1
    assert net.L.bcnn_get_num_nodes(net.net) == 1 and net.index("yolo") < 0
    net.close()


def test_set_mode_train_refused_with_a_yolo_node():
    from bcnn_amd import capi
    net = _status_net(capi.MODE_PREDICT)
    assert _yolo_status(net) == 0
    assert net.set_mode(capi.MODE_TRAIN) == 1
    assert net.set_mode(capi.MODE_VALID) == 0   # other modes are fine
    assert net.set_mode(capi.MODE_TRAIN) == 1
    net.close()
    plain = _status_net(capi.MODE_PREDICT)      # without a head TRAIN is still allowed
    assert plain.set_mode(capi.MODE_TRAIN) == 0
    plain.close()


def test_yolo_channel_check():
    from bcnn_amd import capi
    net = _status_net(capi.MODE_PREDICT)
    assert _yolo_status(net, classes=CLASSES + 1) == 1
    assert net.L.bcnn_get_num_nodes(net.net) == 1
    net.close()


@pytest.mark.parametrize("kind", ["yolo", "concat", "upsample"])
def test_resize_refused_and_shapes_kept(kind):
    from bcnn_amd import capi
    net = _status_net(capi.MODE_PREDICT)
    if kind == "yolo":
        assert _yolo_status(net) == 0
    elif kind == "concat":
        net.concat(["u0", "input"], "cat")
    else:
        net.upsample(2, "u0", "up")
    net.compile()
    nt = 0
    while net.L.bcnn_peek_tensor(net.net, nt):
        nt += 1
    before = [net.shape(i) for i in range(nt)]
    assert net.resize(2 * W, 2 * H, before[0][1]) == 1
    assert [net.shape(i) for i in range(nt)] == before
    net.close()
