"""The switch of detector training through the C API, the INI key and the Python wrapper: what it admits (the head on a
TRAIN net, bcnn_set_mode(TRAIN), the detection-list loader), the label tensor the builder shapes, the statistics getter's
refusals, and the loss bcnn_train_on_batch returns. The refusals WITHOUT the switch are pinned by tests/test_yolo_head.py
and tests/test_data_loader.py."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from tests import _yolo_train as Y

pytestmark = pytest.mark.gpu

HEAD = Y.Head(5, 4, [0, 3], 1)
MAX_BOXES = Y.MAX_BOXES


def _net(mode, switch, n=2):
    from bcnn_amd import capi
    net = capi.Net(mode=mode, w=HEAD.w, h=HEAD.h, c=HEAD.channels, n=n)
    if switch:
        assert net.set_detector_training(True) == 0
    net.upsample(1, "input", "u0")
    return net


def _yolo_status(net, src=b"u0", dst=b"yolo"):
    m = (C.c_int * HEAD.num)(*HEAD.mask)
    a = (C.c_float * len(Y.ANCHORS))(*Y.ANCHORS)
    return net.L.bcnn_add_yolo_layer(net.net, HEAD.num, HEAD.classes, 4, len(Y.ANCHORS) // 2, m, a, src, dst)


def _set_loader(net, kind, path):
    enc = path.encode() if path else None
    return net.L.bcnn_set_data_loader(net.net, kind, enc, None, enc, None)


def test_switch_admits_head_mode_and_loader(tmp_path):
    from bcnn_amd import capi
    lst = tmp_path / "list.txt"
    lst.write_text("nothing.ppm 0 0.5 0.5 0.2 0.2\n")
    net = _net(capi.MODE_TRAIN, switch=False)
    assert net.get_detector_training() == 0
    assert _set_loader(net, 4, str(lst)) == 1                       # no switch, no head: refused as before
    assert net.set_detector_training(True) == 0 and net.get_detector_training() == 1
    assert net.tensor(1).data is None or not net.tensor(1).data     # no label yet
    assert _yolo_status(net) == 0                                   # the builder on a TRAIN net
    assert net.shape(1) == (2, 1, 1, 5 * MAX_BOXES) and net.tensor(1).data and net.tensor(1).data_gpu
    assert _set_loader(net, 4, str(lst)) == 0
    assert net.set_mode(capi.MODE_VALID) == 0
    assert net.set_mode(capi.MODE_TRAIN) == 0                       # back to TRAIN with a head
    assert net.L.bcnn_set_detector_training(None, 1) == 1 and net.L.bcnn_get_detector_training(None) == 0
    net.close()
    # a VALID net gets the label too, and may then be switched to TRAIN; a PREDICT net has no gradient to write
    net = _net(capi.MODE_VALID, switch=True)
    assert _yolo_status(net) == 0 and net.shape(1) == (2, 1, 1, 5 * MAX_BOXES)
    assert net.set_mode(capi.MODE_TRAIN) == 0
    net.close()
    net = _net(capi.MODE_PREDICT, switch=True)
    assert _yolo_status(net) == 0 and net.shape(1) == (2, 1, 1, 5 * MAX_BOXES)
    assert net.set_mode(capi.MODE_TRAIN) == 1
    net.close()
    # a head built before the switch was set has no label: TRAIN stays refused, the loader is admitted by the head
    net = _net(capi.MODE_VALID, switch=False)
    assert _yolo_status(net) == 0
    assert _set_loader(net, 4, str(lst)) == 0
    assert net.set_detector_training(True) == 0
    assert net.set_mode(capi.MODE_TRAIN) == 1
    net.close()


def test_ini_key_switches_detector_training(tmp_path):
    from bcnn_amd import capi
    body = ("input_width=4\ninput_height=5\ninput_channels=12\nbatch_size=2\n%s"
            "[upsample]\nsrc=input\ndst=u0\nstride=1\n"
            "[yolo]\nsrc=u0\ndst=yolo\nnum_anchors=5\nnum_classes=1\nnum_coords=4\nmask=0,3\nanchors=%s\n")
    anchors = ",".join("%g" % a for a in Y.ANCHORS)
    on, off = tmp_path / "on.cfg", tmp_path / "off.cfg"
    on.write_text("[net]\n" + body % ("train_detector=1\n", anchors))
    off.write_text("[net]\n" + body % ("", anchors))
    with pytest.raises(RuntimeError):
        capi.Net.load_net(str(off), None, mode=capi.MODE_TRAIN)      # the builder's refusal aborts the load
    net = capi.Net.load_net(str(on), None, mode=capi.MODE_TRAIN)
    assert net.get_detector_training() == 1 and net.num_nodes == 2
    assert net.shape(1) == (2, 1, 1, 5 * MAX_BOXES)
    lst = tmp_path / "list.txt"
    lst.write_text("nothing.ppm 0 0.5 0.5 0.2 0.2\n")
    assert _set_loader(net, 4, str(lst)) == 0
    net.compile()
    net.forward()                                                    # the TRAIN forward runs (labels: all zero)
    s = net.yolo_train_stats(1)
    assert s["count"] == 0 and s["cost"] > 0 and 0 < s["avg_anyobj"] < 1
    net.close()


def test_stats_getter_refusals():
    from bcnn_amd import capi
    net = _net(capi.MODE_TRAIN, switch=True)
    assert _yolo_status(net) == 0
    out = capi.YoloTrainStats()
    L = net.L
    assert L.bcnn_yolo_get_train_stats(net.net, 0, C.byref(out)) == 1      # the upsample node
    assert L.bcnn_yolo_get_train_stats(net.net, -1, C.byref(out)) == 1 and L.bcnn_yolo_get_train_stats(net.net, 2, C.byref(out)) == 1
    assert L.bcnn_yolo_get_train_stats(net.net, 1, None) == 1
    assert L.bcnn_yolo_get_train_stats(None, 1, C.byref(out)) == 1
    with pytest.raises(ValueError):
        net.yolo_train_stats(0)
    assert L.bcnn_yolo_get_train_stats(net.net, 1, C.byref(out)) == 0      # before any forward: zeros
    assert out.count == 0 and out.cost == 0
    net.close()


def test_train_on_batch_returns_the_mean_of_the_heads_costs():
    """two heads over one source, no loader (the caller filled the host tensors): the step's return value is the mean
    of the two costs the getter reports for that forward, and the heads' gradient reached the source"""
    from bcnn_amd import capi
    heads = [Y.Head(6, 5, [0, 1, 2], 1), Y.Head(6, 5, [3, 4], 4)]
    net = capi.Net(mode=capi.MODE_TRAIN, w=5, h=6, c=heads[0].channels, n=2)
    assert net.set_detector_training(True) == 0
    net.conv(heads[0].channels, 1, 1, 0, 1, 0, capi.ACT_NONE, "input", "c1")
    nodes = [net.yolo(hd.num, hd.classes, hd.mask, list(Y.ANCHORS), "c1", "yolo%d" % k) for k, hd in enumerate(heads)]
    net.compile()
    net.set_sgd(0.0, 0.0)                                            # a step that leaves the weights alone
    rs = np.random.RandomState(9)
    sets = Y.truth_sets(rs, heads[0])
    net.data(0)[...] = rs.uniform(-1, 1, net.shape(0))
    net.data(1)[...] = np.stack([sets["same_slot"], sets["fifty"]]).reshape(net.shape(1))
    loss = net.L.bcnn_train_on_batch(net.net)
    costs = [net.yolo_train_stats(node)["cost"] for node in nodes]
    assert all(c > 0 for c in costs) and costs[0] != costs[1]
    assert loss == np.float32((np.float32(costs[0]) + np.float32(costs[1])) / np.float32(2))
    c1 = net.index("c1")
    net.download(c1)
    assert np.abs(net.grad(c1)).max() > 0
    net.close()
