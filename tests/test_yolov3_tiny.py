"""yolov3-tiny end to end: the Darknet cfg (its layer list, written here) and a seeded random Darknet *.weights file are
loaded by this build and by the unmodified reference (oracle/_ref/libbcnn_ref.so) -- same graph -- then one PREDICT
forward at 416 x 416: both YOLO heads agree within 1e-4 relative, and so do the detections."""
import ctypes
import struct

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from oracle import ref_bind as rb
from tests import _detect_ref as D
from tests.test_load_net import load_both, same_graph

pytestmark = pytest.mark.gpu

ANCHORS = "10,14,  23,27,  37,58,  81,82,  135,169,  344,319"


def _conv(filters, size=3, stride=1, bn=1, act="leaky"):
    return ("[convolutional]\n" + ("batch_normalize=1\n" if bn else "") +
            "filters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n" % (filters, size, stride, act))


def _yolo(mask):
    return ("[yolo]\nmask = %s\nanchors = %s\nclasses=80\nnum=6\njitter=.3\nignore_thresh = .7\ntruth_thresh = 1\n"
            "random=1\n" % (mask, ANCHORS))


def tiny_cfg(batch=1, size=416):
    s = ["[net]\nbatch=%d\nsubdivisions=1\nwidth=%d\nheight=%d\nchannels=3\nmomentum=0.9\ndecay=0.0005\n"
         "learning_rate=0.001\n" % (batch, size, size)]
    for f in (16, 32, 64, 128, 256):                     # layers 0 .. 9
        s += [_conv(f), "[maxpool]\nsize=2\nstride=2\n"]
    s += [_conv(512), "[maxpool]\nsize=2\nstride=1\n"]   # 10, 11
    s += [_conv(1024), _conv(256, 1), _conv(512)]        # 12, 13, 14
    s += [_conv(255, 1, bn=0, act="linear"), _yolo("3,4,5")]  # 15, 16
    s += ["[route]\nlayers = -4\n", _conv(128, 1), "[upsample]\nstride=2\n"]  # 17, 18, 19
    s += ["[route]\nlayers = -1, 8\n", _conv(256), _conv(255, 1, bn=0, act="linear"), _yolo("0,1,2")]  # 20 .. 23
    return "\n".join(s)


# (filters, input channels, size, batch-norm) of the convolutions in file order
TINY_CONVS = [(16, 3, 3, 1), (32, 16, 3, 1), (64, 32, 3, 1), (128, 64, 3, 1), (256, 128, 3, 1), (512, 256, 3, 1),
              (1024, 512, 3, 1), (256, 1024, 1, 1), (512, 256, 3, 1), (255, 512, 1, 0), (128, 256, 1, 1),
              (256, 384, 3, 1), (255, 256, 1, 0)]


def write_tiny_weights(path, seed=0):
    """Darknet *.weights: header, then per convolution biases [, scales, rolling mean, rolling variance], weights.
    He-scaled weights and positive variances keep the activations O(1) through the 13 layers."""
    rs = np.random.RandomState(seed)
    with open(path, "wb") as fp:
        fp.write(struct.pack("<iii", 0, 2, 0) + struct.pack("<Q", 0))
        for f, c, k, bn in TINY_CONVS:
            parts = [rs.uniform(-0.1, 0.1, f)]
            if bn:
                parts += [rs.uniform(0.8, 1.2, f), rs.uniform(-0.1, 0.1, f), rs.uniform(0.5, 1.5, f)]
            parts.append(rs.normal(0, np.sqrt(2.0 / (c * k * k)), f * c * k * k))
            for p in parts:
                fp.write(p.astype(np.float32).tobytes())


def test_yolov3_tiny_forward_and_detections_match_reference(tmp_path):
    D.need_ref()
    D.ref_lib()
    cfg = tmp_path / "yolov3-tiny.cfg"
    cfg.write_text(tiny_cfg())
    model = tmp_path / "yolov3-tiny.weights"
    write_tiny_weights(str(model))
    ref, st_ref, net, st = load_both(str(cfg), str(model), rb.MODE_PREDICT)
    assert st_ref == 0 and st == 0
    nt = same_graph(ref, net)
    from bcnn_amd import capi
    hip = capi.Net.__new__(capi.Net)
    hip.L, hip.net = net.L, net.net
    nn = ref.num_nodes()
    heads = [i for i in range(nn) if ref.L.ref_node_type(ref.net, i) == 14]  # BCNN_LAYER_YOLOV3
    assert len(heads) == 2 and nt > 40
    ref.L.ref_set_threads(ref.net, 8)
    assert ref.L.bcnn_compile_net(ref.net) == 0 and hip.L.bcnn_compile_net(hip.net) == 0
    x = np.random.RandomState(1).uniform(0, 1, ref.shape(0)).astype(np.float32)
    assert ref.shape(0) == (1, 3, 416, 416)
    ref.data(0)[...] = x
    hip.data(0)[...] = x
    hip.upload(0)
    ref.forward()
    hip.forward()
    outs = []
    for hnode in heads:
        y = ref.node_dst(hnode)
        hip.download(y, with_grad=False)
        a, b = hip.data(y).astype(np.float64), ref.data(y).astype(np.float64)
        err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
        assert err <= 1e-4, (hnode, err)
        outs.append(b)
    thresh = 0.5
    # boxes whose objectness lies within 1e-4 of the threshold may fall on either side: counted, reported, excused
    near = sum(int(np.sum(np.abs(o.reshape(3, 85, -1)[:, 4] - thresh) < 1e-4)) for o in outs)
    for relative in (0, 1):
        args = (0, 768, 576, 416, 416, thresh, relative)
        want = D.ref_detections(ref, *args)
        got = hip.get_detections(*args)
        assert len(want) > 0
        if near == 0:
            D.assert_same_detections(got, want, 1e-4)
        else:
            dropped = D.assert_same_detections(got, want, 1e-4,
                                               skip_near=lambda d: abs(d["objectness"] - thresh) < 1e-4)
            print("yolov3-tiny: %d candidate(s) within 1e-4 of the threshold, %d box(es) excused" % (near, dropped))
    ref.close()
    hip.L.bcnn_end_net(ctypes.byref(hip.net))
