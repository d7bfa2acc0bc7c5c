"""The TRAIN-mode forward of the YOLOv3 head (bcnn_set_detector_training; bcnn_amd/csrc/detect.hip) against the
unmodified reference (oracle/_ref/libbcnn_ref.so, bcnn_yolo.c:250-415) on `input -> upsample(1) -> concat -> yolo`:
one forward and one backward with labels written into tensor 1.

  dst.data                 relative 2e-6, the bar of tests/test_yolo_head.py;
  dst.grad, d(concat out)  |got - want| <= 1e-5 max(1, |want|): values that went through the device's expf / logf
                           (tests/test_detections_batch.py);
  cost                     3e-5 relative against the fp64 sum of the REFERENCE's squared gradient: twice the element bar
                           for the squares plus 1e-6 for the fp32 tree;
  statistics               against an fp64 evaluation over the reference's dst (tests/_yolo_train.py). count and the two
                           recalls are exact; the averages are sums of at most 100 terms (2 images x 50 truths) that each
                           hold the element bar of 1e-5, added in fp32 (100 x 2^-24 = 6e-6): 2e-5 max(1, |want|).

The 0.5 / 0.75 IoU thresholds and the choice of the best anchor are comparisons: every case asserts, on the reference's
output, that no value lies within 1e-3 of its threshold (the seed is searched like _input(seed) of tests/test_yolo_head.py
does), and no cell is left out of the comparison."""
import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from oracle import ref_bind as rb
from tests import _detect_ref as D
from tests import _yolo_train as Y

pytestmark = pytest.mark.gpu

# name -> (h, w, [mask per head], [classes per head], n); each the smallest shape at which its branch exists
CASES = {
    "9x11_hw_odd": (9, 11, [[1, 2, 4]], [4], 2),          # h w % 4 != 0, 3 of 5 anchors
    "8x8_hw_aligned": (8, 8, [[1, 2, 4]], [4], 2),
    "3x3_70_classes": (3, 3, [[2]], [70], 2),             # more classes than lanes in a wave
    "one_class": (5, 4, [[0, 3]], [1], 2),
    "two_heads": (6, 5, [[0, 1, 2], [3, 4]], [1, 4], 2),  # 3 x (5 + 1) = 2 x (5 + 4) channels of the same source
}
# the truth sets of image 0 and image 1, per scenario
SCENARIOS = [("none", "fifty"), ("zero_in_the_middle", "same_slot"), ("unmasked_and_corner", "fifty")]


def _heads(case):
    h, w, masks, classes, n = CASES[case]
    return [Y.Head(h, w, m, c) for m, c in zip(masks, classes)], n


def _problem(case, scenario, extra=None):
    """labels and head input of the first seed whose thresholds are clear (in double, from the input's own activation;
    the tests assert it again on the reference's output). extra: truths appended to image 0's list."""
    heads, n = _heads(case)
    for seed in range(40):
        rs = np.random.RandomState(1000 * seed + 17)
        sets = Y.truth_sets(rs, heads[0])
        labels = np.stack([sets[SCENARIOS[scenario][b % 2]] for b in range(n)])
        x = Y.head_input(rs, heads[0], n, labels)
        act = [_activated(hd, x) for hd in heads]
        if all(Y.thresholds_clear(hd, a, labels) for hd, a in zip(heads, act)):
            if extra is not None:
                labels = labels.copy()
                k = len(Y.truths_of(labels[0]))
                assert k + len(extra) <= Y.MAX_BOXES and np.all(labels[0].reshape(-1, 5)[k:] == 0)
                labels[0].reshape(-1, 5)[k:k + len(extra)] = extra
            return heads, n, labels, x
    raise AssertionError("no seed keeps the thresholds clear")


def _activated(head, x):
    v = head.view(x).astype(np.float64).copy()
    for e in [0, 1] + list(range(4, head.per_box)):
        v[:, :, e] = Y._sig(v[:, :, e])
    return v


def _build(net, heads, is_ref):
    anchors = list(Y.ANCHORS)
    nodes = []
    if is_ref:
        D.ref_upsample(net, 1, "input", "u0")
        D.ref_concat(net, ["input"], "cat")
    else:
        assert net.set_detector_training(True) == 0 and net.get_detector_training() == 1
        net.upsample(1, "input", "u0")
        net.concat(["input"], "cat")
    for k, hd in enumerate(heads):
        if is_ref:
            nodes.append(D.ref_yolo(net, hd.num, hd.classes, hd.mask, anchors, "cat", "yolo%d" % k))
        else:
            nodes.append(net.yolo(hd.num, hd.classes, hd.mask, anchors, "cat", "yolo%d" % k))
    net.compile()
    return nodes


def _run_hip(heads, n, labels, x):
    from bcnn_amd import capi
    hip = capi.Net(mode=capi.MODE_TRAIN, w=heads[0].w, h=heads[0].h, c=heads[0].channels, n=n, input_grad=True)  # the reference's upsample backward writes it unguarded
    nodes = _build(hip, heads, False)
    assert hip.shape(1) == (n, 1, 1, 5 * Y.MAX_BOXES)
    hip.data(0)[...] = x
    hip.upload(0)
    hip.data(1)[...] = labels.reshape(hip.shape(1))
    hip.upload(1)
    hip.forward()
    hip.backward()
    out = []
    for node in nodes:
        y = hip.node_dst(node)
        hip.download(y)
        out.append(dict(data=hip.data(y).copy(), grad=hip.grad(y).copy(), stats=hip.yolo_train_stats(node)))
    cat = hip.index("cat")
    hip.download(cat)
    cat_grad = hip.grad(cat).copy()
    hip.close()
    return out, cat_grad


def _run_ref(heads, n, labels, x):
    D.need_ref()
    D.ref_lib()
    ref = rb.RefNet(mode=rb.MODE_TRAIN, w=heads[0].w, h=heads[0].h, c=heads[0].channels, n=n, input_grad=True)  # the reference's upsample backward writes it unguarded
    nodes = _build(ref, heads, True)
    ref.data(0)[...] = x
    ref.data(1)[...] = labels.reshape(ref.shape(1))
    ref.forward()
    ref.backward()
    out = [dict(data=ref.data(ref.node_dst(node)).copy(), grad=ref.grad(ref.node_dst(node)).copy()) for node in nodes]
    cat_grad = ref.grad(ref.index("cat")).copy()
    ref.close()
    return out, cat_grad


def _close(tag, got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    excess = np.abs(got - want) - tol * np.maximum(1.0, np.abs(want))
    assert np.all(excess <= 0), "%s: |got - want| exceeds %g max(1, |want|) by up to %.3g" % (tag, tol, excess.max())


@pytest.mark.parametrize("scenario", range(len(SCENARIOS)), ids=["+".join(s) for s in SCENARIOS])
@pytest.mark.parametrize("case", list(CASES))
def test_train_forward_and_backward_match_reference(case, scenario):
    heads, n, labels, x = _problem(case, scenario)
    want, want_cat = _run_ref(heads, n, labels, x)
    got, got_cat = _run_hip(heads, n, labels, x)
    for k, hd in enumerate(heads):
        r, g = want[k], got[k]
        assert Y.thresholds_clear(hd, r["data"], labels), "a threshold within 1e-3 on the reference's output"
        err = np.max(np.abs(g["data"].astype(np.float64) - r["data"]) / np.maximum(np.abs(r["data"]), 1e-30))
        assert err <= 2e-6, (k, err)
        _close("head %d gradient" % k, g["grad"], r["grad"], 1e-5)
        s = Y.statistics(hd, r["data"], r["grad"], labels)
        print(case, scenario, k, "reference (fp64):", s, "device:", g["stats"])
        assert g["stats"]["count"] == s["count"]
        assert abs(g["stats"]["cost"] - s["cost"]) <= 3e-5 * s["cost"], (g["stats"]["cost"], s["cost"])
        if s["count"]:
            assert g["stats"]["recall50"] == np.float32(s["recall50"]) and g["stats"]["recall75"] == np.float32(s["recall75"])
            for key in ("avg_iou", "avg_class", "avg_obj"):
                _close(key, g["stats"][key], s[key], 2e-5)
        else:
            assert all(np.isnan(g["stats"][key]) for key in ("avg_iou", "avg_class", "avg_obj", "recall50", "recall75"))
        _close("avg_anyobj", g["stats"]["avg_anyobj"], s["avg_anyobj"], 2e-5)
    _close("concat output gradient", got_cat, want_cat, 1e-5)


def test_overlapping_predictions_suppress_the_objectness_gradient():
    """on the reference's result: at least 5 predictions lose their no-object delta to an overlapping truth, at least 5
    keep it, and the device agrees cell by cell"""
    heads, n, labels, x = _problem("9x11_hw_odd", 2)
    want, _ = _run_ref(heads, n, labels, x)
    got, _ = _run_hip(heads, n, labels, x)
    hd = heads[0]
    data, grad = hd.view(want[0]["data"]), hd.view(want[0]["grad"])
    taken = np.zeros(grad[:, :, 4].shape, bool)
    for (b, _, a, j, i, _, _) in Y.assignment(hd, want[0]["data"], labels):
        taken[b, a, j, i] = True
    suppressed = (grad[:, :, 4] == 0) & ~taken & (data[:, :, 4] != 0)
    kept = (grad[:, :, 4] == data[:, :, 4]) & ~taken
    assert suppressed.sum() >= 5 and kept.sum() >= 5, (suppressed.sum(), kept.sum())
    assert np.array_equal(suppressed, (Y.best_iou(hd, want[0]["data"], labels) > 0.5) & ~taken)
    mine = hd.view(got[0]["grad"])[:, :, 4]
    assert np.array_equal(mine == 0, grad[:, :, 4] == 0)


@pytest.mark.parametrize("kind", ["x_is_one", "class_is_classes"])
def test_truth_outside_the_head_is_skipped_as_a_whole(kind):
    """own side only (the reference writes out of bounds): the truth changes neither the gradient nor the count. Its box
    is a thousandth of the input wide, so that it overlaps no prediction by half either."""
    hd = _heads("9x11_hw_odd")[0][0]
    extra = [[1.0, 0.5, 1e-3, 1e-3, 1]] if kind == "x_is_one" else [[0.5, 0.5, 1e-3, 1e-3, hd.classes]]
    heads, n, labels, x = _problem("9x11_hw_odd", 2)
    with_it = _problem("9x11_hw_odd", 2, extra=extra)[2]
    assert len(Y.truths_of(with_it[0])) == len(Y.truths_of(labels[0])) + 1
    a, a_cat = _run_hip(heads, n, labels, x)
    b, b_cat = _run_hip(heads, n, with_it, x)
    assert a[0]["stats"]["count"] > 0
    assert np.array_equal(a[0]["grad"], b[0]["grad"]) and np.array_equal(a_cat, b_cat)
    assert a[0]["stats"] == b[0]["stats"]


def test_two_fresh_nets_give_the_same_bits():
    heads, n, labels, x = _problem("two_heads", 2)
    a, a_cat = _run_hip(heads, n, labels, x)
    b, b_cat = _run_hip(heads, n, labels, x)
    assert np.array_equal(a_cat, b_cat)
    for k in range(len(heads)):
        assert np.array_equal(a[k]["data"], b[k]["data"]) and np.array_equal(a[k]["grad"], b[k]["grad"])
        assert a[k]["stats"] == b[k]["stats"] and a[k]["stats"]["count"] > 0
