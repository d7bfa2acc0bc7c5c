"""bcnn_get_label_maps_batch (Net.label_maps) at the net level: a PREDICT net, input 3 x 12 x 16, a 1 x 1 convolution to
five channels, batch 3. The batch is filled from three images of different sizes with Net.fill_images, forwarded, and the
label maps of the convolution's output at the images' own sizes must equal tests/_label_map_ref.py on the DOWNLOADED
tensor, byte for byte, with the fit the batch was filled with (letterbox: the integer rectangle; stretch: the whole
plane), and the counts of an evaluation against hand-made truths the numpy count. Then the refusals that need a net."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from tests import _label_map_ref as R

pytestmark = pytest.mark.gpu

W, H, CLASSES, N = 16, 12, 5, 3
SIZES = [(40, 10), (10, 40), (23, 17)]     # wide, tall, and one that fills neither axis exactly


def make_net(pool=False):
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_PREDICT, w=W, h=H, c=3, n=N)
    net.conv(CLASSES, 1, 1, 0, src="input", dst="logits")
    if pool:
        net.maxpool(2, 2, src="logits", dst="pooled")
    net.compile()
    return net


def filled(net, fit):
    rs = np.random.RandomState(11)
    images = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for w, h in SIZES]
    assert net.fill_images(images, fit=fit, norm_coeff=1.0 / 64, mean=(100.0, 110.0, 120.0)) == 0
    net.forward()
    idx = net.index("logits")
    net.download(idx, with_grad=False)
    return idx, net.data(idx).copy()


@pytest.mark.parametrize("align_corners", [False, True])
@pytest.mark.parametrize("fit", [R.LETTERBOX, R.STRETCH])
def test_label_maps_of_the_net_equal_the_oracle_on_the_downloaded_tensor(fit, align_corners):
    net = make_net()
    idx, x = filled(net, fit)
    assert x.shape == (N, CLASSES, H, W)
    images = [R.fit(fit, W, H, w, h) for w, h in SIZES]
    want = R.labels(x, images, align_corners)
    assert len({int(v) for a in want for v in np.unique(a)}) > 1           # the convolution separates some classes
    got = net.label_maps(idx, SIZES, fit=fit, align_corners=align_corners)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint8 and g.shape == (SIZES[b][1], SIZES[b][0]) and np.array_equal(g, w), b
    # fewer images than the batch
    got = net.label_maps(idx, SIZES[:2], fit=fit, align_corners=align_corners)
    assert len(got) == 2 and all(np.array_equal(g, w) for g, w in zip(got, want))
    net.close()


@pytest.mark.parametrize("fit", [R.LETTERBOX, R.STRETCH])
def test_evaluation_against_hand_made_truths(fit):
    net = make_net()
    idx, x = filled(net, fit)
    images = [R.fit(fit, W, H, w, h) for w, h in SIZES]
    want = R.labels(x, images, False)
    truths = []
    for b, (w, h) in enumerate(SIZES):      # the prediction itself, a band of each other byte of interest on top
        t = want[b].copy()
        t[0, :] = 255                       # ignored
        t[h // 2, :] = CLASSES              # out of range
        t[h - 1, :] = (np.arange(w) + b) % CLASSES
        truths.append(t)
    wc, wi, wo = R.confusion(want, truths, CLASSES, 255)
    assert wi == sum(w for w, _ in SIZES) and wo == sum(w for w, _ in SIZES) and np.trace(wc) > 0
    got, counts, ignored, oor = net.label_maps(idx, SIZES, fit=fit, truths=truths, ignore_label=255)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(counts, wc) and (ignored, oor) == (wi, wo)
    none, counts, ignored, oor = net.label_maps(idx, SIZES, fit=fit, truths=truths, ignore_label=255, labels=False)
    assert none is None and np.array_equal(counts, wc) and (ignored, oor) == (wi, wo)
    from bcnn_amd import capi
    iou, mean = capi.iou_from_confusion(counts)
    inter = np.diag(wc).astype(np.float64)
    union = wc.sum(0) + wc.sum(1) - inter
    assert np.array_equal(iou[union > 0], inter[union > 0] / union[union > 0]) and 0.0 < mean <= 1.0
    net.close()


def _raw(net, tensor, sizes, fit=R.STRETCH, labels=True, num=None, null_sizes=False, eval_=None, strides=None):
    """bcnn_get_label_maps_batch with buffers a refusal must leave at 0xA5; returns (status, untouched)"""
    k = len(sizes)
    ws, hs = (C.c_int * k)(*[s[0] for s in sizes]), (C.c_int * k)(*[s[1] for s in sizes])
    bufs = [np.full((max(h, 1), max(w, 1)), 0xA5, np.uint8) for w, h in sizes]
    lptr = (C.c_void_p * k)(*[a.ctypes.data for a in bufs])
    ss = (C.c_int * k)(*strides) if strides else None
    st = net.L.bcnn_get_label_maps_batch(net.net, tensor, k if num is None else num, None if null_sizes else ws, hs, fit, 0,
                                         lptr if labels else None, ss, C.byref(eval_) if eval_ is not None else None)
    return st, all((a == 0xA5).all() for a in bufs)


def test_refusals_return_invalid_parameter_and_leave_the_outputs():
    from bcnn_amd import capi
    net = make_net(pool=True)
    logits, pooled = net.index("logits"), net.index("pooled")
    assert net.shape(pooled) == (N, CLASSES, H // 2, W // 2)
    filled(net, R.LETTERBOX)
    counts = np.full((CLASSES, CLASSES), 7, np.int64)
    truth = [np.zeros((h, w), np.uint8) for w, h in SIZES]
    tptr = (C.c_void_p * N)(*[a.ctypes.data for a in truth])

    def ev(truths=tptr, cnt=counts, ignore=255):
        return capi.LabelMapEval(truths, None, ignore, cnt.ctypes.data_as(C.POINTER(C.c_int64)) if cnt is not None else None,
                                 7, 7)
    refused = {
        "letterbox on a tensor of another extent": _raw(net, pooled, SIZES, fit=R.LETTERBOX),
        "more images than the batch": _raw(net, logits, SIZES + [(4, 4)]),
        "no images": _raw(net, logits, SIZES, num=0),
        "tensor index below 0": _raw(net, -1, SIZES),
        "tensor index past the end": _raw(net, 10000, SIZES),
        "widths NULL": _raw(net, logits, SIZES, null_sizes=True),
        "a width of 0": _raw(net, logits, [(0, 4)]),
        "a height below 0": _raw(net, logits, [(4, -2)]),
        "unknown fit": _raw(net, logits, SIZES, fit=2),
        "letterbox extent 0": _raw(net, logits, [(1000, 3)], fit=R.LETTERBOX),
        "neither labels nor eval": _raw(net, logits, SIZES, labels=False),
        "a stride below the width": _raw(net, logits, SIZES, strides=[40, 9, 23]),
        "eval without counts": _raw(net, logits, SIZES, eval_=ev(cnt=None)),
        "eval without truths": _raw(net, logits, SIZES, eval_=ev(truths=None)),
        "ignore label 256": _raw(net, logits, SIZES, eval_=ev(ignore=256)),
    }
    # a host-only tensor: the logits with their device pointer taken away for the call
    t = net.tensor(logits)
    keep = t.data_gpu
    t.data_gpu = None
    refused["no device buffer"] = _raw(net, logits, SIZES)
    t.data_gpu = keep
    assert all(v == (1, True) for v in refused.values()), refused
    assert (counts == 7).all()
    e = ev(ignore=256)
    assert _raw(net, logits, SIZES, eval_=e)[0] == 1 and (e.ignored, e.out_of_range) == (7, 7)
    e = ev()
    with pytest.raises(ValueError):
        net.label_maps(pooled, SIZES, fit=R.LETTERBOX)
    # the same arguments, unbroken, are accepted: the pooled tensor under STRETCH, the logits with an eval
    st, untouched = _raw(net, pooled, SIZES)
    assert st == 0 and not untouched
    st, untouched = _raw(net, logits, SIZES, fit=R.LETTERBOX, eval_=e)
    assert st == 0 and not untouched and counts.sum() == 7 * CLASSES * CLASSES + sum(w * h for w, h in SIZES)
    assert (e.ignored, e.out_of_range) == (7, 7)          # no truth byte is 255 or past the classes: added 0 to both
    net.close()
