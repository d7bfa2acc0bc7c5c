"""bcnn_get_label_maps_batch through the C ABI of libbcnn.so alone: a ctypes handle of its own with raw pointers, caller
strides wider than the rows, eval NULL and non-NULL. The struct is laid out by hand from include/bcnn/bcnn.h (two pointers,
an int, a pointer, two int64: 48 bytes on LP64), so a field the Python binding and the header disagree about shows here."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from tests import _label_map_ref as R

pytestmark = pytest.mark.gpu

W, H, CLASSES, N = 16, 12, 5, 3
SIZES = [(40, 10), (10, 40), (23, 17)]
PADS = [3, 6, 1]
GUARD = 32


def _net_and_tensor(fit):
    from tests.test_label_maps_net import filled, make_net
    net = make_net()
    idx, x = filled(net, fit)
    return net, idx, x


def _handle():
    from bcnn_amd import capi
    capi.lib()
    L = C.CDLL(capi.LIB_PATH)
    vp, i = C.c_void_p, C.c_int
    L.bcnn_get_label_maps_batch.restype = i
    L.bcnn_get_label_maps_batch.argtypes = [vp, i, i, vp, vp, i, i, vp, vp, vp]
    return L


def _padded(arrays):
    bufs = [np.full(h * (w + p) + GUARD, 0xA5, np.uint8) for (w, h), p in zip(SIZES, PADS)]
    if arrays is not None:
        for buf, a, (w, h), p in zip(bufs, arrays, SIZES, PADS):
            buf[:h * (w + p)].reshape(h, w + p)[:, :w] = a
    return bufs


@pytest.mark.parametrize("fit", [R.LETTERBOX, R.STRETCH])
def test_raw_pointers_and_strides_without_and_with_eval(fit):
    net, idx, x = _net_and_tensor(fit)
    L = _handle()
    images = [R.fit(fit, W, H, w, h) for w, h in SIZES]
    want = R.labels(x, images, True)
    ws, hs = (C.c_int * N)(*[s[0] for s in SIZES]), (C.c_int * N)(*[s[1] for s in SIZES])
    strides = (C.c_int * N)(*[w + p for (w, h), p in zip(SIZES, PADS)])

    def check(bufs):
        for b, ((w, h), p) in enumerate(zip(SIZES, PADS)):
            rows = bufs[b][:h * (w + p)].reshape(h, w + p)
            assert np.array_equal(rows[:, :w], want[b]), b
            assert (rows[:, w:] == 0xA5).all() and (bufs[b][h * (w + p):] == 0xA5).all(), b

    # eval NULL
    bufs = _padded(None)
    lptr = (C.c_void_p * N)(*[a.ctypes.data for a in bufs])
    assert L.bcnn_get_label_maps_batch(net.net, idx, N, C.addressof(ws), C.addressof(hs), fit, 1, C.addressof(lptr),
                                       C.addressof(strides), None) == 0
    check(bufs)
    # eval non-NULL, truths at strides of their own, counts and totals added into
    rs = np.random.RandomState(5)
    truths = [rs.randint(0, CLASSES + 2, (h, w)).astype(np.uint8) for w, h in SIZES]
    truths[0][0, :4] = 255
    wc, wi, wo = R.confusion(want, truths, CLASSES, 255)
    assert wi == 4 and wo > 0
    tbufs = _padded(truths)
    tptr = (C.c_void_p * N)(*[a.ctypes.data for a in tbufs])
    counts = np.full((CLASSES, CLASSES), 100, np.int64)
    ev = C.create_string_buffer(struct.pack("@PPiPqq", C.addressof(tptr), C.addressof(strides), 255, counts.ctypes.data,
                                            10, 20), 48)
    assert struct.calcsize("@PPiPqq") == 48
    bufs = _padded(None)
    lptr = (C.c_void_p * N)(*[a.ctypes.data for a in bufs])
    assert L.bcnn_get_label_maps_batch(net.net, idx, N, C.addressof(ws), C.addressof(hs), fit, 1, C.addressof(lptr),
                                       C.addressof(strides), C.addressof(ev)) == 0
    check(bufs)
    _, _, _, _, ignored, oor = struct.unpack("@PPiPqq", ev.raw)
    assert np.array_equal(counts, wc + 100) and (ignored, oor) == (10 + wi, 20 + wo)
    # labels NULL with eval: the counts again, on top
    assert L.bcnn_get_label_maps_batch(net.net, idx, N, C.addressof(ws), C.addressof(hs), fit, 1, None, None,
                                       C.addressof(ev)) == 0
    _, _, _, _, ignored, oor = struct.unpack("@PPiPqq", ev.raw)
    assert np.array_equal(counts, 2 * wc + 100) and (ignored, oor) == (10 + 2 * wi, 20 + 2 * wo)
    # labels and eval both NULL: refused
    assert L.bcnn_get_label_maps_batch(net.net, idx, N, C.addressof(ws), C.addressof(hs), fit, 1, None, None, None) == 1
    net.close()
