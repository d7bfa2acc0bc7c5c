"""bcnn_fill_tensor_with_images (Net.fill_images): the input tensor of a batch from raw uint8 images, prepared on the
device. Every case compares bit for bit (tolerance 0) with the composition that defines it, built from this project's own
host functions: libbip.so bip_resize_bilinear (to the tensor's extent, or to the letterbox extent pasted onto a canvas of
bytes 128), then libbcnn.so bcnn_convert_img_to_float. tests/test_bip.py pins those two to the reference.

The device kernel gives a lane 8 consecutive pixels of a row and 256 lanes a workgroup, so the issue's 3 x 21 x 37 letterbox
plane is one workgroup per image; a 3 x 70 x 61 plane (560 runs: three workgroups, the last one ragged) is added for the
path with several."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

pytestmark = pytest.mark.gpu

STRETCH, LETTERBOX = 0, 1
u8p = C.POINTER(C.c_uint8)
MEAN = (104.5, 117.25, 123.75)
NORM = 1.0 / 57.5


def _ptr(a):
    return a.ctypes.data_as(u8p)


_host = {}


def _host_fns():
    """bip_resize_bilinear and bcnn_convert_img_to_float on handles of their own (their argtypes stay private)"""
    if not _host:
        import os
        from bcnn_amd import capi
        capi.lib()
        bip = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libbip.so"))
        bip.bip_resize_bilinear.argtypes = [u8p] + [C.c_size_t] * 3 + [u8p] + [C.c_size_t] * 4
        bip.bip_resize_bilinear.restype = C.c_int
        L = C.CDLL(capi.LIB_PATH)
        L.bcnn_convert_img_to_float.argtypes = [u8p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float,
                                                C.c_float, C.POINTER(C.c_float)]
        L.bcnn_convert_img_to_float.restype = None
        _host["resize"], _host["convert"] = bip.bip_resize_bilinear, L.bcnn_convert_img_to_float
    return _host["resize"], _host["convert"]


def letterbox_extent(W, H, w, h):
    if np.float32(W) / np.float32(w) < np.float32(H) / np.float32(h):
        return W, (h * W) // w
    return (w * H) // h, H


def expected(buf, w, h, c, W, H, fit, norm, swap, mean):
    """entry of the tensor for the image in `buf` (h rows of buf.shape[1] bytes, w * c of them pixels): (c, H, W) float32"""
    resize, convert = _host_fns()
    nw, nh = (W, H) if fit == STRETCH else letterbox_extent(W, H, w, h)
    tmp = np.zeros((nh, nw * c), np.uint8)
    assert resize(_ptr(buf), w, h, buf.shape[1], _ptr(tmp), nw, nh, nw * c, c) == 0
    canvas = np.full((H, W, c), 128, np.uint8)
    xo, yo = (W - nw) // 2, (H - nh) // 2
    canvas[yo:yo + nh, xo:xo + nw] = tmp.reshape(nh, nw, c)
    out = np.empty((c, H, W), np.float32)
    convert(_ptr(canvas), W, H, c, norm, 1 if swap else 0, mean[0], mean[1], mean[2],
            out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def source(rs, w, h, c, pad=0):
    """(buffer of h rows of w * c + pad bytes, its h x w x c view): random pixels, random padding"""
    buf = rs.randint(0, 256, (h, w * c + pad)).astype(np.uint8)
    view = buf[:, :w * c].reshape(h, w, c)
    assert view.strides == (w * c + pad, c, 1) and np.shares_memory(view, buf)
    return buf, view


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def make_net(w, h, c, n, filters=8):
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_PREDICT, w=w, h=h, c=c, n=n)
    net.conv(filters, 3, 1, 1, src="input", dst="conv")
    net.compile()
    return net


def preset(net, seed=99):
    """uploads a known pattern into the input tensor and returns a copy of it"""
    before = np.random.RandomState(seed).uniform(-9, 9, net.shape(0)).astype(np.float32)
    net.data(0)[...] = before
    net.upload(0)
    return before


def device_input(net):
    net.download(0, with_grad=False)
    return net.data(0).copy()


# ---- stretch ------------------------------------------------------------------------------------------------------

# (w, h, row padding): up, down with padded rows, identity, one-sample axes
STRETCH_SOURCES = [(7, 5, 0), (40, 31, 5), (18, 13, 0), (1, 1, 0), (1, 9, 0)]


@pytest.mark.parametrize("c", [3, 1, 4])
@pytest.mark.parametrize("swap", [0, 1])
def test_stretch_matches_host_composition(c, swap):
    W, H, N = 18, 13, 5        # row length 18 and plane 234 are not multiples of 4: heads and tails of the runs are live
    rs = np.random.RandomState(10 * c + swap)
    srcs = [source(rs, w, h, c, pad) for w, h, pad in STRETCH_SOURCES]
    want = np.stack([expected(buf, w, h, c, W, H, STRETCH, NORM, swap, MEAN)
                     for (buf, _), (w, h, _) in zip(srcs, STRETCH_SOURCES)])
    # the identity case really is one: the resize returns the source, so the entry is the plain conversion of it
    ident = np.ascontiguousarray(srcs[2][1]).astype(np.float32).transpose(2, 0, 1)
    ks = [2, 1, 0] if (swap and c == 3) else list(range(c))
    m = np.array([MEAN[k] if c == 3 else MEAN[0] for k in ks], np.float32)[:, None, None]
    assert same_bits(want[2], (ident[ks] - m) * np.float32(NORM))
    net = make_net(W, H, c, N)
    preset(net)
    assert net.fill_images([v for _, v in srcs], fit=STRETCH, norm_coeff=NORM, swap_to_bgr=swap, mean=MEAN) == 0
    got = device_input(net)
    net.close()
    for b in range(N):
        assert same_bits(got[b], want[b]), "image %d (%s)" % (b, STRETCH_SOURCES[b])


# ---- letterbox ----------------------------------------------------------------------------------------------------

# net (W, H) -> sources (w, h): wide with H - new_h odd, tall with W - new_w odd, exactly the net's aspect ratio
LETTERBOX_CASES = [((37, 21), [(50, 20), (12, 30), (74, 42)]),
                   ((61, 70), [(90, 31), (24, 64), (122, 140)])]


@pytest.mark.parametrize("plane,sizes", LETTERBOX_CASES)
def test_letterbox_matches_host_composition(plane, sizes):
    W, H = plane
    c, swap = 3, 1
    rs = np.random.RandomState(W)
    srcs = [source(rs, w, h, c) for w, h in sizes]
    ext = [letterbox_extent(W, H, w, h) for w, h in sizes]
    assert ext[0][0] == W and (H - ext[0][1]) % 2 == 1, ext     # the floor of the y offset shows
    assert ext[1][1] == H and (W - ext[1][0]) % 2 == 1, ext     # ... and of the x offset
    assert ext[2] == (W, H), ext
    want = np.stack([expected(buf, w, h, c, W, H, LETTERBOX, NORM, swap, MEAN) for (buf, _), (w, h) in zip(srcs, sizes)])
    net = make_net(W, H, c, len(sizes))
    preset(net)
    assert net.fill_images([v for _, v in srcs], fit=LETTERBOX, norm_coeff=NORM, swap_to_bgr=swap, mean=MEAN) == 0
    got = device_input(net)
    net.close()
    for b in range(len(sizes)):
        assert same_bits(got[b], want[b]), "image %d (%s)" % (b, sizes[b])
    # the bands: (128 - mean) * norm, the mean of the source channel the plane reads (planes are B, G, R after the swap)
    for b, (nw, nh) in enumerate(ext[:2]):
        xo, yo = (W - nw) // 2, (H - nh) // 2
        band = np.ones((H, W), bool)
        band[yo:yo + nh, xo:xo + nw] = False
        assert band.any()
        for k in range(3):
            value = (np.float32(128) - np.float32(MEAN[2 - k])) * np.float32(NORM)
            assert same_bits(got[b, k][band], np.full(int(band.sum()), value, np.float32)), (b, k)


# ---- partial batch ------------------------------------------------------------------------------------------------

def test_partial_batch_leaves_the_other_entries():
    W, H, c = 18, 13, 3
    rs = np.random.RandomState(3)
    srcs = [source(rs, 9, 11, c), source(rs, 25, 8, c, 3)]
    want = [expected(srcs[0][0], 9, 11, c, W, H, STRETCH, NORM, 0, MEAN),
            expected(srcs[1][0], 25, 8, c, W, H, STRETCH, NORM, 0, MEAN)]
    net = make_net(W, H, c, 4)
    before = preset(net)
    assert net.fill_images([v for _, v in srcs], fit=STRETCH, norm_coeff=NORM, mean=MEAN) == 0
    got = device_input(net)
    net.close()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert same_bits(got[2:], before[2:])


# ---- refusals -----------------------------------------------------------------------------------------------------

def _raw(net, images, widths, heights, strides, c, fit=STRETCH, tensor=0, num=None,
         null_images=False, null_widths=False, null_heights=False):
    k = len(images)
    ptrs = (C.c_void_p * k)(*[(a.ctypes.data if a is not None else None) for a in images])
    ws, hs = (C.c_int * k)(*widths), (C.c_int * k)(*heights)
    ss = (C.c_int * k)(*strides) if strides is not None else None
    return net.L.bcnn_fill_tensor_with_images(net.net, tensor, k if num is None else num,
                                              None if null_images else ptrs, None if null_widths else ws,
                                              None if null_heights else hs, ss, c, fit, NORM, 0, *MEAN)


def test_refusals_return_invalid_parameter_and_leave_the_tensor():
    W, H, N = 37, 21, 2
    net = make_net(W, H, 3, N)
    before = preset(net)
    rs = np.random.RandomState(5)
    a, b, g = rs.randint(0, 256, (6, 8, 3)).astype(np.uint8), rs.randint(0, 256, (5, 4, 3)).astype(np.uint8), \
        rs.randint(0, 256, (6, 8, 1)).astype(np.uint8)
    ok = dict(images=[a, b], widths=[8, 4], heights=[6, 5], strides=[24, 12], c=3)
    num_tensors_bound = 10000
    refused = {
        "tensor index below 0": _raw(net, tensor=-1, **ok),
        "tensor index past the end": _raw(net, tensor=num_tensors_bound, **ok),
        "no images": _raw(net, num=0, **ok),
        "more images than the batch": _raw(net, [a, b, a], [8, 4, 8], [6, 5, 6], None, 3),
        "channels differ from the tensor's": _raw(net, [g], [8], [6], None, 1),
        "images NULL": _raw(net, null_images=True, **ok),
        "widths NULL": _raw(net, null_widths=True, **ok),
        "heights NULL": _raw(net, null_heights=True, **ok),
        "an image NULL": _raw(net, [a, None], [8, 4], [6, 5], None, 3),
        "width 0": _raw(net, [a, b], [8, 0], [6, 5], None, 3),
        "height 0": _raw(net, [a, b], [8, 4], [0, 5], None, 3),
        "stride below width * c": _raw(net, [a, b], [8, 4], [6, 5], [24, 11], 3),
        "unknown fit": _raw(net, fit=2, **ok),
        "letterbox extent 0": _raw(net, [np.zeros((1, 1000, 3), np.uint8)], [1000], [1], None, 3, fit=LETTERBOX),
        "through the wrapper": net.fill_images([g]),
    }
    # a tensor without a device buffer: the input tensor with its device pointer taken away for the call
    t = net.tensor(0)
    keep = t.data_gpu
    t.data_gpu = None
    refused["no device buffer"] = _raw(net, **ok)
    t.data_gpu = keep
    assert all(v == 1 for v in refused.values()), refused
    assert same_bits(device_input(net), before)
    assert _raw(net, **ok) == 0        # the same arguments, unbroken, are accepted
    net.close()
    # c outside 1..4, on a tensor that has that many channels
    net5 = make_net(9, 7, 5, 1)
    before = preset(net5)
    assert _raw(net5, [rs.randint(0, 256, (7, 9, 5)).astype(np.uint8)], [9], [7], None, 5) == 1
    assert same_bits(device_input(net5), before)
    net5.close()


# ---- staging reuse ------------------------------------------------------------------------------------------------

def test_back_to_back_calls_with_a_growing_staging_block():
    """the second call stages more than the first (and more than the device block's initial 1 MiB), with no
    synchronisation in between; each source buffer is zeroed as soon as its call has returned"""
    W, H, c = 18, 13, 3
    rs = np.random.RandomState(8)
    small = [source(rs, 7, 5, c), source(rs, 30, 17, c, 2)]
    large = [source(rs, 700, 610, c), source(rs, 33, 20, c, 1)]
    sizes_small, sizes_large = [(7, 5), (30, 17)], [(700, 610), (33, 20)]
    assert sum(b.size for b, _ in large) > (1 << 20) > sum(b.size for b, _ in small)
    want_small = [expected(b, w, h, c, W, H, LETTERBOX, NORM, 1, MEAN) for (b, _), (w, h) in zip(small, sizes_small)]
    want_large = [expected(b, w, h, c, W, H, STRETCH, NORM, 0, MEAN) for (b, _), (w, h) in zip(large, sizes_large)]
    net_a, net_b = make_net(W, H, c, 2), make_net(W, H, c, 2)
    preset(net_a)
    preset(net_b)
    net_a.sync()
    assert net_a.fill_images([v for _, v in small], fit=LETTERBOX, norm_coeff=NORM, swap_to_bgr=1, mean=MEAN) == 0
    for buf, _ in small:
        buf[...] = 0
    assert net_b.fill_images([v for _, v in large], fit=STRETCH, norm_coeff=NORM, swap_to_bgr=0, mean=MEAN) == 0
    for buf, _ in large:
        buf[...] = 0
    got_a, got_b = device_input(net_a), device_input(net_b)
    net_a.close()
    net_b.close()
    for b in range(2):
        assert same_bits(got_a[b], want_small[b]), b
        assert same_bits(got_b[b], want_large[b]), b


# ---- through a forward --------------------------------------------------------------------------------------------

def test_forward_from_filled_input_equals_forward_from_uploaded_input():
    W, H, c, N = 18, 13, 3, 2
    rs = np.random.RandomState(12)
    srcs, sizes = [source(rs, 29, 14, c), source(rs, 11, 23, c, 4)], [(29, 14), (11, 23)]
    net = make_net(W, H, c, N)
    out = net.node_dst(0)
    assert net.fill_images([v for _, v in srcs], fit=LETTERBOX, norm_coeff=1 / 255.0, swap_to_bgr=1) == 0
    net.forward()
    net.download(out, with_grad=False)
    y_fill = net.data(out).copy()
    net.data(0)[...] = np.stack([expected(b, w, h, c, W, H, LETTERBOX, 1 / 255.0, 1, (0, 0, 0))
                                 for (b, _), (w, h) in zip(srcs, sizes)])
    net.upload(0)
    net.forward()
    net.download(out, with_grad=False)
    y_host = net.data(out).copy()
    net.close()
    assert np.abs(y_host).max() > 0
    assert same_bits(y_fill, y_host)


def test_detections_from_filled_input_equal_those_from_uploaded_input():
    """A PREDICT net with a YOLO head. The head's source has num * (coords + 1 + classes) >= 5 channels and an image has at
    most 4, so a 1 x 1 convolution stands between the image and the head (tests/test_yolo_head.py feeds the head from the
    input tensor itself, which an image cannot fill)."""
    from bcnn_amd import capi
    NUM, CLASSES, COORDS = 3, 4, 4
    MASK, ANCHORS = [1, 2, 4], [1.5, 2.0, 2.5, 1.0, 3.0, 3.5, 4.0, 2.5, 1.2, 1.7]
    W, H, c, N = 11, 9, 3, 2
    rs = np.random.RandomState(21)
    frames = [(64, 48), (30, 50)]
    srcs = [source(rs, w, h, c) for w, h in frames]
    net = capi.Net(mode=capi.MODE_PREDICT, w=W, h=H, c=c, n=N)
    net.conv(NUM * (COORDS + 1 + CLASSES), 1, 1, 0, src="input", dst="conv")
    net.yolo(NUM, CLASSES, MASK, ANCHORS, "conv", "yolo")
    net.compile()
    assert net.fill_images([v for _, v in srcs], fit=LETTERBOX, norm_coeff=1 / 255.0, swap_to_bgr=1) == 0
    net.forward()
    det_fill = net.get_detections_batch(frames, W, H, 0.5, 0)
    net.data(0)[...] = np.stack([expected(b, w, h, c, W, H, LETTERBOX, 1 / 255.0, 1, (0, 0, 0))
                                 for (b, _), (w, h) in zip(srcs, frames)])
    net.upload(0)
    net.forward()
    det_host = net.get_detections_batch(frames, W, H, 0.5, 0)
    net.close()
    assert sum(len(d) for d in det_host) > 0
    assert [len(d) for d in det_fill] == [len(d) for d in det_host]
    for a, b in zip(det_fill, det_host):
        for da, db in zip(a, b):
            assert all(da[k] == db[k] for k in ("x", "y", "w", "h", "objectness")), (da, db)
            assert np.array_equal(da["prob"], db["prob"])
