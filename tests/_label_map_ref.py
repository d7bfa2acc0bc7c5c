"""The label-map rule (include/bcnn_hip.h, bcnn_amd/csrc/label_map_rule.h) restated in numpy. Not a test.

Labels. Image b of a call has an extent out_w x out_h and a rectangle (roi_x, roi_y, roi_w, roi_h) of plane b of the
[n][C][h][w] tensor. Its label map is
    y = _interp_ref.forward(x[b:b+1, :, roi_y:roi_y+roi_h, roi_x:roi_x+roi_w], out_h, out_w, align_corners)   (float32)
    labels = first-maximum argmax of y over axis 1, as uint8
numpy's argmax returns the first maximum, and the test inputs hold no NaN. No tolerance anywhere: labels and counts are
compared for equality.

Fit (integer rule of bcnn_fill_tensor_with_images, include/bcnn/bcnn.h), an iw x ih image in the W x H plane:
    STRETCH   : rectangle (0, 0, W, H)
    LETTERBOX : if float32(W) / float32(iw) < float32(H) / float32(ih): new_w = W, new_h = (ih * W) // iw
                else: new_h = H, new_w = (iw * H) // ih;   rectangle ((W - new_w) // 2, (H - new_h) // 2, new_w, new_h)
    refused (None): an extent below 1, an unknown fit, a letterbox extent of 0.

Plan: image b's labels are out_h rows of round_up(out_w, 4) bytes, every image starts on a 16-byte boundary, and a total
-- doubled when truths are staged -- past 2^31 bytes is refused (None).

Confusion: a truth byte t is ignored when ignore_label >= 0 and t == ignore_label (that wins over the range), valid when
t < C, out of range otherwise; a valid pixel labelled a adds 1 to counts[t][a]."""
import numpy as np

from tests import _interp_ref

F32 = np.float32
STRETCH, LETTERBOX = 0, 1


def fit(kind, W, H, iw, ih):
    """(out_w, out_h, roi_x, roi_y, roi_w, roi_h) or None"""
    if min(W, H, iw, ih) < 1 or kind not in (STRETCH, LETTERBOX):
        return None
    new_w, new_h = W, H
    if kind == LETTERBOX:
        if F32(W) / F32(iw) < F32(H) / F32(ih):
            new_h = (ih * W) // iw
        else:
            new_w = (iw * H) // ih
    if new_w < 1 or new_h < 1 or new_w > W or new_h > H:
        return None
    return iw, ih, (W - new_w) // 2, (H - new_h) // 2, new_w, new_h


def fill_extent(kind, W, H, iw, ih):
    """(new_w, new_h, x_off, y_off) as bcnn_fill_tensor_with_images documents them (bcnn.h), written from that text alone"""
    if kind == STRETCH:
        new_w, new_h = W, H
    elif np.float32(W) / np.float32(iw) < np.float32(H) / np.float32(ih):
        new_w, new_h = W, (ih * W) // iw
    else:
        new_h, new_w = H, (iw * H) // ih
    return new_w, new_h, (W - new_w) // 2, (H - new_h) // 2


def plan(images, with_truths=False):
    """(row_strides, offsets, total_bytes) or None; images: (out_w, out_h, ...) tuples"""
    strides, offsets, at = [], [], 0
    for im in images:
        out_w, out_h = im[0], im[1]
        if out_w < 1 or out_h < 1:
            return None
        stride = (out_w + 3) // 4 * 4
        strides.append(stride)
        offsets.append(at)
        at += (stride * out_h + 15) // 16 * 16
    if at * (2 if with_truths else 1) > 2 ** 31:
        return None
    return strides, offsets, at


def resample(x, b, image, align_corners):
    """the float32 values [C][out_h][out_w] of image b"""
    out_w, out_h, rx, ry, rw, rh = image
    return _interp_ref.forward(x[b:b + 1, :, ry:ry + rh, rx:rx + rw], out_h, out_w, align_corners)[0]


def labels(x, images, align_corners):
    """x: [n][C][h][w] float32 numpy; one uint8 array [out_h][out_w] per image"""
    out = []
    for b, im in enumerate(images):
        y = resample(x, b, im, align_corners)
        assert y.dtype == F32 and not np.isnan(y).any()
        out.append(np.argmax(y, axis=0).astype(np.uint8))
    return out


def tied_share(x, images, align_corners):
    """(pixels whose maximum is attained by more than one class, pixels) over the images of a call"""
    tied = total = 0
    for b, im in enumerate(images):
        y = resample(x, b, im, align_corners)
        tied += int(((y == y.max(axis=0, keepdims=True)).sum(axis=0) > 1).sum())
        total += y.shape[1] * y.shape[2]
    return tied, total


def confusion(label_maps, truths, c, ignore_label):
    """(counts [c][c] int64, ignored, out_of_range) of uint8 label maps against uint8 truth maps"""
    counts = np.zeros((c, c), np.int64)
    ignored = out_of_range = 0
    for lab, tr in zip(label_maps, truths):
        t = tr.astype(np.int64).ravel()
        a = lab.astype(np.int64).ravel()
        ign = (t == ignore_label) if ignore_label >= 0 else np.zeros(t.shape, bool)
        valid = ~ign & (t < c)
        ignored += int(ign.sum())
        out_of_range += int((~ign & ~valid).sum())
        np.add.at(counts, (t[valid], a[valid]), 1)
    return counts, ignored, out_of_range


def raw_call(L, x_d=0x1000, n=2, c=5, h=7, w=9, images=((4, 3, 0, 0, 9, 7), (5, 2, 1, 1, 3, 3)), num=None, labels=True,
           label_strides=None, truths=False, truth_strides=None, ignore=-1, counts=True, null_row=None):
    """one call with host buffers that a refusal must leave untouched; x_d is never dereferenced by a refused call"""
    import ctypes as C
    from bcnn_amd import ops
    arr = ops._label_map_images(list(images))
    k = len(images)
    dims = [(min(max(im[1], 1), 8), min(max(im[0], 1), 8) + 3) for im in images]   # (a refused call never indexes them)
    bufs = [np.full(d, 0xA5, np.uint8) for d in dims]
    trs = [np.full(d, 1, np.uint8) for d in dims]
    lptr = (C.c_void_p * k)(*[None if null_row == ("l", b) else a.ctypes.data for b, a in enumerate(bufs)])
    tptr = (C.c_void_p * k)(*[None if null_row == ("t", b) else a.ctypes.data for b, a in enumerate(trs)])
    ls = (C.c_int * k)(*label_strides) if label_strides else None
    ts = (C.c_int * k)(*truth_strides) if truth_strides else None
    cnt = np.full(c * c if c > 0 else 1, 7, np.int64)
    ign, oor = C.c_longlong(7), C.c_longlong(7)
    st = L.bcnn_hip_label_maps_batch(
        x_d, n, c, h, w, 0, C.cast(arr, C.c_void_p) if images is not None else None, k if num is None else num,
        C.cast(lptr, C.c_void_p) if labels else None, C.cast(ls, C.c_void_p) if ls else None,
        C.cast(tptr, C.c_void_p) if truths else None, C.cast(ts, C.c_void_p) if ts else None, ignore,
        cnt.ctypes.data if counts else None, C.cast(C.pointer(ign), C.c_void_p), C.cast(C.pointer(oor), C.c_void_p))
    untouched = all((a == 0xA5).all() for a in bufs) and (cnt == 7).all() and ign.value == 7 and oor.value == 7
    return st, untouched
