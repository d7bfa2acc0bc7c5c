"""bcnn_hip_label_maps_batch (ops.label_maps; bcnn_amd/csrc/label_map.hip) at the op level: label
maps at each image's own size, byte for byte against tests/_label_map_ref.py -- tests/_interp_ref.forward of the cropped
rectangle in float32, then numpy's first-maximum argmax -- and the confusion counts against the numpy count. No tolerance.

The tensor planes are 9 x 7 (w x h). One call holds images of 9 x 7 (the identity), 13 x 11, 4 x 3 (downsampling), 1 x 1,
33 x 17, 16 x 8 and 36 x 28, n = 7: out_w % 4 in {0, 1, 3}, widths shorter than one four-pixel item, rows of one pixel, an
image of one item, and (36 x 28: 252 items, 33 x 17: 153) images next to each other in the prefix of workgroup counts.
Both align_corners values, C in {1, 2, 5, 21, 33, 64, 65, 256} (64 / 65: the LDS tile and its first miss; 256: the last
byte value). Two input families: integers of {-1, 0, 1}, so that tied maxima are everywhere and a wrong tie rule cannot
pass, and standard-normal logits with a planted winner per source pixel, so that every class wins somewhere."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _label_map_ref as R

W, H = 9, 7
SIZES = [(9, 7), (13, 11), (4, 3), (1, 1), (33, 17), (16, 8), (36, 28)]
IMAGES = [R.fit(R.STRETCH, W, H, w, h) for w, h in SIZES]
N = len(SIZES)
CLASSES = [1, 2, 5, 21, 33, 64, 65, 256]
GUARD = 64


@functools.lru_cache(maxsize=None)
def logits(family, c, n=N, h=H, w=W):
    rs = np.random.RandomState(1000 * c + 10 * h + (family == "ties"))
    if family == "ties":
        return rs.randint(-1, 2, (n, c, h, w)).astype(np.float32)
    x = rs.standard_normal((n, c, h, w)).astype(np.float32)
    win = np.arange(n * h * w) % c          # the planted winner of every source pixel: each class wins somewhere
    win[1] = c - 1                          # ... and the last class inside the identity image, next to class 0
    b, y, xx = np.unravel_index(np.arange(n * h * w), (n, h, w))
    x[b, win, y, xx] += np.float32(12.0)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle(family, c, align_corners):
    """computed once per case and shared; the arrays are read-only"""
    out = R.labels(logits(family, c), IMAGES, align_corners)
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, np.float32, order="C")).to("cuda")   # (a copy: the cached arrays are read-only)


def _trace(on):
    from bcnn_amd import _lib
    L = _lib.load()
    if on:
        L.bcnn_hip_trace_enable(1)
        return None
    n = L.bcnn_hip_trace_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return buf.value.decode().split()


def _same(got, want):
    return len(got) == len(want) and all(g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w)
                                         for g, w in zip(got, want))


# ---- what the oracle itself must show (no device) -----------------------------------------------------------------

def test_oracle_has_ties_everywhere_and_every_edge_class():
    tied = total = 0
    for c in CLASSES:
        for ac in (False, True):
            t, p = R.tied_share(logits("ties", c), IMAGES, ac)
            tied, total = tied + t, total + p
            labs = np.concatenate([a.ravel() for a in oracle("planted", c, ac)])
            assert (labs == 0).any() and (labs == c - 1).any(), (c, ac)
            assert labs.max() == c - 1                      # 255 at C = 256: a signed byte would not compare equal
    assert tied * 10 >= total, (tied, total)


# ---- labels -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("family", ["ties", "planted"])
@pytest.mark.parametrize("align_corners", [False, True])
@pytest.mark.parametrize("c", CLASSES)
def test_labels_equal_the_oracle(c, align_corners, family):
    from bcnn_amd import ops
    x = _dev(logits(family, c))
    want = oracle(family, c, align_corners)
    _trace(True)
    got = ops.label_maps(x, IMAGES, align_corners)
    assert _trace(False) == ["label_map"]                  # exactly one kernel for the seven images
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), "image %d (%s): %d bytes differ" % (
            b, SIZES[b], int((g != w).sum()))
    assert _same(ops.label_maps(x, IMAGES, align_corners), got)      # a second run gives the same bytes


@pytest.mark.gpu
@pytest.mark.parametrize("align_corners", [False, True])
def test_caller_strides_padding_and_guard_bands_are_untouched(align_corners):
    from bcnn_amd import _lib, ops
    c = 21
    x = _dev(logits("ties", c))
    want = oracle("ties", c, align_corners)
    pads = [5, 0, 7, 3, 1, 16, 2]
    bufs = [np.full(h * (w + p) + GUARD, 0xA5, np.uint8) for (w, h), p in zip(SIZES, pads)]
    arr = ops._label_map_images(IMAGES)
    lptr = (C.c_void_p * N)(*[a.ctypes.data for a in bufs])
    strides = (C.c_int * N)(*[w + p for (w, h), p in zip(SIZES, pads)])
    st = _lib.load().bcnn_hip_label_maps_batch(x.data_ptr(), N, c, H, W, 1 if align_corners else 0, C.cast(arr, C.c_void_p),
                                               N, C.cast(lptr, C.c_void_p), C.cast(strides, C.c_void_p), None, None, -1,
                                               None, None, None)
    assert st == 0
    for b, ((w, h), p) in enumerate(zip(SIZES, pads)):
        rows = bufs[b][:h * (w + p)].reshape(h, w + p)
        assert np.array_equal(rows[:, :w], want[b]), b
        assert (rows[:, w:] == 0xA5).all() and (bufs[b][h * (w + p):] == 0xA5).all(), b


# ---- rectangles -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("family", ["ties", "planted"])
@pytest.mark.parametrize("align_corners", [False, True])
def test_rectangles_of_a_letterboxed_plane(align_corners, family):
    from bcnn_amd import ops
    w, h, c = 16, 12, 5
    images = [ops.label_map_fit(R.LETTERBOX, w, h, 40, 10), ops.label_map_fit(R.LETTERBOX, w, h, 10, 40),
              ops.label_map_fit(R.LETTERBOX, w, h, 16, 12), (7, 5, 13, 2, 1, 1)]      # the last: off-centre, one element
    assert images[:3] == [(40, 10, 0, 4, 16, 4), (10, 40, 6, 0, 3, 12), (16, 12, 0, 0, 16, 12)]
    x = logits(family, c, n=4, h=h, w=w)
    want = R.labels(x, images, align_corners)
    got = ops.label_maps(_dev(x), images, align_corners)
    assert _same(got, want)
    assert (got[3] == got[3][0, 0]).all() and got[3][0, 0] == np.argmax(x[3, :, 2, 13])
    # fewer images than the batch: entries 0 and 1 alone
    assert _same(ops.label_maps(_dev(x), images[:2], align_corners), want[:2])


# ---- evaluation -------------------------------------------------------------------------------------------------------

def _truths(c, ignore):
    """random truth maps in which every value of 0 .. C + 1 (as far as a byte goes) and the ignore byte occur"""
    rs = np.random.RandomState(77 + c)
    top = min(c + 2, 256)
    out = [rs.randint(0, top, (h, w)).astype(np.uint8) for w, h in SIZES]
    big = out[6].reshape(-1)
    big[:top] = np.arange(top, dtype=np.uint8)
    if ignore >= 0:
        big[top] = ignore
        out[0][0, 0] = ignore
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c,ignore", [(c, 255) for c in CLASSES] + [(5, 3), (21, -1), (65, 0)])
def test_evaluation_counts_equal_numpy(c, ignore):
    from bcnn_amd import ops
    x = _dev(logits("ties", c))
    truths = _truths(c, ignore)
    labs = oracle("ties", c, True)
    want, want_ign, want_oor = R.confusion(labs, truths, c, ignore)
    assert want.sum() + want_ign + want_oor == sum(w * h for w, h in SIZES)
    assert want_ign > 0 or ignore < 0
    assert want_oor > 0 or c + (ignore == 255) >= 256
    name = "label_map:eval:lds" if c <= 64 else "label_map:eval"
    _trace(True)
    got, counts, ign, oor = ops.label_maps(x, IMAGES, True, truths=truths, ignore_label=ignore)
    assert _trace(False) == [name]
    assert _same(got, labs)
    assert np.array_equal(counts, want) and (ign, oor) == (want_ign, want_oor)
    # labels = NULL: the same counts, ADDED into a pre-filled array; and a second run gives equal counts
    pre = np.arange(c * c, dtype=np.int64).reshape(c, c) * 3 + 1
    acc = pre.copy()
    _trace(True)
    none, counts2, ign2, oor2 = ops.label_maps(x, IMAGES, True, truths=truths, ignore_label=ignore, labels=False, counts=acc)
    assert _trace(False) == [name]
    assert none is None and counts2 is acc and np.array_equal(acc, pre + want) and (ign2, oor2) == (want_ign, want_oor)


@pytest.mark.gpu
def test_evaluation_with_truth_strides_and_added_totals():
    from bcnn_amd import _lib, ops
    c, ignore = 21, 255
    x = _dev(logits("planted", c))
    truths = _truths(c, ignore)
    labs = oracle("planted", c, False)
    want, want_ign, want_oor = R.confusion(labs, truths, c, ignore)
    pads = [3, 0, 1, 9, 2, 0, 5]
    padded = [np.full((h, w + p), 7, np.uint8) for (w, h), p in zip(SIZES, pads)]   # 7 is a valid class: a read past the
    for buf, t, (w, h) in zip(padded, truths, SIZES):                               # row width would show in the counts
        buf[:, :w] = t
    arr = ops._label_map_images(IMAGES)
    tptr = (C.c_void_p * N)(*[a.ctypes.data for a in padded])
    strides = (C.c_int * N)(*[w + p for (w, h), p in zip(SIZES, pads)])
    counts = np.zeros((c, c), np.int64)
    ign, oor = C.c_longlong(1000), C.c_longlong(2000)
    for rounds in (1, 2):
        st = _lib.load().bcnn_hip_label_maps_batch(x.data_ptr(), N, c, H, W, 0, C.cast(arr, C.c_void_p), N, None, None,
                                                   C.cast(tptr, C.c_void_p), C.cast(strides, C.c_void_p), ignore,
                                                   counts.ctypes.data, C.cast(C.pointer(ign), C.c_void_p),
                                                   C.cast(C.pointer(oor), C.c_void_p))
        assert st == 0
        assert np.array_equal(counts, want * rounds)
        assert (ign.value, oor.value) == (1000 + want_ign * rounds, 2000 + want_oor * rounds)


# ---- several workgroups per image, a staging block that grows ---------------------------------------------------------

@pytest.mark.gpu
def test_images_of_several_workgroups_after_small_ones():
    """133 x 67 is 34 items a row and 2278 items: nine workgroups, the last one ragged; the block of the call is larger
    than the ones the calls above staged"""
    from bcnn_amd import ops
    c = 5
    x = logits("ties", c, n=3)
    images = [R.fit(R.STRETCH, W, H, 133, 67), R.fit(R.STRETCH, W, H, 2, 3), R.fit(R.STRETCH, W, H, 70, 150)]
    want = R.labels(x, images, False)
    truths = [np.random.RandomState(b).randint(0, c + 1, (im[1], im[0])).astype(np.uint8) for b, im in enumerate(images)]
    got, counts, ign, oor = ops.label_maps(_dev(x), images, False, truths=truths, ignore_label=-1)
    assert _same(got, want)
    wc, wi, wo = R.confusion(want, truths, c, -1)
    assert np.array_equal(counts, wc) and (ign, oor) == (wi, wo) and wo > 0


# ---- refusals that need a device pointer ------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals_leave_outputs_and_the_trace_untouched():
    from bcnn_amd import _lib
    L = _lib.load()
    x = _dev(logits("ties", 5, n=2))
    ptr = x.data_ptr()
    cases = dict(
        num_above_n=dict(n=1), num_zero=dict(num=0), c_257=dict(c=257),
        out_w_zero=dict(images=((0, 3, 0, 0, 9, 7),)), roi_leaves_right=dict(images=((4, 3, 1, 0, 9, 7),)),
        roi_empty=dict(images=((4, 3, 0, 0, 9, 0),)), label_stride_short=dict(label_strides=(4, 4)),
        truth_stride_short=dict(truths=True, truth_strides=(4, 4)), neither=dict(labels=False),
        truths_without_counts=dict(truths=True, counts=False), ignore_256=dict(truths=True, ignore=256),
        null_label_row=dict(null_row=("l", 0)), null_truth_row=dict(truths=True, null_row=("t", 1)),
        two_gib=dict(images=((65536, 32768, 0, 0, 9, 7), (1, 1, 0, 0, 9, 7))),
    )
    _trace(True)
    for name, kw in cases.items():
        st, untouched = R.raw_call(L, x_d=ptr, **kw)
        assert st == 1 and untouched, name
    assert _trace(False) == []
    # the same call, unbroken, is accepted and writes
    _trace(True)
    st, untouched = R.raw_call(L, x_d=ptr, label_strides=(4 + 3, 5 + 3))
    assert st == 0 and not untouched and _trace(False) == ["label_map"]
