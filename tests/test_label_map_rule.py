"""The host side of the label maps, without a device: bcnn_hip_label_map_fit against the numpy
restatement and against the extents bcnn_fill_tensor_with_images documents, bcnn_hip_label_maps_plan on ragged batches and
at the 2^31-byte limit (no memory is allocated: the plan is arithmetic), every refusal of bcnn_hip_label_maps_batch that
comes before the device is touched, iou_from_confusion on a hand-made matrix, and the symbols in both libraries and in the
Python bindings. All of it fails without the feature."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _label_map_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRETCH, LETTERBOX = R.STRETCH, R.LETTERBOX

# (W, H) planes and (iw, ih) images: wide, tall, square, one-pixel, extent-equal, and extents whose letterbox divisions
# leave a remainder or an odd margin
PLANES = [(16, 12), (9, 7), (416, 416), (513, 513), (1, 1), (12, 16)]
IMAGES = [(40, 10), (10, 40), (16, 12), (12, 16), (9, 7), (1, 1), (500, 375), (375, 500), (333, 500), (7, 7), (1, 40),
          (40, 1), (417, 415), (513, 513), (1000, 3)]


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


@pytest.mark.parametrize("kind", [STRETCH, LETTERBOX])
def test_fit_equals_the_restatement_and_the_fill(kind):
    from bcnn_amd import ops
    seen = set()
    for W, H in PLANES:
        for iw, ih in IMAGES:
            got, want = ops.label_map_fit(kind, W, H, iw, ih), R.fit(kind, W, H, iw, ih)
            assert got == want, (kind, W, H, iw, ih, got, want)
            if got is None:
                seen.add("refused")
                continue
            out_w, out_h, rx, ry, rw, rh = got
            # what bcnn_fill_tensor_with_images documents for the same image: the rectangle is where the fill pasted it
            new_w, new_h, x_off, y_off = R.fill_extent(kind, W, H, iw, ih)
            assert (out_w, out_h) == (iw, ih) and (rx, ry, rw, rh) == (x_off, y_off, new_w, new_h)
            assert 0 <= rx and rx + rw <= W and 0 <= ry and ry + rh <= H and rw >= 1 and rh >= 1
            seen.add("full" if (rw, rh) == (W, H) else ("bars_x" if rh == H else "bars_y"))
    assert seen == ({"full"} if kind == STRETCH else {"full", "bars_x", "bars_y", "refused"}), seen


def test_fit_refusals():
    from bcnn_amd import _lib, ops
    assert ops.label_map_fit(LETTERBOX, 16, 12, 1000, 3) is None      # new_h = 3 * 16 // 1000 = 0
    for args in [(2, 16, 12, 4, 4), (-1, 16, 12, 4, 4), (STRETCH, 0, 12, 4, 4), (STRETCH, 16, 0, 4, 4),
                 (STRETCH, 16, 12, 0, 4), (LETTERBOX, 16, 12, 4, -3)]:
        assert ops.label_map_fit(*args) is None, args                 # (the wrapper asserts that *out kept its poison)
    assert _lib.load().bcnn_hip_label_map_fit(STRETCH, 16, 12, 4, 4, None) == 1


def test_plan_of_ragged_batches():
    from bcnn_amd import ops
    sizes = [(9, 7), (13, 11), (4, 3), (1, 1), (33, 17), (16, 8), (36, 28)]
    images = [R.fit(STRETCH, 9, 7, w, h) for w, h in sizes]
    for with_truths in (False, True):
        got = ops.label_maps_plan(images, 21, 7, 9, with_truths)
        assert got == R.plan(images, with_truths)
    strides, offsets, total = got
    assert strides == [12, 16, 4, 4, 36, 16, 36]
    assert offsets == [0, 96, 272, 288, 304, 928, 1056] and total == 1056 + 36 * 28
    assert all(o % 16 == 0 for o in offsets) and all(s % 4 == 0 for s in strides)
    # one image, and extents at the edges of the four-byte rows and the sixteen-byte blocks
    for w, h in [(1, 1), (3, 5), (4, 4), (5, 3), (15, 1), (16, 1), (17, 1)]:
        im = [(w, h, 0, 0, 9, 7)]
        assert ops.label_maps_plan(im, 1, 7, 9) == R.plan(im) == ([(w + 3) // 4 * 4], [0], ((w + 3) // 4 * 4 * h + 15) // 16 * 16)


def test_plan_refuses_past_two_gib_without_allocating():
    from bcnn_amd import ops
    big = (65536, 32768, 0, 0, 9, 7)                 # 2^31 bytes exactly: the limit itself is accepted
    assert ops.label_maps_plan([big], 21, 7, 9) == ([65536], [0], 2 ** 31) == R.plan([big])
    assert ops.label_maps_plan([big, (1, 1, 0, 0, 9, 7)], 21, 7, 9) is None and R.plan([big, (1, 1, 0, 0, 9, 7)]) is None
    assert ops.label_maps_plan([big], 21, 7, 9, with_truths=True) is None        # the truths double it
    half = (65536, 16384, 0, 0, 9, 7)
    assert ops.label_maps_plan([half], 21, 7, 9, with_truths=True) == ([65536], [0], 2 ** 30)
    assert ops.label_maps_plan([half, (1, 1, 0, 0, 9, 7)], 21, 7, 9, with_truths=True) is None
    assert ops.label_maps_plan([(2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 9, 7)] * 3, 21, 7, 9) is None   # no wrap of the sum
    # what the plan refuses besides: classes, planes, rectangles, extents, an empty batch
    ok = (4, 4, 1, 1, 8, 6)
    assert ops.label_maps_plan([ok], 21, 7, 9) is not None
    for c, h, w in [(0, 7, 9), (257, 7, 9), (21, 0, 9), (21, 7, 0)]:
        assert ops.label_maps_plan([ok], c, h, w) is None, (c, h, w)
    assert ops.label_maps_plan([ok], 256, 7, 9) is not None
    for bad in [(0, 4, 0, 0, 9, 7), (4, 0, 0, 0, 9, 7), (4, 4, 0, 0, 0, 7), (4, 4, 0, 0, 9, 0), (4, 4, -1, 0, 9, 7),
                (4, 4, 0, -1, 9, 7), (4, 4, 1, 0, 9, 7), (4, 4, 0, 1, 9, 7), (4, 4, 0, 0, 10, 7), (4, 4, 0, 0, 9, 8),
                (4, 4, 2 ** 31 - 1, 0, 2, 2), (4, 4, 9, 0, 1, 1)]:
        assert ops.label_maps_plan([ok, bad], 21, 7, 9) is None, bad
    assert ops.label_maps_plan([], 21, 7, 9) is None


def test_batch_refusals_that_need_no_device():
    from bcnn_amd import _lib
    L = _lib.load()
    cases = dict(
        null_x=dict(x_d=None), n_zero=dict(n=0), num_zero=dict(num=0), num_above_n=dict(n=1),
        c_zero=dict(c=0), c_257=dict(c=257), h_zero=dict(h=0), w_zero=dict(w=0),
        out_w_zero=dict(images=((0, 3, 0, 0, 9, 7),)), out_h_negative=dict(images=((4, -1, 0, 0, 9, 7),)),
        roi_empty=dict(images=((4, 3, 0, 0, 0, 7),)), roi_leaves_right=dict(images=((4, 3, 1, 0, 9, 7),)),
        roi_leaves_bottom=dict(images=((4, 3, 0, 5, 9, 3),)), roi_negative=dict(images=((4, 3, -1, 0, 4, 4),)),
        label_stride_short=dict(label_strides=(4, 4)), truth_stride_short=dict(truths=True, truth_strides=(3, 5)),
        neither=dict(labels=False), truths_without_counts=dict(truths=True, counts=False),
        ignore_256=dict(truths=True, ignore=256), null_label_row=dict(null_row=("l", 1)),
        null_truth_row=dict(truths=True, null_row=("t", 0)),
        two_gib=dict(images=((65536, 32768, 0, 0, 9, 7), (1, 1, 0, 0, 9, 7)), labels=False, truths=True),
    )
    for name, kw in cases.items():
        st, untouched = R.raw_call(L, **kw)
        assert st == 1 and untouched, name
    # imgs NULL
    assert L.bcnn_hip_label_maps_batch(0x1000, 2, 5, 7, 9, 0, None, 1, 0x1000, None, None, None, -1, None, None, None) == 1


def test_iou_from_confusion_on_a_hand_made_matrix():
    from bcnn_amd import capi
    m = np.array([[5, 1, 0],
                  [2, 3, 0],
                  [0, 0, 0]], np.int64)
    iou, mean = capi.iou_from_confusion(m)
    assert iou[0] == 5 / 8 and iou[1] == 3 / 6 and np.isnan(iou[2])    # 5 / (6 + 7 - 5), 3 / (5 + 4 - 3), absent
    assert mean == (5 / 8 + 3 / 6) / 2
    iou, mean = capi.iou_from_confusion(np.zeros((2, 2), np.int64))
    assert np.isnan(iou).all() and np.isnan(mean)
    iou, mean = capi.iou_from_confusion([[0, 4], [0, 0]])             # a class that is only ever predicted wrongly
    assert list(iou) == [0.0, 0.0] and mean == 0.0


def test_symbols_are_declared_listed_and_exported():
    from bcnn_amd import _lib, capi, ops
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    hip = C.CDLL(_lib.LIB_PATH)
    for name, nargs in {"bcnn_hip_label_map_fit": 6, "bcnn_hip_label_maps_plan": 9, "bcnn_hip_label_maps_batch": 16}.items():
        assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1, name
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols(), name
        assert len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is C.c_int, name
        assert hasattr(hip, name), name
    image = re.search(r"typedef\s+struct\s+bcnn_hip_label_map_image\s*\{([^}]*)\}", header).group(1)
    assert re.sub(r"\s+", " ", image).strip() == "int out_w, out_h, roi_x, roi_y, roi_w, roi_h;"
    assert C.sizeof(ops.LabelMapImage) == 24
    public = _no_comments(open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read())
    decl = re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_get_label_maps_batch\s*\(([^;{]*)\)\s*;", public)
    assert len(decl) == 1
    assert re.sub(r"\s+", " ", decl[0]).strip() == (
        "bcnn_net *net, int tensor_index, int num_images, const int *widths, const int *heights, int fit, "
        "int align_corners, uint8_t *const *labels, const int *strides, bcnn_label_map_eval *eval")
    ev = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*bcnn_label_map_eval\s*;", public).group(1)
    assert re.sub(r"\s+", " ", ev).strip() == ("const uint8_t *const *truths; const int *strides; int ignore_label; "
                                                "int64_t *counts; int64_t ignored, out_of_range;")
    assert C.sizeof(capi.LabelMapEval) == 48
    assert hasattr(C.CDLL(capi.LIB_PATH), "bcnn_get_label_maps_batch")
    for name in ("label_maps", "label_map_fit", "label_maps_plan"):
        assert callable(getattr(ops, name)), name
    assert callable(capi.Net.label_maps) and callable(capi.iou_from_confusion)
    for build_file in (os.path.join("bcnn_amd", "host", "Makefile"), "CMakeLists.txt"):
        assert "bcnn_layers_label_map.c" in open(os.path.join(ROOT, build_file)).read(), build_file
    assert "label_map.hip" in open(os.path.join(ROOT, "bcnn_amd", "csrc", "Makefile")).read()
    rule = open(os.path.join(ROOT, "bcnn_amd", "csrc", "label_map_rule.h")).read()
    assert '#include "interp_rule.h"' in rule and '#include "softmax_loss_rule.h"' in rule
