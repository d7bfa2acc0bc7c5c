"""Shared by the detector-node tests: the extra reference symbols (concat, upsample, YOLO head, detections) bound on
oracle/_ref/libbcnn_ref.so, and the detection-list comparison."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_bind as rb


def need_ref():
    if not rb.available():
        pytest.skip("oracle/_ref/libbcnn_ref.so not present (built from the reference tree by oracle/Makefile)")


def ref_lib():
    """the reference library with argtypes for the symbols oracle/ref_bind.py does not declare"""
    from bcnn_amd import capi
    L = rb.lib()
    vp, i, f, cp = C.c_void_p, C.c_int, C.c_float, C.c_char_p
    L.bcnn_add_concat_layer.argtypes = [vp, i, C.POINTER(cp), cp]
    L.bcnn_add_concat_layer.restype = i
    L.bcnn_add_upsample_layer.argtypes = [vp, i, cp, cp]
    L.bcnn_add_upsample_layer.restype = i
    L.bcnn_add_yolo_layer.argtypes = [vp, i, i, i, i, C.POINTER(i), C.POINTER(f), cp, cp]
    L.bcnn_add_yolo_layer.restype = i
    L.bcnn_yolo_get_detections.argtypes = [vp, i, i, i, i, i, f, i, C.POINTER(i)]
    L.bcnn_yolo_get_detections.restype = C.POINTER(capi.Detection)  # same struct layout in both libraries
    return L


def ref_concat(ref, srcs, dst):
    arr = (C.c_char_p * len(srcs))(*[s.encode() for s in srcs])
    assert ref.L.bcnn_add_concat_layer(ref.net, len(srcs), arr, dst.encode()) == 0
    return ref.num_nodes() - 1


def ref_upsample(ref, size, src, dst):
    assert ref.L.bcnn_add_upsample_layer(ref.net, size, src.encode(), dst.encode()) == 0
    return ref.num_nodes() - 1


def ref_yolo(ref, num, classes, mask, anchors, src, dst, coords=4):
    m = (C.c_int * len(mask))(*mask)
    a = (C.c_float * len(anchors))(*anchors)
    assert ref.L.bcnn_add_yolo_layer(ref.net, num, classes, coords, len(anchors) // 2, m, a, src.encode(),
                                     dst.encode()) == 0
    return ref.num_nodes() - 1


def ref_detections(ref, batch, w, h, netw, neth, thresh, relative):
    from bcnn_amd import capi
    n = C.c_int(0)
    dets = ref.L.bcnn_yolo_get_detections(ref.net, batch, w, h, netw, neth, thresh, relative, C.byref(n))
    return capi.detections_to_list(dets, n.value)


def assert_same_detections(got, want, tol, skip_near=None):
    """element-wise after the NMS sort (both lists come out sorted by objectness); `skip_near(det)` marks reference boxes
    that may be missing or extra on one side (objectness within tolerance of the threshold): those are dropped from
    both lists first, matched by position. Returns how many were dropped."""
    dropped = 0
    if skip_near is not None:
        keep_w = [d for d in want if not skip_near(d)]
        keep_g = [d for d in got if not skip_near(d)]
        dropped = (len(want) - len(keep_w)) + (len(got) - len(keep_g))
        want, got = keep_w, keep_g
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, r) in enumerate(zip(got, want)):
        for key in ("x", "y", "w", "h", "objectness"):
            assert abs(g[key] - r[key]) <= tol * max(1.0, abs(r[key])), (k, key, g[key], r[key])
        np.testing.assert_allclose(g["prob"], r["prob"], rtol=tol, atol=tol, err_msg="box %d" % k)
    return dropped
