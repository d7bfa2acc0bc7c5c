"""The records, tap tables and maps the label-warp tests share (CPU: tests/test_label_warp.py against the numpy
restatement; GPU: tests/test_augment_label.py against the host function). Records and taps come from the loader's own
fill_record through its exported door bcnn_loader_fill_record, so the float -> integer steps are the loader's."""
import ctypes as C
import math

import numpy as np

FLIP, SHIFT, SCALE, ROTATE = 1, 2, 4, 8
SIZES = [(5, 3), (16, 12), (33, 17), (1, 7), (7, 1)]     # (w, h); the last two: the one-sample axis
FILLS = [0, 21, 255]


def loader_record(w, h, flip=False, shift=None, scale=None, theta=None):
    """(record int32[8], taps int32[(w + h) * 2]) as fill_record makes them from these draws"""
    from bcnn_amd import capi
    L = capi.lib()
    fn = L.bcnn_loader_fill_record
    fn.restype = None
    fn.argtypes = [C.c_int] * 5 + [C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rec, taps = np.zeros(8, np.int32), np.zeros((w + h) * 2, np.int32)
    sx, sy = shift if shift is not None else (0, 0)
    fn(int(bool(flip)), int(shift is not None), int(sx), int(sy), int(scale is not None), float(scale or 0.0),
       int(theta is not None), float(theta or 0.0), w, h, rec.ctypes.data, taps.ctypes.data)
    return rec, taps


def tie_taps(w, h):
    """a SCALE record whose every tap is valid and whose fractions sit on and just below the tie: 8 on even columns / rows
    (index + 1 is taken where the extent is > 1), 7 on odd ones; every third row is not covered (index -1)"""
    rec = np.zeros(8, np.int32)
    rec[0] = SCALE
    taps = np.zeros((w + h, 2), np.int32)
    for i in range(w):
        taps[i] = (min(i, max(w - 2, 0)), 8 if i % 2 == 0 else 7)
    for j in range(h):
        taps[w + j] = (-1, 0) if j % 3 == 2 else (min(j, max(h - 2, 0)), 8 if j % 2 == 0 else 7)
    return rec, taps.reshape(-1)


def tie_rotation():
    """ca = 1.0, sa = -0.5 in 16.16: px = (x << 16) + 0x8000 (y - cy), py = (y << 16) - 0x8000 (x - cx): the fraction is
    exactly 0x8000 on every odd offset from the centre, and 0 on every even one"""
    rec = np.zeros(8, np.int32)
    rec[0], rec[3], rec[4] = ROTATE, 0x10000, -0x8000
    return rec, None


def label_map(w, h, seed):
    """classes 1 .. 20: none of them is one of FILLS"""
    return np.random.RandomState(seed).randint(1, 21, (h, w)).astype(np.uint8)


def cases(w, h):
    """(name, record, taps, expectation) with expectation in (None, "all_fill", "identity")"""
    out = [("identity", None, None, "identity"),
           ("flip",) + loader_record(w, h, flip=True) + (None,),
           ("shift",) + loader_record(w, h, shift=(2, -1)) + (None,),
           ("shift_zero",) + loader_record(w, h, shift=(0, 0)) + ("identity",),
           ("shift_beyond_x",) + loader_record(w, h, shift=(w + 3, 0)) + ("all_fill",),
           ("shift_beyond_y",) + loader_record(w, h, shift=(1, -h - 2)) + ("all_fill",),
           ("scale_half",) + loader_record(w, h, shift=(1, 1), scale=0.5) + (None,),
           ("scale_1.7",) + loader_record(w, h, scale=1.7) + (None,),
           ("rotate_0",) + loader_record(w, h, theta=0.0) + (None,),
           ("rotate_small",) + loader_record(w, h, theta=0.15) + (None,),
           ("rotate_quarter",) + loader_record(w, h, theta=math.pi / 2) + (None,),
           ("all_four",) + loader_record(w, h, flip=True, shift=(-2, 1), scale=1.3, theta=-0.2) + (None,),
           ("all_four_small",) + loader_record(w, h, flip=True, shift=(1, 0), scale=0.6, theta=0.3) + (None,),
           ("tie_taps",) + tie_taps(w, h) + (None,),
           ("tie_rotation",) + tie_rotation() + (None,)]
    if w == 1 or h == 1:   # no pixel has 0 <= m < extent - 1 on the one-sample axis: rotation covers nothing
        out = [(n, r, t, "all_fill" if (r is not None and r[0] & ROTATE) else e) for n, r, t, e in out]
    return out
