"""CPU: libbip's bip_warp_label_map (the double loop over bcnn_amd/host/bip_label_warp.h, the rule the segmentation-list
loader and the device kernel compile as well) against the independent numpy restatement tests/_label_warp_ref.py, byte for
byte; and the rule against the image path: a label follows its pixel."""
import ctypes as C

import numpy as np
import pytest

from bcnn_amd import ops
from tests import _label_cases as LC
from tests import _label_warp_ref as ref
from tests.test_data_loader import Aug, _u8


@pytest.mark.parametrize("w,h", LC.SIZES, ids=["%dx%d" % s for s in LC.SIZES])
def test_host_warp_equals_the_restatement(w, h):
    seen = set()
    for k, (name, rec, taps, expect) in enumerate(LC.cases(w, h)):
        m = LC.label_map(w, h, seed=k)
        for fill in LC.FILLS:
            got = ops.warp_label_map(m, rec, taps, fill)
            want = ref.warp(m, rec, taps, fill)
            assert got.shape == (h, w) and got.dtype == np.uint8
            assert np.array_equal(got, want), (name, fill, int((got != want).sum()))
            assert np.all((got == fill) | ((got >= 1) & (got <= 20))), (name, fill)   # a byte of the map, or F
            if expect == "all_fill":
                assert np.all(got == fill), (name, fill)
            if expect == "identity":
                assert np.array_equal(got, m), (name, fill)
            seen.add(name)
    assert {"flip", "shift", "scale_half", "scale_1.7", "rotate_quarter", "all_four", "tie_taps", "tie_rotation"} <= seen


def test_the_cases_reach_what_they_are_for():
    w, h = 16, 12
    by = {n: (r, t) for n, r, t, _ in LC.cases(w, h)}
    m = LC.label_map(w, h, seed=3)
    # scale 0.5: the resized image covers a corner, the border falls through to the shifted label
    rec, taps = by["scale_half"]
    t = taps.reshape(-1, 2)
    assert rec[0] & LC.SCALE and (t[:w, 0] >= 0).any() and (t[:w, 0] < 0).any() and (t[w:, 0] < 0).any()
    unscaled = rec.copy()
    unscaled[0] &= ~LC.SCALE
    got, plain = ops.warp_label_map(m, rec, taps, 255), ops.warp_label_map(m, unscaled, None, 255)
    uncovered = ~((t[w:, 0] >= 0)[:, None] & (t[:w, 0] >= 0)[None, :])
    assert uncovered.any() and np.array_equal(got[uncovered], plain[uncovered]) and not np.array_equal(got, plain)
    # the tap tie: frac 8 goes up, frac 7 stays
    rec, taps = by["tie_taps"]
    got = ops.warp_label_map(m, rec, taps, 255)
    assert got[0, 0] == m[1, 1] and got[1, 1] == m[1, 1] and got[0, 1] == m[1, 1] and got[1, 0] == m[1, 1]
    assert got[1, 2] == m[1, 3] and np.array_equal(got[2], m[2])            # row 2 is not covered: itself
    # the rotation tie: fraction 0x8000 goes up
    rec, _ = by["tie_rotation"]
    got = ops.warp_label_map(m, rec, None, 21)
    cx, cy = w // 2, h // 2
    # (cx, cy - 1): px = (cx << 16) - 0x8000 -> mx = cx - 1, tie -> cx; py = (cy - 1) << 16 -> cy - 1
    assert got[cy - 1, cx] == m[cy - 1, cx]
    # (cx - 1, cy - 1): px -> mx = cx - 2, tie -> cx - 1; py = ((cy - 1) << 16) + 0x8000 -> tie -> cy
    assert got[cy - 1, cx - 1] == m[cy, cx - 1]
    # rotation by a quarter turn leaves canvas on a 16 x 12 sample, rotation by 0 only the last row and column
    assert (ops.warp_label_map(m, by["rotate_quarter"][0], None, 255) == 255).any()
    zero = ops.warp_label_map(m, by["rotate_0"][0], None, 255)
    assert np.array_equal(zero[:h - 1, :w - 1], m[:h - 1, :w - 1]) and np.all(zero[h - 1] == 255) and np.all(zero[:, w - 1] == 255)


def test_refusals():
    m = LC.label_map(5, 3, seed=0)
    rec, taps = LC.loader_record(5, 3, scale=1.7)
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            ops.warp_label_map(m, rec, taps, bad)
    with pytest.raises(ValueError):
        ops.warp_label_map(m, rec, None, 255)               # SCALE without taps
    for at, value in ((0, 4), (0, -2), (2 * 5, 2), (2 * 5 + 4, -3)):   # a column index past w - 2, a row index past h - 2
        t = taps.copy()
        t[at] = value
        with pytest.raises(ValueError):
            ops.warp_label_map(m, rec, t, 255)


def test_a_label_follows_its_pixel_through_flip_and_shift():
    """An image whose bytes are 32 * class + 7 goes through the image path (bcnn_apply_data_augmentation with precomputed
    draws), its class map through the warp: image >> 5 == label wherever the label is not F. Range 6 keeps |x_ul|, |y_ul|
    <= 3 on 16 x 16, so at least 13 * 13 of 256 pixels (66 %) stay covered: the 60 % floor holds by the rule alone."""
    from bcnn_amd import capi
    L = capi.lib()
    L.bcnn_apply_data_augmentation.argtypes = [C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.POINTER(Aug),
                                               C.POINTER(C.c_uint8)]
    w = h = 16
    rs = np.random.RandomState(11)
    for flip in (0, 1):
        for sx in range(-3, 4):
            for sy in range(-3, 4):
                cls = rs.randint(0, 8, (h, w)).astype(np.uint8)
                img = (cls.astype(np.int32) * 32 + 7).astype(np.uint8).reshape(h, w, 1).copy()
                aug = Aug(range_shift_x=6, range_shift_y=6, random_fliph=flip, apply_fliph=flip, use_precomputed=1,
                          shift_x=sx, shift_y=sy)
                scratch = np.zeros_like(img)
                assert L.bcnn_apply_data_augmentation(_u8(img), w, h, 1, C.byref(aug), _u8(scratch)) == 0
                rec, taps = LC.loader_record(w, h, flip=bool(flip), shift=(sx, sy))
                lab = ops.warp_label_map(cls, rec, taps, 255)
                seen = lab != 255
                assert seen.mean() >= 0.6, (flip, sx, sy, float(seen.mean()))
                assert np.array_equal(img[:, :, 0][seen] >> 5, lab[seen]), (flip, sx, sy)
                assert np.all(img[:, :, 0][~seen] == 128)         # where the label is F the image shows its canvas
