"""Pins tests/_interp_ref.py, the numpy restatement of the bilinear interpolation rule, and the library's host code of
that rule (bcnn_hip_interp_axis_taps). No device.

Bar 1: the restatement's float32 forward against F.interpolate in float64:
    |y - y64| <= (8 * (H + W) + 6) * 2^-24 * max|x|.
    A tap position is at most four roundings of a quantity <= I, so l1 is off by at most 4 * I * 2^-24, and it multiplies a
    difference of at most 2 * max|x| per axis; the remaining 6 cover the six roundings of the blend. A wrong tap index
    misses the bar by orders of magnitude.
Bar 2: forward and backward equal torch's float32 BIT FOR BIT on data where every weight is dyadic (integer factors
    without align_corners, (O - 1) a multiple of (I - 1) with it) and the values are multiples of 1/16: every product and
    every sum is then exact, whatever the order.
Bar 3: bcnn_hip_interp_axis_taps equals the restatement's taps bit for bit on every (in, out, align_corners) with in, out
    in 1..40 and on (65, 513), (33, 257), (64, 512) -- a host build with contraction on would not."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _interp_ref as R

BAR1 = [((5, 7), (10, 14)), ((5, 7), (13, 9)), ((8, 8), (64, 64)), ((7, 5), (3, 2)), ((9, 12), (4, 5)), ((1, 1), (4, 4)),
        ((4, 6), (1, 1)), ((17, 19), (40, 31)), ((65, 65), (513, 513))]

@pytest.mark.parametrize("align_corners", [False, True])
@pytest.mark.parametrize("hw,out", BAR1)
def test_float32_forward_against_torch_float64(hw, out, align_corners):
    x = torch.randn((2, 3) + hw, generator=torch.Generator().manual_seed(hw[0] * 100 + out[1]))
    y64 = F.interpolate(x.double(), size=out, mode="bilinear", align_corners=align_corners).numpy()
    y = R.forward(x.numpy(), out[0], out[1], align_corners)
    assert y.dtype == np.float32 and y.shape == y64.shape
    err = np.abs(y.astype(np.float64) - y64).max()
    bound = (8 * (hw[0] + hw[1]) + 6) * 2.0 ** -24 * float(x.abs().max())
    print("max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound


@pytest.mark.parametrize("hw,out,align_corners", R.DYADIC)
def test_dyadic_weights_equal_torch_bit_for_bit(hw, out, align_corners):
    ref = R.dyadic_case(hw, out, align_corners)
    for axis in (0, 1):
        _, _, l0, l1 = R.axis_taps(hw[axis], out[axis], align_corners)
        assert np.array_equal(l0 * 16, np.round(l0 * 16)) and np.array_equal(l1 * 16, np.round(l1 * 16))
    y = R.forward(ref["x"].numpy(), out[0], out[1], align_corners)
    assert np.array_equal(y.view(np.int32), ref["y"].numpy().view(np.int32))
    dx, _, count = R.backward(ref["dy"].numpy(), hw[0], hw[1], align_corners)
    assert np.array_equal(dx, ref["grad"].numpy().astype(np.float64))   # exact sums: float64 holds torch's float32 bits
    got = (ref["dx0"].numpy().astype(np.float64) + dx).astype(np.float32)
    want = (ref["dx0"] + ref["grad"]).numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert bool((count > 0).all()) == (out[0] >= hw[0] and out[1] >= hw[1])  # only a downsampling skips elements


def test_library_host_taps_equal_the_restatement():
    from bcnn_amd import ops
    pairs = [(i, o) for i in range(1, 41) for o in range(1, 41)] + [(65, 513), (33, 257), (64, 512)]
    for size_in, size_out in pairs:
        for align_corners in (False, True):
            i0, i1, l1 = ops.interp_axis_taps(size_in, size_out, align_corners)
            r0, r1, _, rl1 = R.axis_taps(size_in, size_out, align_corners)
            key = (size_in, size_out, align_corners)
            assert np.array_equal(i0, r0) and np.array_equal(i1, r1), key
            assert np.array_equal(l1.view(np.int32), rl1.view(np.int32)), key
