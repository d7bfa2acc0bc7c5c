"""The stand-alone activation (csrc/activation.hip) through every branch of chan_reduce.h's launch_chan_map, which the
act_* goldens -- all (n, c, hw) = (2, 3, 37), the first sweep of flat_map_kernel -- leave out:
  non-PReLU (one long plane of `size` elements)
      size < 1024            flat_map_kernel; 1 and 1023 end in a partial float4 group
      1024                   the first plane_map_kernel size, one chunk
      1027                   plane_map, a 3-element tail; repeated one float off a 16-byte boundary (scalar bodies)
      4096 + 5               two chunks, the second holds the 5-element remainder
      9001                   three chunks, HW % 4 == 1
  PReLU (n, c, hw)
      (4, 5, 1) (3, 4, 2) (2, 7, 3)   a float4 group straddles several planes (the full-connected node runs hw = 1)
      (2, 3, 1025)                    plane_map, every plane but the first starts off a 16-byte boundary
      (2, 3, 2048)                    plane_map, aligned planes
      (32, 96, 729)                   2 239 488 elements: the second sweep of flat_map_kernel with non-zero step_in and
                                      step_c, and a slope-gradient reduction over 6 splits per channel
The reference is the oracle's orc_act_forward / orc_act_backward (pinned to the reference by the act_* goldens)."""
import numpy as np
import pytest

from oracle import orc_bind as ob
from tests import _golden as G
from tests import _next_ref as R
from tests.test_hip_parity import ACT_TOL, REL_TOL

pytestmark = pytest.mark.gpu

F32 = np.float32
PLAIN_SIZES = [(1, 0), (1023, 0), (1024, 0), (1027, 0), (1027, 1), (4096 + 5, 0), (9001, 0)]   # (size, shift in floats)
PRELU_SHAPES = [(4, 5, 1), (3, 4, 2), (2, 7, 3), (2, 3, 1025), (2, 3, 2048), (32, 96, 729)]


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401
    from bcnn_amd import _lib
    return _lib.load()


def values(rs, size):
    x = rs.uniform(-2, 2, size).astype(F32)
    x[rs.permutation(size)[:max(1, size // 32)]] = F32(0)
    return x


def compare(tag, act, got, want):
    if R.FWD_BAR[act] == R.EXACT and R.BWD_BAR[act] == R.EXACT:
        R.assert_bits(tag, got, want)
    else:
        G.assert_close(tag, got, want, ACT_TOL, rtol=ACT_TOL, afrac=ACT_TOL / 10)


@pytest.mark.parametrize("act", [R.ACT_RELU, R.ACT_LOGISTIC], ids=lambda a: R.ACT_NAMES[a])
@pytest.mark.parametrize("size,shift", PLAIN_SIZES, ids=lambda v: str(v))
def test_activation_without_slopes(L, size, shift, act):
    O = ob.lib()
    rs = np.random.RandomState(size + shift)
    x = values(rs, size)
    tag = "act/%s/%d+%d" % (R.ACT_NAMES[act], size, shift)
    gx = R.Guarded(x, shift)
    L.bcnn_hip_activation_forward(gx.ptr, size, act, None, 1, 1)
    L.bcnn_hip_sync()
    y = x.copy()
    O.orc_act_forward(ob.P(y), size, None, 1, 1, act)
    compare(tag + "/y", act, gx.read(), y)
    # backward from the post-activation values
    dy = rs.uniform(-1, 1, size).astype(F32)
    gy, gd = R.Guarded(y, shift), R.Guarded(dy, shift)
    L.bcnn_hip_activation_backward(gy.ptr, gd.ptr, size, act, None, None, 1, 1)
    L.bcnn_hip_sync()
    gy.assert_unchanged("y")
    dx = dy.copy()
    O.orc_act_backward(ob.P(y), ob.P(dx), size, None, None, 1, 1, act)
    R.assert_bits(tag + "/dx", gd.read(), dx)      # RELU: a 0 / 1 factor; LOGISTIC: (1 - y) * y * dy, three roundings


@pytest.mark.parametrize("n,c,hw", PRELU_SHAPES, ids=lambda v: str(v))
def test_prelu_per_channel_maps_and_slope_gradient(L, n, c, hw):
    O = ob.lib()
    size = n * c * hw
    rs = np.random.RandomState(size)
    x = values(rs, size)
    slopes = rs.uniform(0.05, 0.9, c).astype(F32) * np.where(np.arange(c) % 2, F32(-1), F32(1))   # both signs
    tag = "prelu/%dx%dx%d" % (n, c, hw)
    gx, gs = R.Guarded(x), R.Guarded(slopes)
    L.bcnn_hip_activation_forward(gx.ptr, size, R.ACT_PRELU, gs.ptr, hw, c)
    L.bcnn_hip_sync()
    gs.assert_unchanged("slopes")
    y = x.copy()
    O.orc_act_forward(ob.P(y), size, ob.P(slopes), hw, c, R.ACT_PRELU)
    assert np.array_equal(y, R.act_forward32(x, R.ACT_PRELU, slopes[R.chan_index(n, c, hw)]))      # the numpy form agrees
    R.assert_bits(tag + "/y", gx.read(), y)

    dy = rs.uniform(-1, 1, size).astype(F32)
    ds0 = rs.uniform(-1, 1, c).astype(F32)          # non-zero: the slope gradient accumulates
    dx = dy.copy()
    ds_orc = ds0.copy()
    O.orc_act_backward(ob.P(y), ob.P(dx), size, ob.P(slopes), ob.P(ds_orc), hw, c, R.ACT_PRELU)
    ds_want = ds0.astype(np.float64) + R.prelu_dslopes64(y, dy, n, c, hw)
    G.assert_close(tag + "/dslopes(oracle)", ds_orc, ds_want, REL_TOL)     # the float64 sum states the oracle's loop
    for with_ds in (True, False):
        gy, gd, gs, gds = R.Guarded(y), R.Guarded(dy), R.Guarded(slopes), R.Guarded(ds0)
        L.bcnn_hip_activation_backward(gy.ptr, gd.ptr, size, R.ACT_PRELU, gs.ptr, gds.ptr if with_ds else None, hw, c)
        L.bcnn_hip_sync()
        gy.assert_unchanged("y")
        gs.assert_unchanged("slopes")
        R.assert_bits(tag + "/dx", gd.read(), dx)
        if with_ds:
            G.assert_close(tag + "/dslopes", gds.read(), ds_want, REL_TOL)
        else:
            gds.assert_unchanged("dslopes when NULL is passed")
