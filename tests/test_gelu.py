"""GELU, the exact form x Phi(x) = 0.5 x (1 + erf(x / sqrt 2)), through the activation worker (activation.hip: gated_fwd /
gated_bwd) against float64 (torch.erf on CPU doubles). The kernels evaluate in double and round once: one rounding of a
double result is 2^-24 relative, the factor 2 covers the double erf; the bar is 2^-23 |want| + 2^-149."""
import math

import numpy as np
import pytest
import torch

from tests.test_gated_activations import _dev

pytestmark = pytest.mark.gpu
F32 = np.float32
# 0, +-tiny, +-1, the minimum of x Phi(x), both tails: where 1 + erf cancels (-6), where it is 0 (-10, -40) and 1 (6, 10, 40)
VALUES = np.array([0.0, 1e-30, -1e-30, 1.0, -1.0, -0.7517916, 6.0, -6.0, 10.0, -10.0, 40.0, -40.0], F32)


def _reference(x, g):
    xd, gd = torch.tensor(x, dtype=torch.float64), torch.tensor(g, dtype=torch.float64)
    cdf = 0.5 * (1.0 + torch.erf(xd / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * xd * xd) / math.sqrt(2.0 * math.pi)
    return (xd * cdf).numpy(), (gd * (cdf + xd * pdf)).numpy()


def _within_the_bar(got, want, what):
    err, bar = np.abs(got.astype(np.float64) - want), 2.0 ** -23 * np.abs(want) + 2.0 ** -149
    print(what, "worst error / bar:", (err / bar).max())
    assert (err <= bar).all(), (what, np.flatnonzero(err > bar), got[err > bar], want[err > bar])


@pytest.mark.parametrize("size,offset", [(s, o) for s in (1, 3, 4, 5, 1027) for o in (0, 1)])
def test_forward_and_backward_against_float64(size, offset):
    from bcnn_amd import capi, ops
    act = ops.ACT_ALL["gelu"]
    assert act == capi.ACT_GELU == 15
    x = np.resize(np.roll(VALUES, -size), size)   # every value is met: the sizes below 12 start at different ones
    g = np.random.RandomState(size).uniform(-2, 2, size).astype(F32)
    y64, dx64 = _reference(x, g)
    t, kept = _dev(x, offset), _dev(np.full_like(x, 7.0), offset)
    ops.activation_forward_keep(t, kept, act)
    _within_the_bar(t.cpu().numpy(), y64, "forward")
    assert np.array_equal(kept.cpu().numpy().view(np.int32), x.view(np.int32)), "the saved input is the input"
    t2 = _dev(x, offset)
    ops.activation_forward(t2, act)
    assert torch.equal(t2.view(torch.int32), t.view(torch.int32)), "a null buffer changes nothing in y"
    tg = _dev(g, offset)
    ops.activation_backward_from_input(kept, tg, act)
    _within_the_bar(tg.cpu().numpy(), dx64, "backward")


def test_the_backward_from_the_output_is_refused():
    """as for hard-swish, swish and mish: every builder with a fused activation refuses it and adds nothing; the stand-alone
    node takes it and keeps its input"""
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=4, h=4, c=2, n=1)
    net.conv(2, 1, 1, 0, src="input", dst="a")
    net.conv(2, 1, 1, 0, src="input", dst="b")
    L, h, act = net.L, net.net, capi.ACT_GELU
    nodes = L.bcnn_get_num_nodes(h)
    for refused in (lambda: L.bcnn_add_convolutional_layer(h, 2, 1, 1, 0, 1, 0, capi.FILLER_XAVIER, act, 0, b"a", b"x"),
                    lambda: L.bcnn_add_depthwise_conv_layer(h, 3, 1, 1, 0, capi.FILLER_XAVIER, act, b"a", b"x"),
                    lambda: L.bcnn_add_fullc_layer(h, 5, capi.FILLER_XAVIER, act, 0, b"a", b"x"),
                    lambda: L.bcnn_add_eltwise_layer(h, act, b"a", b"b", b"x")):
        assert refused() == 1 and L.bcnn_get_num_nodes(h) == nodes
    node = net.activation(act, "a")
    assert net.node_activation(node) == act and net.node_state(node, 0)
    net.close()
