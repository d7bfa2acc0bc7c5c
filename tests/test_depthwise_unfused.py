"""The unfused tier of the depthwise ladder (bcnn_amd/csrc/depthwise.hip) against the oracle (oracle/bcnn_oracle.c orc_dw_forward /
orc_dw_backward, a restatement of bcnn_depthwise_conv_layer.c:165-293, :295-547): the register-window 3x3 kernels
(dw3_fwd_kernel, dw3_bwd_weight_kernel, dw3_bwd_data_s1_kernel, dw3_bwd_data_kernel<2> / <0>) and the kernels for any shape
(dw_fwd_kernel, dw_bwd_weight_kernel<3> / <5>, dw_bwd_weight_tap_kernel, dw_bwd_data_kernel). Three kinds of layer fall to
them: 3x3 with pad != 1 or stride >= 3, every other kernel size, and 3x3 / pad 1 layers whose rows are too wide for both fused
families (depthwise_march.hip: at most 64 column groups; depthwise_lds.hip: W <= 512). The shapes are the smallest that have
several workgroups, several splits of the weight-gradient sum with a ragged last one, an odd OH under DW_VR = 2, OW % 4 != 0,
both tap parities of the stride-2 data kernel, a second turn of the grid-stride loops, and aligned as well as misaligned
tensors (the 16-byte and the per-element window loads of dw_window on the same data). Every case asserts the kernels the
dispatch trace names: a case that lands on another branch fails.

Forward and the data gradient are the reference's own sums in the reference's tap order (separate multiply and add): bit-exact.
Weight / bias gradients are sums over the batch in a different (fixed) order: 1e-4 relative, and bit-identical from run to run."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import orc_bind as ob

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
ACT_NONE, ACT_TANH, ACT_RELU, ACT_SOFTPLUS, ACT_LRELU, ACT_CLAMP, ACT_LOGISTIC = 0, 1, 2, 4, 5, 7, 9

# what the trace has to say: (forward, weight gradient, data gradient)
W3_S1 = ("dw3_fwd_kernel<1>", "dw3_bwd_weight_kernel<1>", "dw3_bwd_data_s1_kernel")
W3_S2 = ("dw3_fwd_kernel<2>", "dw3_bwd_weight_kernel<2>", "dw3_bwd_data_kernel<2>")
K3_S3 = ("dw_fwd_kernel", "dw_bwd_weight_kernel<3>", "dw3_bwd_data_kernel<0>")
K5 = ("dw_fwd_kernel", "dw_bwd_weight_kernel<5>", "dw_bwd_data_kernel")
TAP = ("dw_fwd_kernel", "dw_bwd_weight_tap_kernel", "dw_bwd_data_kernel")

# (n, c, h, w, k, s, p, act), kernels
CASES = [
    # register-window 3x3, pad != 1: the per-element window loads
    ((2, 3, 41, 52, 3, 1, 0, ACT_RELU), W3_S1),    # OH = 39 odd under DW_VR = 2, OW = 50 (% 4 == 2), six workgroups
    ((2, 3, 41, 52, 3, 2, 0, ACT_LRELU), W3_S2),
    ((1, 2, 37, 48, 3, 1, 2, ACT_CLAMP), W3_S1),
    ((2, 3, 40, 50, 3, 2, 2, ACT_NONE), W3_S2),    # even pad: parity 0 of the stride-2 data kernel; rows of 200 bytes
    ((1, 2, 9, 12, 3, 2, 3, ACT_RELU), W3_S2),     # odd pad: parity 1; windows that lie wholly in the padding
    # register-window 3x3, pad 1, rows too wide for both fused families (516 > 512 floats; more than 64 column groups)
    ((1, 2, 21, 516, 3, 1, 1, ACT_RELU), W3_S1),   # M = 10836 per channel: three splits, ragged last; 16-byte window loads
    ((1, 2, 21, 516, 3, 2, 1, ACT_LRELU), W3_S2),  # OW = 258
    ((1, 2, 6, 518, 3, 1, 1, ACT_NONE), W3_S1),    # W % 4 == 2
    # stride 3 on 3x3
    ((2, 3, 40, 44, 3, 3, 1, ACT_RELU), K3_S3),
    # 5x5
    ((2, 4, 48, 44, 5, 1, 2, ACT_RELU), K5),       # M = 4224: two splits of 2112
    ((2, 4, 47, 45, 5, 2, 2, ACT_LRELU), K5),
    ((4, 16, 96, 96, 5, 1, 2, ACT_RELU), K5),      # 589824 outputs: the grid-stride loops of forward and data gradient turn over
    # any other size: one tap per workgroup
    ((2, 3, 40, 36, 7, 2, 3, ACT_RELU), TAP),
    ((1, 3, 17, 19, 2, 2, 0, ACT_NONE), TAP),
    ((1, 2, 18, 22, 4, 2, 1, ACT_RELU), TAP),
    ((2, 5, 9, 11, 1, 1, 0, ACT_LRELU), TAP),
    # expensive activations: a pass of their own behind / in front of the same kernels
    ((2, 3, 20, 24, 5, 1, 2, ACT_TANH), K5),
    ((2, 3, 20, 24, 5, 1, 2, ACT_SOFTPLUS), K5),
    ((2, 3, 20, 24, 5, 1, 2, ACT_LOGISTIC), K5),
]
WIDE = (1, 2, 21, 516, 3, 1, 1, ACT_RELU)
FIVE = (2, 4, 48, 44, 5, 1, 2, ACT_RELU)
NO_DX = (2, 3, 40, 44, 3, 3, 1, ACT_RELU)


def _trace_start():
    from bcnn_amd import _lib
    _lib.load().bcnn_hip_trace_enable(1)


def _trace_stop():
    """the kernels named since _trace_start, in launch order"""
    from bcnn_amd import _lib
    L = _lib.load()
    n = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return buf.value.decode().split()


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    den = float(np.abs(b).max())
    d = float(np.abs(a.astype(np.float64) - b).max())
    return d if den == 0 else d / den


def _case(n, c, h, w, k, s, p, act, seed=0):
    """tests/test_depthwise_lds.py::_case for any (k, s, p)"""
    rs = np.random.RandomState(1000 + seed)
    x = rs.uniform(-1, 1, (n, c, h, w)).astype(np.float32)
    wt = rs.uniform(-0.5, 0.5, (c * k * k,)).astype(np.float32)
    bias = rs.uniform(-0.2, 0.2, (c,)).astype(np.float32)
    bias[0] = 0.0  # the reference skips the add for 0 and 1 (bcnn_add_bias quirk)
    if c > 1:
        bias[1] = 1.0
    oh, ow = ob.conv_out_hw(h, w, k, s, p)
    dy = rs.uniform(-1, 1, (n, c, oh, ow)).astype(np.float32)
    dx0 = rs.uniform(-1, 1, (n, c, h, w)).astype(np.float32)
    dw0 = rs.uniform(-1, 1, (c * k * k,)).astype(np.float32)
    db0 = rs.uniform(-1, 1, (c,)).astype(np.float32)
    return dict(n=n, c=c, h=h, w=w, k=k, s=s, p=p, act=act, input_grad=1, x=x, wt=wt, bias=bias, dy=dy, dx0=dx0,
                dw0=dw0, db0=db0)


def _dev(a, off=0, fill=None):
    """a device tensor of a's shape that starts `off` floats into its allocation, holding a (or `fill`)"""
    buf = torch.empty(a.size + off, dtype=torch.float32, device=DEV)
    t = buf[off:off + a.size].view(a.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * off
    if fill is None:
        t.copy_(torch.tensor(a))  # a copy: the oracle's cached results are read-only
    else:
        t.fill_(fill)
    return t


def _run(cs, off=0):
    """forward, backward accumulating, backward overwriting; x, y, dy and dx start `off` floats past a 16-byte boundary"""
    from bcnn_amd import ops
    k, s, p, act = cs["k"], cs["s"], cs["p"], cs["act"]
    exp = _oracle(cs)
    x, wt, bias = _dev(cs["x"], off), _dev(cs["wt"]), _dev(cs["bias"])
    y = _dev(exp["y"], off, fill=7.0)
    _trace_start()
    ops.depthwise_forward(x, wt, bias, y, k, s, p, act)
    t_fwd = _trace_stop()
    # backward on the oracle's own forward output: accumulate onto the given dx / dw / db, dy rewritten in place
    yt = _dev(exp["y"], off)
    dy, dx, dw, db = _dev(cs["dy"], off), _dev(cs["dx0"], off), _dev(cs["dw0"]), _dev(cs["db0"])
    _trace_start()
    ops.depthwise_backward(x, wt, yt, dy, dx, dw, db, k, s, p, act)
    t_bwd = _trace_stop()
    # the executor's no-fill mode: dx = 0 + sums, whatever the buffer held
    dy2, dx2, dw2, db2 = _dev(cs["dy"], off), _dev(cs["dx0"], off, fill=9.0), _dev(cs["dw0"]), _dev(cs["db0"])
    _trace_start()
    ops.depthwise_backward(x, wt, yt, dy2, dx2, dw2, db2, k, s, p, act, overwrite=True)
    t_ovw = _trace_stop()
    torch.cuda.synchronize()
    return dict(y=_np(y), dy=_np(dy), dx=_np(dx), dw=_np(dw), db=_np(db), dy2=_np(dy2), dx2=_np(dx2), dw2=_np(dw2), db2=_np(db2),
                trace=(t_fwd, t_bwd, t_ovw))


_ORACLE = {}


def _oracle(cs):
    """the oracle's results for a case of CASES (by shape: computed once), started from dx0 and from zeros"""
    key = tuple(cs[q] for q in ("n", "c", "h", "w", "k", "s", "p", "act"))
    if key not in _ORACLE:
        exp = ob.orc_dw(cs)
        cz = dict(cs)
        cz["dx0"] = np.zeros_like(cs["dx0"])
        exp["dx_from_zero"] = ob.orc_dw(cz)["dx"]
        for v in exp.values():
            v.setflags(write=False)
        _ORACLE[key] = exp
    return _ORACLE[key]


def _check(cs, got, kernels):
    exp = _oracle(cs)
    fwd, wgrad, dgrad = kernels
    assert got["trace"] == ([fwd], [wgrad, dgrad], [wgrad, dgrad]), got["trace"]
    if cs["act"] not in (ACT_TANH, ACT_SOFTPLUS, ACT_LOGISTIC):
        assert np.array_equal(got["y"], exp["y"])
        assert np.array_equal(got["dy"], exp["dy_out"]) and np.array_equal(got["dy2"], exp["dy_out"])
        assert np.array_equal(got["dx"], exp["dx"])
        assert np.array_equal(got["dx2"], exp["dx_from_zero"])
    else:  # exp() in double on both sides, libm against ocml
        assert _rel(got["y"], exp["y"]) <= 1e-6
        assert _rel(got["dy"], exp["dy_out"]) <= 1e-6 and _rel(got["dy2"], exp["dy_out"]) <= 1e-6
        assert _rel(got["dx"], exp["dx"]) <= 1e-6
        assert _rel(got["dx2"], exp["dx_from_zero"]) <= 1e-6
    assert _rel(got["dw"] - cs["dw0"], exp["dw"] - cs["dw0"]) <= TOL
    assert _rel(got["db"] - cs["db0"], exp["db"] - cs["db0"]) <= TOL
    # run-to-run determinism of the two-level sums
    assert np.array_equal(got["dw2"].view(np.int32), got["dw"].view(np.int32))
    assert np.array_equal(got["db2"].view(np.int32), got["db"].view(np.int32))


@pytest.mark.parametrize("shape,kernels", CASES, ids=["n%d_c%d_%dx%d_k%d_s%d_p%d_act%d" % c[0] for c in CASES])
def test_forward_and_backward_against_the_oracle(shape, kernels):
    cs = _case(*shape)
    _check(cs, _run(cs), kernels)


def test_wide_rows_misaligned_take_the_per_element_window_loads_to_the_same_bits():
    """the 516-wide layer with x, y, dy and dx one float past a 16-byte boundary: dw_window's per-element loads and the scalar
    stores instead of the 16-byte ones, on the same data -- the bits of the aligned run, weight gradient included"""
    cs = _case(*WIDE)
    aligned, shifted = _run(cs), _run(cs, off=1)
    _check(cs, shifted, W3_S1)
    _check(cs, aligned, W3_S1)
    for key in ("y", "dy", "dx", "dw", "db", "dx2"):
        assert np.array_equal(aligned[key].view(np.int32), shifted[key].view(np.int32)), key


def test_without_a_source_gradient_only_dy_and_the_bias_gradient_change():
    """dx = NULL: dy *= act'(y) and dbias += its sums; the weight gradient is skipped with the data gradient
    (bcnn_depthwise_conv_layer.c:318, :432)"""
    from bcnn_amd import ops
    cs = _case(*NO_DX)
    cs["input_grad"] = 0
    exp = ob.orc_dw(cs)
    assert np.array_equal(exp["dw"], cs["dw0"])  # the oracle leaves it alone too
    x, wt, yt = _dev(cs["x"]), _dev(cs["wt"]), _dev(exp["y"])
    dy, dw, db = _dev(cs["dy"]), _dev(cs["dw0"]), _dev(cs["db0"])
    _trace_start()
    ops.depthwise_backward(x, wt, yt, dy, None, dw, db, cs["k"], cs["s"], cs["p"], cs["act"])
    trace = _trace_stop()
    torch.cuda.synchronize()
    assert trace == [], trace  # neither the weight-gradient nor a data-gradient kernel
    assert np.array_equal(_np(dy), exp["dy_out"])
    assert not np.array_equal(exp["dy_out"], cs["dy"])
    assert _rel(_np(db) - cs["db0"], exp["db"] - cs["db0"]) <= TOL
    assert np.array_equal(_np(dw).view(np.int32), cs["dw0"].view(np.int32))


def test_a_layer_without_output_pixels_touches_nothing():
    """5x5 without padding on a 3 x 3 plane: (3 - 5) / 1 + 1 = -1 rows and columns -- no output, not (-1) * (-1) = one pixel per
    plane. The C ABI itself, on sentinel-filled buffers."""
    from bcnn_amd import _lib
    L = _lib.load()
    n, c, h, w, k = 2, 3, 3, 3, 5
    names = ("x", "wt", "bias", "y", "dy", "dx", "dw", "db")
    buf = {q: torch.full((256,), 3.0 + i, device=DEV) for i, q in enumerate(names)}
    P = lambda q: buf[q].data_ptr()
    _trace_start()
    L.bcnn_hip_depthwise_forward(P("x"), P("wt"), P("bias"), P("y"), n, c, h, w, k, 1, 0, ACT_RELU)
    for overwrite in (0, 1):
        L.bcnn_hip_depthwise_backward(P("x"), P("wt"), P("y"), P("dy"), P("dx"), P("dw"), P("db"), n, c, h, w, k, 1, 0,
                                      ACT_RELU, overwrite)
    trace = _trace_stop()
    torch.cuda.synchronize()
    assert trace == [], trace
    for i, q in enumerate(names):
        assert float(buf[q].min()) == float(buf[q].max()) == 3.0 + i, q


def test_an_inf_stays_in_the_windows_that_cover_it():
    """one Inf in x at (3, 7) of the 5x5 / stride 1 layer reaches exactly the 5 x 5 outputs whose window covers it; the taps
    in the padding are skipped, not multiplied by zero into NaN"""
    from bcnn_amd import ops
    cs = _case(*FIVE)
    cs["x"][0, 1, 3, 7] = np.inf
    cs["wt"] = np.abs(cs["wt"]) + np.float32(0.125)  # positive taps: +Inf survives the ReLU
    exp = ob.orc_dw(cs)
    y = _dev(exp["y"], fill=7.0)
    _trace_start()
    ops.depthwise_forward(_dev(cs["x"]), _dev(cs["wt"]), _dev(cs["bias"]), y, cs["k"], cs["s"], cs["p"], cs["act"])
    assert _trace_stop() == ["dw_fwd_kernel"]
    yn = _np(y)
    covered = np.zeros(yn.shape, bool)
    covered[0, 1, 1:6, 5:10] = True  # oh - 2 <= 3 <= oh + 2, ow - 2 <= 7 <= ow + 2
    assert not np.isnan(yn).any()
    assert (yn[covered] == np.inf).all() and np.isfinite(yn[~covered]).all()
    assert np.array_equal(yn, exp["y"])
