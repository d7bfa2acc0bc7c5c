"""Every branch of the pooling dispatchers (bcnn_amd/csrc/pool.hip) against the oracle (oracle/bcnn_oracle.c orc_maxpool_* /
orc_avgpool_*, restatements of bcnn_maxpool_layer.c:145-191, :258-273 and bcnn_avgpool_layer.c:82-125) at the smallest shapes
where each can still go wrong: more than one workgroup per plane, rows that straddle waves, windows that overlap nine times or
leave pixels uncovered (stride > size), a single output row, the plane-count limit of the vectorised backward kernels, tensors
that start 4 bytes past a 16-byte boundary, and windows without a winner. Each case runs forward, then backward twice --
accumulating onto a random dx and overwriting a buffer of 7.0 -- and asserts the kernels the dispatch trace names: a case that
lands on another branch fails. y, indexes and dx are compared bit for bit; the inputs sit on a grid of 1/16 with a plateau
above everything else, so ties are everywhere and the order of the additions into one dx element matters."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import orc_bind as ob

gpu = pytest.mark.gpu
DEV = "cuda:0"
SAME, VALID, CAFFE = 0, 1, 2
FLT_MAX = np.finfo(np.float32).max

FWD_S2_2, FWD_S2_3, FWD_ANY = "maxpool_fwd_s2_kernel<2>", "maxpool_fwd_s2_kernel<3>", "maxpool_fwd_kernel"
PAIR, K3S2, VEC4, SCALAR = ("maxpool_bwd_vec4_k3s2_pair_kernel", "maxpool_bwd_vec4_k3s2_kernel", "maxpool_bwd_vec4_kernel",
                            "maxpool_bwd_kernel")

# (n, c, h, w, k, s, padding), forward kernel, backward kernel
CASES = [
    # the vectorised gather for any window (LeNet's and YOLOv3-tiny's 2x2 pools)
    ((3, 5, 36, 40, 2, 2, SAME), FWD_S2_2, VEC4),    # 360 groups of four pixels per plane: two workgroups
    ((2, 3, 13, 16, 2, 1, SAME), FWD_ANY, VEC4),     # YOLOv3-tiny's stride-1 pool on a W % 4 == 0 row
    ((2, 4, 20, 24, 3, 1, SAME), FWD_ANY, VEC4),     # nine windows per pixel
    ((1, 2, 23, 28, 5, 3, VALID), FWD_ANY, VEC4),
    ((1, 3, 20, 24, 2, 3, VALID), FWD_ANY, VEC4),    # stride > size: pixels no window covers
    ((2, 2, 1, 4, 2, 2, SAME), FWD_S2_2, VEC4),      # one group per row, one output row
    # 3x3 / stride 2 with OW == W / 2 (2 == 4 / 2) is the pair kernel's by the dispatcher's rule, on one group per row as well
    ((1, 1, 2, 4, 3, 2, SAME), FWD_S2_3, PAIR),
    # 3x3 / stride 2 with OW * 2 != W: several workgroups per plane, rows that straddle waves
    ((2, 3, 35, 72, 3, 2, VALID), FWD_S2_3, K3S2),   # OW = 35
    # CAFFE padding gives OW = ceil(65 / 2) + 1 = 34 == W / 2 (as for every W % 4 == 0): the pair kernel, 17 groups per row
    ((2, 3, 34, 68, 3, 2, CAFFE), FWD_S2_3, PAIR),
    # W % 4 != 0: one thread per output forward, one thread per source pixel backward
    ((2, 3, 33, 37, 3, 2, SAME), FWD_ANY, SCALAR),
    ((2, 3, 13, 13, 2, 1, SAME), FWD_ANY, SCALAR),
    # plane count: 65536 planes exceed grid.y, and a million inputs turn the scalar gather's grid-stride loop over; 65535 is the
    # largest grid.y of the vectorised kernel
    ((256, 256, 4, 4, 2, 2, SAME), FWD_S2_2, SCALAR),
    ((255, 257, 4, 4, 2, 2, SAME), FWD_S2_2, VEC4),
]
SCATTER_PINS = [(2, 3, 13, 16, 2, 1, SAME), (2, 3, 35, 72, 3, 2, VALID), (2, 3, 33, 37, 3, 2, SAME)]
UNCOVERED = (1, 3, 20, 24, 2, 3, VALID)

# which kernels each tensor takes the layer to when it starts one element past a 16-byte boundary
ALIGN = [
    ((2, 3, 16, 16, 3, 2, SAME), {None: (FWD_S2_3, PAIR), "x": (FWD_ANY, PAIR), "dx": (FWD_S2_3, SCALAR),
                                   "dy": (FWD_S2_3, K3S2), "indexes": (FWD_S2_3, K3S2)}),
    ((2, 3, 12, 16, 2, 2, SAME), {None: (FWD_S2_2, VEC4), "x": (FWD_ANY, VEC4), "dx": (FWD_S2_2, SCALAR),
                                   "dy": (FWD_S2_2, VEC4), "indexes": (FWD_S2_2, VEC4)}),
]

NO_WINNER = [
    ((1, 4, 8, 8, 2, 2, SAME), FWD_S2_2, VEC4),
    ((1, 4, 8, 8, 3, 2, SAME), FWD_S2_3, PAIR),
    ((1, 4, 7, 9, 3, 1, SAME), FWD_ANY, SCALAR),
]


def _id(case):
    shape = case[0] if isinstance(case[0], tuple) else case
    return "n%d_c%d_%dx%d_k%d_s%d_pad%d" % shape


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


def _dev(a, off=0, fill=None):
    """a device tensor of a's shape and type that starts `off` elements into its allocation, holding a (or `fill`)"""
    dt = torch.int32 if a.dtype == np.int32 else torch.float32
    buf = torch.empty(a.size + off, dtype=dt, device=DEV)
    t = buf[off:off + a.size].view(a.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * off
    if fill is None:
        t.copy_(torch.tensor(a))  # a copy: the oracle's cached results are read-only
    else:
        t.fill_(fill)
    return t


def _case(n, c, h, w, k, s, padding):
    rs = np.random.RandomState(h * 1000 + w * 10 + k)
    x = (np.round(rs.uniform(-1, 1, (n, c, h, w)) * 16) / 16).astype(np.float32)  # ties everywhere
    x[:, :, : min(h, 4), 2:6] = 2.0  # a plateau of maxima: the first one wins, and several windows add into it
    oh, ow = ob.maxpool_out_hw(h, w, k, s, padding)
    dy = rs.uniform(-1, 1, (n, c, oh, ow)).astype(np.float32)
    dx0 = rs.uniform(-1, 1, (n, c, h, w)).astype(np.float32)
    return dict(n=n, c=c, h=h, w=w, k=k, s=s, padding=padding, x=x, dx0=dx0, dy=dy)


_ORACLE = {}


def _oracle(cs):
    """orc_maxpool for a case of _case (by shape: computed once): y, indexes, dx onto dx0 and dx onto zeros"""
    key = tuple(cs[q] for q in ("n", "c", "h", "w", "k", "s", "padding"))
    if key not in _ORACLE:
        exp = ob.orc_maxpool(cs, cs["dy"])
        exp["dx_from_zero"] = ob.orc_maxpool(dict(cs, dx0=np.zeros_like(cs["dx0"])), cs["dy"])["dx"]
        for v in exp.values():
            v.setflags(write=False)
        _ORACLE[key] = exp
    return _ORACLE[key]


def _scatter(dy, indexes, dx0):
    """dx0 with dx[indexes[o]] += dy[o] in ascending o, in float32, for the o that have a winner (index >= 0)"""
    dx = dx0.copy().reshape(-1)
    assert dx.dtype == np.float32 and dy.dtype == np.float32
    idx, g = indexes.reshape(-1), dy.reshape(-1)
    np.add.at(dx, idx[idx >= 0], g[idx >= 0])
    return dx.reshape(dx0.shape)


def _run(cs, shifted=None):
    """forward, backward accumulating onto dx0, backward overwriting 7.0; `shifted`: the one tensor that starts an element late"""
    from bcnn_amd import ops
    k, s = cs["k"], cs["s"]
    oh, ow = ob.maxpool_out_hw(cs["h"], cs["w"], k, s, cs["padding"])
    off = lambda name: 1 if shifted == name else 0
    x = _dev(cs["x"], off("x"))
    y = _dev(np.empty((cs["n"], cs["c"], oh, ow), np.float32), 0, fill=5.0)
    idx = _dev(np.empty((cs["n"], cs["c"], oh, ow), np.int32), off("indexes"), fill=-7)
    _trace_start()
    ops.maxpool_forward(x, y, idx, k, s)
    t_fwd = _trace_stop()
    dy = _dev(cs["dy"], off("dy"))
    dx = _dev(cs["dx0"], off("dx"))
    _trace_start()
    ops.maxpool_backward(dy, idx, dx, k, s)
    t_bwd = _trace_stop()
    dxo = _dev(cs["dx0"], off("dx"), fill=7.0)
    _trace_start()
    ops.maxpool_backward(dy, idx, dxo, k, s, overwrite=True)
    t_ovw = _trace_stop()
    torch.cuda.synchronize()
    return dict(y=_np(y), indexes=_np(idx), dx=_np(dx), dx_from_zero=_np(dxo), trace=(t_fwd, t_bwd, t_ovw))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _check(got, exp, fwd, bwd):
    assert got["trace"] == ([fwd], [bwd], [bwd + ":overwrite"]), got["trace"]
    assert np.array_equal(got["y"], exp["y"])
    assert np.array_equal(got["indexes"], exp["indexes"])
    assert np.array_equal(got["dx"], exp["dx"])
    assert np.array_equal(got["dx_from_zero"], exp["dx_from_zero"])


@gpu
@pytest.mark.parametrize("shape,fwd,bwd", CASES, ids=[_id(c) for c in CASES])
def test_maxpool_branches_against_the_oracle(shape, fwd, bwd):
    cs = _case(*shape)
    got = _run(cs)
    _check(got, _oracle(cs), fwd, bwd)
    if shape == UNCOVERED:  # rows and columns 2, 5, 8, .. and column 23 lie between the windows
        free = np.ones((cs["h"], cs["w"]), bool)
        for i in range(got["y"].shape[2]):
            for j in range(got["y"].shape[3]):
                free[3 * i:3 * i + 2, 3 * j:3 * j + 2] = False
        assert free.sum() == 20 * 24 - 7 * 8 * 4
        assert _same_bits(got["dx"][..., free], cs["dx0"][..., free])
        assert (got["dx_from_zero"][..., free] == 0).all()


@gpu
@pytest.mark.parametrize("shape,kernels", ALIGN, ids=[_id(c) for c in ALIGN])
def test_maxpool_tensors_off_the_16_byte_boundary_change_the_kernel_not_the_bits(shape, kernels):
    cs = _case(*shape)
    exp = _oracle(cs)
    aligned = _run(cs)
    _check(aligned, exp, *kernels[None])
    for name in ("x", "dx", "dy", "indexes"):
        got = _run(cs, shifted=name)
        _check(got, exp, *kernels[name])
        for key in ("y", "indexes", "dx", "dx_from_zero"):
            assert _same_bits(got[key], aligned[key]), (name, key)


@gpu
@pytest.mark.parametrize("shape,fwd,bwd", NO_WINNER, ids=[_id(c) for c in NO_WINNER])
def test_maxpool_windows_without_a_winner(shape, fwd, bwd):
    """a plane of NaN, one of -Inf and one of -FLT_MAX: nothing is greater than the -FLT_MAX the scan starts from, so
    y = -FLT_MAX and the index stays -1 (orc_maxpool_forward says the same); the backward pass adds nothing for them. The oracle's
    backward would write dx[-1]: the expected dx is _scatter, pinned to the oracle by the CPU test below."""
    cs = _case(*shape)
    cs["x"][0, 0], cs["x"][0, 1], cs["x"][0, 2] = np.nan, -np.inf, -FLT_MAX
    exp = ob.orc_maxpool(cs)
    assert (exp["y"][0, :3] == -FLT_MAX).all() and (exp["indexes"][0, :3] == -1).all() and (exp["indexes"][0, 3] >= 0).all()
    exp["dx"] = _scatter(cs["dy"], exp["indexes"], cs["dx0"])
    exp["dx_from_zero"] = _scatter(cs["dy"], exp["indexes"], np.zeros_like(cs["dx0"]))
    got = _run(cs)
    _check(got, exp, fwd, bwd)
    assert _same_bits(got["dx"][0, :3], cs["dx0"][0, :3]) and (got["dx_from_zero"][0, :3] == 0).all()


@pytest.mark.parametrize("shape", SCATTER_PINS, ids=[_id(c) for c in SCATTER_PINS])
def test_scatter_helper_is_the_oracles_backward(shape):
    """no GPU: _scatter, the expected dx of the cases the oracle's backward cannot take, gives orc_maxpool's bits where both can"""
    cs = _case(*shape)
    exp = _oracle(cs)
    assert (exp["indexes"] >= 0).all()
    assert _same_bits(_scatter(cs["dy"], exp["indexes"], cs["dx0"]), exp["dx"])
    assert _same_bits(_scatter(cs["dy"], exp["indexes"], np.zeros_like(cs["dx0"])), exp["dx_from_zero"])


# ---------------------------------------------------------------------------------------------------
# global average pooling: one wave per plane
# ---------------------------------------------------------------------------------------------------
# HW = 1, 63, 64, 65, 4097 around the 64 lanes of a wave; 9000 planes against the 8192 waves of the capped grid
# (STREAM_GRID_PER_CU = 8 workgroups of four waves on each of 256 CUs): the plane loop turns over
AVG = [(3, 5, 1, 1), (3, 5, 7, 9), (3, 5, 8, 8), (3, 5, 5, 13), (3, 5, 17, 241), (100, 90, 3, 3)]


def _avg_case(n, c, h, w):
    rs = np.random.RandomState(h * 1000 + w)
    return dict(n=n, c=c, h=h, w=w, x=rs.uniform(-1, 1, (n, c, h, w)).astype(np.float32),
                dy=rs.uniform(-1, 1, (n, c, 1, 1)).astype(np.float32), dx0=rs.uniform(-1, 1, (n, c, h, w)).astype(np.float32))


def _avg_forward_within_bound(y, cs):
    """the kernel adds ceil(HW / 64) values per lane, combines the lanes in six shuffle steps and divides once: every input goes
    through at most ceil(HW / 64) + 7 roundings of 2^-24 relative each, so |y - mean| <= (ceil(HW / 64) + 7) 2^-24 mean(|x|)"""
    hw = cs["h"] * cs["w"]
    x64 = cs["x"].astype(np.float64).reshape(cs["n"], cs["c"], hw)
    bound = ((hw + 63) // 64 + 7) * 2.0 ** -24 * np.abs(x64).mean(axis=2)
    err = np.abs(y.astype(np.float64).reshape(cs["n"], cs["c"]) - x64.mean(axis=2))
    return bool((err <= bound).all()), float((err / np.maximum(bound, 1e-300)).max())


@gpu
@pytest.mark.parametrize("shape", AVG, ids=["n%d_c%d_%dx%d" % s for s in AVG])
def test_avgpool_against_the_oracle(shape):
    from bcnn_amd import ops
    cs = _avg_case(*shape)
    exp = ob.orc_avgpool(cs)
    y = _dev(exp["y"], fill=5.0)
    _trace_start()
    ops.avgpool_forward(_dev(cs["x"]), y)
    assert _trace_stop() == ["avgpool_fwd_kernel"]
    dx = _dev(cs["dx0"])
    _trace_start()
    ops.avgpool_backward(_dev(cs["dy"]), dx)
    assert _trace_stop() == ["avgpool_bwd_kernel"]
    torch.cuda.synchronize()
    ok, worst = _avg_forward_within_bound(_np(y), cs)
    assert ok, worst
    assert np.array_equal(_np(dx), exp["dx"])  # dx += dy / HW element by element: the oracle's bits


@pytest.mark.parametrize("shape", AVG, ids=["n%d_c%d_%dx%d" % s for s in AVG])
def test_avgpool_bound_holds_for_the_oracle_too(shape):
    """no GPU: the oracle adds the HW values of a plane one after the other, a deeper sum than the kernel's, and still stays inside
    the kernel's bound on these inputs -- the bound does not single out one summation order"""
    cs = _avg_case(*shape)
    ok, worst = _avg_forward_within_bound(ob.orc_avgpool(cs)["y"], cs)
    assert ok, worst
