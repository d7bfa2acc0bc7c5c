"""The pool2d kernels (bcnn_amd/csrc/pool2d.hip) at operator level against torch's CPU pooling, on every dispatch branch.

Max pooling: inputs, gradients and the starting dx sit on a grid of 1/16 with a plateau above everything else, so ties are
everywhere and every sum is exact: y and the indexes are compared BIT FOR BIT with F.max_pool2d(return_indices=True)
(torch's plane-local index moved to the whole-tensor offset), dx bit for bit with torch's gradient, added onto a random
grid-valued dx and written over a buffer of 7.0.

Average pooling: N(0, 1) data against torch in float64, both values of count_include_pad:
    forward   |y - y64|   <= 1.01 * size^2 * 2^-24 * (sum |x| over the window / divisor)
              (size^2 - 1 roundings of the sum in any order, one of the division),
    backward  |dx - dx64| <= 1.01 * (T + 2) * 2^-24 * (|dx0| + sum |dy| / divisor over the covering windows),
              T = ceil(size / stride)^2, dx0 the starting value (0 in the overwrite form).
Elements no window covers (stride > size) keep their bits in the add form and are 0 in the overwrite form.

Each case asserts the kernels the dispatch trace names: a case that lands on another branch fails."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._pool2d_cases import TABLE

gpu = pytest.mark.gpu
DEV = "cuda:0"

FWD_ANY, BWD_ANY, BWD_V4 = "pool2d_fwd_kernel<%s>", "pool2d_bwd_kernel<%s>", "pool2d_bwd_vec4_kernel<%s>"
FWD_S2, BWD_FIXED = "pool2d_fwd_s2x4_kernel<%s,%d>", "pool2d_bwd_vec4_kernel<%s,%d,2,%d>"
BWD_PAIR = "pool2d_bwd_k3s2p1_pair_kernel<%s>"   # 3 / s2 / p1 with out_w == w / 2


def _kernels(kind, h, w, size, stride, pad, ow, aligned=True, y_aligned=True, dy_aligned=True):
    """the dispatch rule of pool2d.hip restated: (forward, backward) kernel names"""
    s2 = stride == 2 and (size, pad) in ((2, 0), (3, 1))
    if s2 and w % 4 == 0 and aligned:
        fwd = FWD_S2 % (kind, size) + (":v4" if ow % 4 == 0 and y_aligned else "")
    else:
        fwd = FWD_ANY % kind
    if w % 4 == 0 and aligned and s2 and size == 3 and ow * 2 == w and dy_aligned:
        bwd = BWD_PAIR % kind
    elif w % 4 == 0 and aligned:
        bwd = BWD_FIXED % (kind, size, pad) if s2 else BWD_V4 % kind
    else:
        bwd = BWD_ANY % kind
    return fwd, bwd


# (n, c, h, w), kind, size, stride, pad, ceil, (forward kernel, backward kernel) -- the names are written out, not derived
CASES = []
_EXPECT = {  # the table of tests/_pool2d_cases.py with N = 2, C = 3, in its order
    0: (FWD_ANY % "max", BWD_ANY % "max"),
    1: (FWD_S2 % ("max", 3) + ":v4", BWD_PAIR % "max"),
    2: (FWD_ANY % "max", BWD_ANY % "max"),          # 2 / s2 with pad 1 is not the specialised 2 / s2 / p0
    3: (FWD_ANY % "max", BWD_ANY % "max"),
    4: (FWD_ANY % "avg", BWD_ANY % "avg"),
    5: (FWD_S2 % ("avg", 2), BWD_FIXED % ("avg", 2, 0)),   # out_w = 6: scalar stores
    6: (FWD_ANY % "avg", BWD_ANY % "avg"),
    7: (FWD_ANY % "avg", BWD_ANY % "avg"),
    8: (FWD_ANY % "avg", BWD_ANY % "avg"),
    9: (FWD_ANY % "avg", BWD_ANY % "avg"),
    10: (FWD_ANY % "max", BWD_ANY % "max"),
    11: (FWD_ANY % "max", BWD_ANY % "max"),
    12: (FWD_ANY % "max", BWD_ANY % "max"),
    13: (FWD_S2 % ("max", 3) + ":v4", BWD_PAIR % "max"),
    14: (FWD_ANY % "avg", BWD_ANY % "avg"),
}
for _i, (_kind, _h, _w, _k, _s, _p, _ceil, _) in enumerate(TABLE):
    CASES.append(((2, 3, _h, _w), _kind, _k, _s, _p, _ceil, _EXPECT[_i]))
CASES += [
    # 65792 planes: past any grid.y, and the capped grids turn their grid-stride loops over
    ((256, 257, 4, 4), "max", 2, 2, 0, 0, (FWD_S2 % ("max", 2), BWD_FIXED % ("max", 2, 0))),
    ((256, 257, 4, 4), "avg", 2, 2, 0, 0, (FWD_S2 % ("avg", 2), BWD_FIXED % ("avg", 2, 0))),
    # a plane spans more than one workgroup
    ((3, 5, 36, 40), "max", 3, 2, 1, 0, (FWD_S2 % ("max", 3) + ":v4", BWD_PAIR % "max")),
    ((3, 5, 36, 40), "avg", 3, 2, 1, 0, (FWD_S2 % ("avg", 3) + ":v4", BWD_PAIR % "avg")),
    # odd heights under the pair kernel: the last source row has one covering window row, out_h = 18 / 3
    ((2, 3, 35, 8), "max", 3, 2, 1, 0, (FWD_S2 % ("max", 3) + ":v4", BWD_PAIR % "max")),
    ((2, 3, 5, 12), "avg", 3, 2, 1, 0, (FWD_S2 % ("avg", 3), BWD_PAIR % "avg")),
    # the specialised kernels in ceil mode: a last window that hangs over the right / bottom edge, W % 8 == 0 so that a
    # thread's second 16-byte load and (size 3) its first lie past the row; out_w = 9 != w / 2: the gather with fixed geometry
    ((2, 3, 9, 16), "max", 3, 2, 1, 1, (FWD_S2 % ("max", 3), BWD_FIXED % ("max", 3, 1))),      # out 5 x 9
    ((2, 3, 9, 16), "avg", 3, 2, 1, 1, (FWD_S2 % ("avg", 3), BWD_FIXED % ("avg", 3, 1))),
    ((2, 3, 7, 12), "max", 2, 2, 0, 1, (FWD_S2 % ("max", 2), BWD_FIXED % ("max", 2, 0))),      # out 4 x 6
    ((2, 3, 12, 16), "max", 2, 2, 0, 0, (FWD_S2 % ("max", 2) + ":v4", BWD_FIXED % ("max", 2, 0))),
    ((2, 3, 12, 16), "avg", 2, 2, 0, 0, (FWD_S2 % ("avg", 2) + ":v4", BWD_FIXED % ("avg", 2, 0))),
    # the run-time vectorised gather: any window on a W % 4 == 0 row
    ((2, 3, 13, 16), "max", 5, 1, 2, 0, (FWD_ANY % "max", BWD_V4 % "max")),
    ((2, 3, 12, 16), "avg", 3, 1, 1, 0, (FWD_ANY % "avg", BWD_V4 % "avg")),
    ((1, 3, 20, 24), "avg", 2, 3, 0, 0, (FWD_ANY % "avg", BWD_V4 % "avg")),     # stride > size on the vectorised route
    ((1, 3, 20, 24), "max", 2, 3, 0, 0, (FWD_ANY % "max", BWD_V4 % "max")),
    ((1, 2, 23, 28), "max", 5, 3, 1, 1, (FWD_ANY % "max", BWD_V4 % "max")),
]

# tensors that start 4 bytes past a 16-byte boundary: every tensor of the case at once (the scalar routes), and the
# output tensors alone (the specialised forward with scalar stores; backward, the pair kernel wants dy and the indexes
# on 8 bytes, the gather with fixed geometry does not)
ALIGN = [
    ((2, 3, 16, 16), "max", 3, 2, 1, 0, ("x", "y", "dx", "dy", "indexes"), (FWD_ANY % "max", BWD_ANY % "max")),
    ((2, 3, 12, 16), "avg", 2, 2, 0, 0, ("x", "y", "dx", "dy", "indexes"), (FWD_ANY % "avg", BWD_ANY % "avg")),
    ((2, 3, 16, 16), "max", 3, 2, 1, 0, ("y", "dy", "indexes"), (FWD_S2 % ("max", 3), BWD_FIXED % ("max", 3, 1))),
    ((2, 3, 12, 16), "avg", 2, 2, 0, 0, ("y", "dy"), (FWD_S2 % ("avg", 2), BWD_FIXED % ("avg", 2, 0))),
]


def _id(case):
    (n, c, h, w), kind, k, s, p, ceil = case[:6]
    return "%s_n%d_c%d_%dx%d_k%d_s%d_p%d_%s" % (kind, n, c, h, w, k, s, p, "ceil" if ceil else "floor")


def _trace_start():
    from bcnn_amd import _lib
    _lib.load().bcnn_hip_trace_enable(1)


def _trace_stop():
    from bcnn_amd import _lib
    L = _lib.load()
    n = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return buf.value.decode().split()


def _dev(t, off=0, fill=None):
    """a device tensor of t's shape and type that starts `off` elements into its allocation, holding t (or `fill`)"""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    d = buf[off:off + t.numel()].view(t.shape)
    assert d.is_contiguous() and d.data_ptr() % 16 == 4 * off
    if fill is None:
        d.copy_(t)  # a copy: the cached references stay as they are
    else:
        d.fill_(fill)
    return d


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _grid(gen, shape):
    """values on a grid of 1/16 in [-1, 1], without negative zeros (x + 0.0)"""
    return torch.round((torch.rand(shape, generator=gen) * 2 - 1) * 16) / 16 + 0.0


@functools.lru_cache(maxsize=None)
def _max_ref(shape, k, s, p, ceil):
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(h * 1000 + w * 10 + k)
    x = _grid(gen, shape)
    x[:, :, : min(h, 4), 2:6] = 2.0  # a plateau of maxima: the first one wins, and several windows add into it
    xr = x.clone().requires_grad_(True)
    y, idx = F.max_pool2d(xr, k, s, p, ceil_mode=bool(ceil), return_indices=True)
    dy = _grid(gen, y.shape)
    y.backward(dy)
    planes = torch.arange(n * c, dtype=torch.int64).view(n, c, 1, 1) * (h * w)
    dx0 = _grid(gen, shape)
    return dict(x=x, y=y.detach(), indexes=(idx + planes).to(torch.int32), dy=dy, grad=xr.grad.clone(), dx0=dx0)


@functools.lru_cache(maxsize=None)
def _avg_ref(shape, k, s, p, ceil, cip):
    gen = torch.Generator().manual_seed(shape[2] * 1000 + shape[3] * 10 + k)
    x = torch.randn(shape, generator=gen)
    kw = dict(kernel_size=k, stride=s, padding=p, ceil_mode=bool(ceil), count_include_pad=bool(cip))
    x64 = x.double().requires_grad_(True)
    y64 = F.avg_pool2d(x64, **kw)
    dy = torch.randn(y64.shape, generator=gen)
    y64.backward(dy.double())
    grad64 = x64.grad.clone()
    x64.grad = None
    F.avg_pool2d(x64, **kw).backward(dy.double().abs())   # sum |dy| / divisor over the covering windows
    gabs = x64.grad.clone()
    x64.grad = None
    F.avg_pool2d(x64, **kw).backward(torch.ones_like(y64))
    covered = x64.grad > 0
    yabs = F.avg_pool2d(x.double().abs(), **kw)             # sum |x| over the window / divisor
    dx0 = torch.randn(shape, generator=gen)
    return dict(x=x, y64=y64.detach(), yabs=yabs, dy=dy, grad64=grad64, gabs=gabs, covered=covered, dx0=dx0)


def _run(kind, shape, k, s, p, ceil, cip, ref, off=(), kernels=None):
    """forward, backward onto dx0, backward over 7.0; returns (y, indexes, dx_add, dx_over) on the host"""
    from bcnn_amd import ops
    o = lambda name: 1 if name in off else 0
    n, c, h, w = shape
    oh, ow = ops.pool2d_out_hw(kind, h, w, k, s, p, bool(ceil))
    x = _dev(ref["x"], o("x"))
    y = _dev(torch.empty(n, c, oh, ow), o("y"), fill=float("nan"))
    idx = _dev(torch.empty(n, c, oh, ow, dtype=torch.int32), o("indexes"), fill=-7) if kind == "max" else None
    dy = _dev(ref["dy"], o("dy"))
    dx_add = _dev(ref["dx0"], o("dx"))
    dx_over = _dev(ref["dx0"], o("dx"), fill=7.0)
    _trace_start()
    ops.pool2d_forward(x, y, idx, kind, k, s, p, bool(ceil), bool(cip))
    ops.pool2d_backward(dy, idx, dx_add, kind, k, s, p, bool(ceil), bool(cip), overwrite=False)
    ops.pool2d_backward(dy, idx, dx_over, kind, k, s, p, bool(ceil), bool(cip), overwrite=True)
    torch.cuda.synchronize()
    names = _trace_stop()
    if kernels is not None:
        assert names == [kernels[0], kernels[1], kernels[1] + ":overwrite"], names
    return y.cpu(), idx.cpu() if idx is not None else None, dx_add.cpu(), dx_over.cpu()


def _check_max(shape, k, s, p, ceil, kernels, off=()):
    ref = _max_ref(shape, k, s, p, ceil)
    y, idx, dx_add, dx_over = _run("max", shape, k, s, p, ceil, True, ref, off, kernels)
    assert torch.equal(_bits(y), _bits(ref["y"]))
    assert torch.equal(idx, ref["indexes"])
    assert torch.equal(_bits(dx_add), _bits(ref["dx0"] + ref["grad"]))   # grid values: the sum is exact in any order
    assert torch.equal(_bits(dx_over), _bits(ref["grad"]))


def _check_avg(shape, k, s, p, ceil, kernels, off=()):
    eps = 2.0 ** -24
    T = math.ceil(k / s) ** 2
    for cip in (True, False):
        ref = _avg_ref(shape, k, s, p, ceil, cip)
        y, _, dx_add, dx_over = _run("avg", shape, k, s, p, ceil, cip, ref, off, kernels)
        err = (y.double() - ref["y64"]).abs()
        bound = 1.01 * k * k * eps * ref["yabs"]
        print("avg fwd cip=%d: max err %.3e, max err / bound %.3f" % (cip, err.max().item(), (err / bound.clamp_min(1e-300)).max().item()))
        assert bool((err <= bound).all())
        for dx, dx0 in ((dx_add, ref["dx0"].double()), (dx_over, torch.zeros(shape, dtype=torch.float64))):
            err = (dx.double() - (dx0 + ref["grad64"])).abs()
            bound = 1.01 * (T + 2) * eps * (dx0.abs() + ref["gabs"])
            print("avg bwd cip=%d: max err %.3e" % (cip, err.max().item()))
            assert bool((err <= bound).all())
        un = ~ref["covered"]
        assert torch.equal(_bits(dx_add)[un], _bits(ref["dx0"])[un])   # untouched, bit for bit
        assert bool((_bits(dx_over)[un] == 0).all())                   # +0.0
        if s > k:
            assert bool(un.any())


@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_pool2d_matches_torch(case):
    shape, kind, k, s, p, ceil, kernels = case
    from bcnn_amd import ops
    ow = ops.pool2d_out_hw(kind, shape[2], shape[3], k, s, p, bool(ceil))[1]
    assert kernels == _kernels(kind, shape[2], shape[3], k, s, p, ow)   # the written-out names follow the documented rule
    (_check_max if kind == "max" else _check_avg)(shape, k, s, p, ceil, kernels)


@gpu
@pytest.mark.parametrize("case", ALIGN, ids=lambda c: _id(c) + "_off_" + "_".join(c[6]))
def test_pool2d_unaligned_tensors(case):
    shape, kind, k, s, p, ceil, off, kernels = case
    (_check_max if kind == "max" else _check_avg)(shape, k, s, p, ceil, kernels, off)


@gpu
def test_pool2d_without_indexes_and_determinism():
    """indexes = NULL (PREDICT) gives the same y; two runs of one case give identical bits"""
    from bcnn_amd import ops
    for shape, k, s, p in (((3, 5, 36, 40), 3, 2, 1), ((2, 3, 13, 13), 5, 1, 2)):
        ref = _max_ref(shape, k, s, p, 0)
        y1, idx1, add1, over1 = _run("max", shape, k, s, p, 0, True, ref)
        y2, idx2, add2, over2 = _run("max", shape, k, s, p, 0, True, ref)
        for a, b in ((y1, y2), (add1, add2), (over1, over2)):
            assert torch.equal(_bits(a), _bits(b))
        assert torch.equal(idx1, idx2)
        y = torch.full(y1.shape, float("nan"), device=DEV)
        ops.pool2d_forward(ref["x"].to(DEV), y, None, "max", k, s, p)
        assert torch.equal(_bits(y), _bits(y1))
    shape = (3, 5, 36, 40)
    ref = _avg_ref(shape, 3, 2, 1, 0, True)
    r1 = _run("avg", shape, 3, 2, 1, 0, True, ref)
    r2 = _run("avg", shape, 3, 2, 1, 0, True, ref)
    for a, b in ((r1[0], r2[0]), (r1[2], r2[2]), (r1[3], r2[3])):
        assert torch.equal(_bits(a), _bits(b))
