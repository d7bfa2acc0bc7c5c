"""The bilinear interpolation kernels (bcnn_amd/csrc/interp.hip) at operator level, on every dispatch branch.

Forward: N(0, 1) data into a buffer of 7.0, BIT FOR BIT against the float32 restatement of the rule (tests/_interp_ref.py,
pinned to torch by tests/test_interp_ref_pinning.py).
Backward, dyadic shapes (every weight a multiple of 1/16, data on a grid of 1/16: every sum exact): bit for bit against
torch's CPU gradient, added onto a grid-valued dx and written over a buffer of 7.0; the forward likewise against torch.
Backward, general ratios, against the restatement evaluated in float64 over the same float32 weights:
    |dx - dx64| <= 1.01 * (T + 3) * 2^-24 * (|dx0| + sum |h * w * dy|),  T = the number of contributions to the element
    (two roundings per product h * (w * dy) and one per addition; derived, not measured).
Elements no output names (downsampling) keep their bits in the add form and are +0.0 in the overwrite form; a second run
gives the same bits.

Each case asserts the kernels the dispatch trace names, written out per case: a case on another branch fails."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _interp_ref as R

gpu = pytest.mark.gpu
DEV = "cuda:0"

TABLES = "interp_tables_kernel"   # the prologue of every call
FWD, FWD_V4, BWD = "interp_fwd_kernel", "interp_fwd_kernel:v4", "interp_bwd_kernel"

# (n, c, h, w), (out_h, out_w), the values of align_corners, the forward kernel
CASES = [
    ((2, 3, 5, 7), (10, 14), (False, True), FWD),            # baseline x2; out_w = 14: scalar stores
    ((2, 3, 5, 7), (13, 9), (False, True), FWD),             # up along h, barely up along w
    ((2, 3, 9, 12), (4, 5), (False, True), FWD),             # down: elements no output names
    ((2, 3, 1, 1), (4, 4), (False, True), FWD_V4),           # i1 == i0 everywhere
    ((2, 3, 4, 6), (1, 1), (False, True), FWD),              # O = 1 under align_corners
    ((2, 3, 6, 6), (6, 6), (False, True), FWD),              # identity: an exact copy
    ((2, 3, 9, 9), (65, 65), (True,), FWD),                  # zoom 8
    ((3, 5, 36, 40), (72, 80), (False, True), FWD_V4),       # a plane spans more than one workgroup
    # 65 792 planes, more than any grid.y. The grids are capped at 2048 workgroups = 524 288 threads (stream_grid): this
    # case has 263 168 forward items and as many dx elements, one pass each. The two cases below pass the cap, so the
    # grid-stride step and the index divisions on dividends past the first pass run under these assertions
    ((256, 257, 2, 2), (4, 4), (False, True), FWD_V4),
    ((256, 257, 2, 2), (8, 8), (False, True), FWD_V4),       # 1 052 672 forward items: the forward loop turns over twice
    ((256, 257, 3, 3), (6, 6), (False, True), FWD),          # 592 128 dx elements and 789 504 forward items (scalar stores)
    ((1, 2, 2, 1100), (3, 2200), (False, True), FWD_V4),     # a row wider than a workgroup: the column table is per call
    ((2, 3, 5, 8), (10, 16), (False, True), FWD_V4),         # out_w % 4 == 0
    ((2, 3, 5, 8), (10, 18), (False, True), FWD),            # out_w % 4 != 0
    ((2, 3, 7, 5), (3, 2), (False, True), FWD),              # down on both axes, one four-column item per row
]
# tensors that start 4 bytes past a 16-byte boundary
ALIGN = [
    ((2, 3, 5, 7), (10, 14), ("y", "dy", "dx"), FWD),
    ((2, 3, 5, 8), (10, 16), ("y", "dy", "dx"), FWD),        # out_w % 4 == 0, but y is not on 16 bytes: scalar stores
    ((2, 3, 5, 8), (10, 16), ("x",), FWD_V4),                # only y's alignment matters to the stores
]


def _id(case):
    (n, c, h, w), (oh, ow) = case[:2]
    return "n%d_c%d_%dx%d_to_%dx%d" % (n, c, h, w, oh, ow)


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
    """a device tensor of t's shape that starts `off` elements into its allocation, holding t (or `fill`)"""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    d = buf[off:off + t.numel()].view(t.shape)
    assert d.is_contiguous() and d.data_ptr() % 16 == 4 * off
    if fill is None:
        d.copy_(t)  # a copy: the cached references stay as they are
    else:
        d.fill_(fill)
    return d


def _bits(t):
    t = torch.as_tensor(t)
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _general_ref(shape, out, align_corners):
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(h * 1000 + w * 10 + out[0] + int(align_corners))
    x = torch.randn(shape, generator=gen)
    dy = torch.randn((n, c) + out, generator=gen)
    dx0 = torch.randn(shape, generator=gen)
    y = torch.from_numpy(R.forward(x.numpy(), out[0], out[1], align_corners))
    dx64, dabs, count = R.backward(dy.numpy(), h, w, align_corners)
    return dict(x=x, dy=dy, dx0=dx0, y=y, dx64=torch.from_numpy(dx64), dabs=torch.from_numpy(dabs),
                count=torch.from_numpy(count))


def _run(ref, out, align_corners, fwd_kernel, off=()):
    """forward into 7.0, backward onto dx0, backward over 7.0; returns (y, dx_add, dx_over) on the host"""
    from bcnn_amd import ops
    o = lambda name: 1 if name in off else 0
    n, c = ref["x"].shape[:2]
    x = _dev(ref["x"], o("x"))
    y = _dev(torch.empty((n, c) + tuple(out)), o("y"), fill=7.0)
    dy = _dev(ref["dy"], o("dy"))
    dx_add = _dev(ref["dx0"], o("dx"))
    dx_over = _dev(ref["dx0"], o("dx"), fill=7.0)
    _trace_start()
    ops.interp_forward(x, y, align_corners)
    ops.interp_backward(dy, dx_add, align_corners, overwrite=False)
    ops.interp_backward(dy, dx_over, align_corners, overwrite=True)
    torch.cuda.synchronize()
    names = _trace_stop()
    assert names == [TABLES, fwd_kernel, TABLES, BWD, TABLES, BWD + ":overwrite"], names
    return y.cpu(), dx_add.cpu(), dx_over.cpu()


def _check_general(shape, out, align_corners, fwd_kernel, off=()):
    ref = _general_ref(shape, out, align_corners)
    y, dx_add, dx_over = _run(ref, out, align_corners, fwd_kernel, off)
    assert torch.equal(_bits(y), _bits(ref["y"]))
    if tuple(shape[2:]) == tuple(out):
        assert torch.equal(_bits(y), _bits(ref["x"]))   # the identity is an exact copy
    eps = 2.0 ** -24
    T = ref["count"].double()
    for dx, dx0 in ((dx_add, ref["dx0"].double()), (dx_over, torch.zeros(shape, dtype=torch.float64))):
        err = (dx.double() - (dx0 + ref["dx64"])).abs()
        bound = 1.01 * (T + 3) * eps * (dx0.abs() + ref["dabs"])
        print("bwd: max err %.3e, max err / bound %.3f" % (err.max().item(), (err / bound.clamp_min(1e-300)).max().item()))
        assert bool((err <= bound).all())
    un = (ref["count"] == 0).expand(shape)
    assert torch.equal(_bits(dx_add)[un], _bits(ref["dx0"])[un])   # untouched, bit for bit
    assert bool((_bits(dx_over)[un] == 0).all())                   # +0.0
    if out[0] * 2 < shape[2] or out[1] * 2 < shape[3]:   # fewer taps than elements on an axis
        assert bool(un.any())
    y2, add2, over2 = _run(ref, out, align_corners, fwd_kernel, off)   # the same bits on every run
    for a, b in ((y, y2), (dx_add, add2), (dx_over, over2)):
        assert torch.equal(_bits(a), _bits(b))


@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_interp_matches_the_rule(case):
    shape, out, corners, fwd_kernel = case
    for align_corners in corners:
        _check_general(shape, out, align_corners, fwd_kernel)


@gpu
@pytest.mark.parametrize("case", ALIGN, ids=lambda c: _id(c) + "_off_" + "_".join(c[2]))
def test_interp_unaligned_tensors(case):
    shape, out, off, fwd_kernel = case
    for align_corners in (False, True):
        _check_general(shape, out, align_corners, fwd_kernel, off)


DYADIC_FWD = [FWD_V4, FWD_V4, FWD_V4, FWD, FWD_V4]   # the rows of R.DYADIC: out_w = 12, 16, 32, 13, 4


@gpu
@pytest.mark.parametrize("row", range(len(R.DYADIC)))
def test_interp_dyadic_equals_torch_bit_for_bit(row):
    hw, out, align_corners = R.DYADIC[row]
    ref = R.dyadic_case(hw, out, align_corners)
    y, dx_add, dx_over = _run(ref, out, align_corners, DYADIC_FWD[row])
    assert torch.equal(_bits(y), _bits(ref["y"]))
    assert torch.equal(_bits(dx_add), _bits(ref["dx0"] + ref["grad"]))   # grid values: the sum is exact in any order
    assert torch.equal(_bits(dx_over), _bits(ref["grad"]))
