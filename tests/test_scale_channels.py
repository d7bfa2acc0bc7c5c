"""The scale-channels kernels (bcnn_amd/csrc/scale_channels.hip) through bcnn_amd.ops.

Forward and the source gradient are one multiply (and one add) per element, not contracted by the build: held to numpy float32
bit for bit, the gradient starting from a non-zero dx0. The gate gradient of the per-plane form is a sum over the plane:
    |got - ref| <= HW 2^-23 sum_hw |dy x|    per plane, ref in float64,
the bound every summation order of the float32 products satisfies; two runs give the same bits, and a start value dg0 enters
as one float32 addition (dg0 + the sum a zero start gives). The same-shape gate has the exact bits of dg0 + dy x. With dx or
dgate absent the other half is unchanged bitwise. The shapes cover every kernel: one lane group per plane from 1 lane (1 x 1)
to a wave (7 x 7, 14 x 14), the sliced planes (112 x 112), many tiny planes, plane starts that are odd for 16-byte vectors
(49 values per plane) and an unaligned base."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SHAPES = [(1, 1, 1, 1), (2, 3, 1, 1), (2, 5, 3, 3), (3, 16, 7, 7), (2, 8, 14, 14), (1, 2, 112, 112), (4, 130, 2, 2),
          (2, 3, 40, 40), (1, 3, 33, 35)]
CASES = [(s, same, 0) for s in SHAPES for same in (0, 1)] + [((3, 16, 7, 7), 0, 1), ((3, 16, 7, 7), 1, 1),
                                                              ((1, 2, 112, 112), 0, 1)]


def _dev(a, offset=0):
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
    return view.view(a.shape)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


def _case(shape, same, seed=0):
    n, c, h, w = shape
    rs = np.random.RandomState(n * 1000 + c * 100 + h + seed)
    x = rs.uniform(-2, 2, shape).astype(F32)
    g = rs.uniform(-1.5, 1.5, shape if same else (n, c, 1, 1)).astype(F32)
    dy = rs.uniform(-1, 1, shape).astype(F32)
    dx0 = rs.uniform(-1, 1, shape).astype(F32)
    dg0 = rs.uniform(-1, 1, g.shape).astype(F32)
    return x, g, dy, dx0, dg0


def _trace(on):
    from bcnn_amd import _lib
    L = _lib.load()
    if on:
        L.bcnn_hip_trace_enable(1)
        return None
    n = L.bcnn_hip_trace_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return buf.value.decode().split()


def _backward(x, g, dy, dx0, dg0, offset):
    from bcnn_amd import ops
    tx, tg, tdy = _dev(x, offset), _dev(g, offset), _dev(dy, offset)
    tdx = None if dx0 is None else _dev(dx0, offset)
    tdg = None if dg0 is None else _dev(dg0, offset)
    ops.scale_channels_backward(tx, tg, tdy, tdx, tdg)
    torch.cuda.synchronize()
    return (None if tdx is None else tdx.cpu().numpy()), (None if tdg is None else tdg.cpu().numpy())


@pytest.mark.parametrize("shape,same,offset", CASES)
def test_forward_and_backward(shape, same, offset):
    from bcnn_amd import ops
    x, g, dy, dx0, dg0 = _case(shape, same)
    n, c, h, w = shape
    tx, tg, ty = _dev(x, offset), _dev(g, offset), _dev(np.full(shape, 3.0, F32), offset)
    ops.scale_channels_forward(tx, tg, ty)
    assert np.array_equal(_bits(ty.cpu().numpy()), _bits(x * g)), "forward"
    assert np.array_equal(_bits(tx.cpu().numpy()), _bits(x)) and np.array_equal(_bits(tg.cpu().numpy()), _bits(g))

    _trace(True)
    dx, dg = _backward(x, g, dy, dx0, dg0, offset)
    ran = _trace(False)
    assert len(ran) == 1 and ran[0].startswith("scale_channels_bwd"), ran   # ONE sweep
    if not same or h * w == 1:
        want = "scale_channels_bwd:split" if h * w > 1024 else "scale_channels_bwd:small"
        assert ran == [want], ran
    assert np.array_equal(_bits(dx), _bits(dx0 + dy * g)), "dx = dx0 + dy * g"
    if same and h * w > 1:
        assert np.array_equal(_bits(dg), _bits(dg0 + dy * x)), "same-shape gate: dg0 + dy * x"
    else:
        # from a zero start: the summation bound against float64
        _, dg_z = _backward(x, g, dy, dx0, np.zeros_like(dg0), offset)
        prod = dy.astype(np.float64) * x.astype(np.float64)
        ref = prod.sum(axis=(2, 3)).reshape(dg0.shape)
        bound = h * w * 2.0 ** -23 * np.abs(prod).sum(axis=(2, 3)).reshape(dg0.shape)
        err = np.abs(dg_z.astype(np.float64) - ref)
        assert (err <= bound).all(), "plane sums: worst err / bound %.3g" % float((err / np.maximum(bound, 1e-300)).max())
        # a start value enters as one float32 addition
        assert np.array_equal(_bits(dg), _bits(dg0 + dg_z)), "dgate accumulates"
    # run to run
    dx2, dg2 = _backward(x, g, dy, dx0, dg0, offset)
    assert np.array_equal(_bits(dx2), _bits(dx)) and np.array_equal(_bits(dg2), _bits(dg)), "two runs, same bits"
    # either gradient absent: the other half unchanged
    dx3, none_g = _backward(x, g, dy, dx0, None, offset)
    assert none_g is None and np.array_equal(_bits(dx3), _bits(dx)), "dgate=None leaves dx as it is"
    none_x, dg3 = _backward(x, g, dy, None, dg0, offset)
    assert none_x is None and np.array_equal(_bits(dg3), _bits(dg)), "dx=None leaves dgate as it is"


def test_inputs_are_not_written():
    """the backward reads x, gate and dy only"""
    from bcnn_amd import ops
    x, g, dy, dx0, dg0 = _case((3, 16, 7, 7), 0, seed=5)
    tx, tg, tdy, tdx, tdg = (_dev(a) for a in (x, g, dy, dx0, dg0))
    ops.scale_channels_backward(tx, tg, tdy, tdx, tdg)
    for t, a in ((tx, x), (tg, g), (tdy, dy)):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a))
