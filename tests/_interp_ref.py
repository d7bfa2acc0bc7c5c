"""The bilinear interpolation rule (include/bcnn_hip.h, bcnn_amd/csrc/interp_rule.h) restated in numpy. Not a test.

Per axis, input extent I, output extent O, output index o, everything float32 and every operation rounded on its own:
    align_corners:      s = (I - 1) / (O - 1) if O > 1 else 0;  src = s * o
    not align_corners:  s = I / O;  src = max(s * (o + 0.5) - 0.5, 0)
    i0 = min(int(src), I - 1);  i1 = i0 + (i0 < I - 1);  l1 = clamp(src - i0, 0, 1);  l0 = 1 - l1
    y = h0 * (w0 * x[y0][x0] + w1 * x[y0][x1]) + h1 * (w0 * x[y1][x0] + w1 * x[y1][x1])
numpy rounds every float32 operation on its own, so `forward(..., np.float32)` gives the bits the rule defines.
The backward is the gather the issue describes: per input element, the sum of h * (w * dy) over every (output row, output
column, row tap, column tap) that names it."""
import numpy as np

F32 = np.float32


def axis_taps(size_in, size_out, align_corners):
    """(i0, i1, l0, l1) of one axis: int64 indices and float32 weights"""
    o = np.arange(size_out, dtype=F32)
    if align_corners:
        s = F32(size_in - 1) / F32(size_out - 1) if size_out > 1 else F32(0)
        src = s * o
    else:
        s = F32(size_in) / F32(size_out)
        src = s * (o + F32(0.5)) - F32(0.5)
        src = np.maximum(src, F32(0))
    assert src.dtype == F32
    i0 = np.minimum(src.astype(np.int64), size_in - 1)
    i1 = i0 + (i0 < size_in - 1)
    l1 = np.clip(src - i0.astype(F32), F32(0), F32(1)).astype(F32)
    l0 = F32(1) - l1
    return i0, i1, l0, l1


def forward(x, out_h, out_w, align_corners, dtype=F32):
    """x [n][c][h][w] float32 -> [n][c][out_h][out_w] in `dtype` arithmetic over the float32 taps, the rule's association"""
    y0, y1, h0, h1 = axis_taps(x.shape[2], out_h, align_corners)
    x0, x1, w0, w1 = axis_taps(x.shape[3], out_w, align_corners)
    x = x.astype(dtype)
    h0, h1 = h0.astype(dtype)[:, None], h1.astype(dtype)[:, None]
    w0, w1 = w0.astype(dtype)[None, :], w1.astype(dtype)[None, :]
    top, bot = x[:, :, y0, :], x[:, :, y1, :]
    y = h0 * (w0 * top[..., x0] + w1 * top[..., x1]) + h1 * (w0 * bot[..., x0] + w1 * bot[..., x1])
    assert y.dtype == dtype
    return y


def _axis_matrix(size_in, size_out, align_corners):
    """[2][size_out][size_in] float64: tap t of output o names input i with this weight (0 elsewhere), and the same as a mask"""
    i0, i1, l0, l1 = axis_taps(size_in, size_out, align_corners)
    m = np.zeros((2, size_out, size_in), np.float64)
    hit = np.zeros((2, size_out, size_in), bool)
    o = np.arange(size_out)
    m[0, o, i0], m[1, o, i1] = l0, l1
    hit[0, o, i0] = hit[1, o, i1] = True
    return m, hit


def backward(dy, h, w, align_corners):
    """dy [n][c][out_h][out_w] float32 -> (dx, dabs, count) for an [n][c][h][w] input, evaluated in float64 over the float32
    weights: dx = sum of h * (w * dy) over the contributions of each element, dabs = sum of |h * w * dy|, count [h][w] =
    the number of contributions T (0: no output names the element)"""
    mh, hh = _axis_matrix(h, dy.shape[2], align_corners)
    mw, hw = _axis_matrix(w, dy.shape[3], align_corners)
    # the two taps of one output that name the same element (the far edge) add up exactly in float64
    mh, mw = mh.sum(0), mw.sum(0)                        # [out_h][h], [out_w][w]
    d = dy.astype(np.float64)
    dx = np.matmul(np.matmul(mh.T, d), mw)               # weights are >= 0: the same product bounds the absolute sum
    dabs = np.matmul(np.matmul(mh.T, np.abs(d)), mw)
    count = np.outer(hh.sum((0, 1)), hw.sum((0, 1)))      # (row, tap) pairs naming h times (column, tap) pairs naming w
    return dx, dabs, count


# ---- shared test data: shapes on which every weight is a multiple of 1/16, so that every product and every sum is exact ----
# (h, w), (out_h, out_w), align_corners
DYADIC = [((5, 6), (10, 12), False), ((3, 4), (12, 16), False), ((4, 4), (32, 32), False), ((5, 7), (9, 13), True),
          ((6, 9), (3, 4), False)]


def grid(gen, shape):
    """torch values on a grid of 1/16 in [-1, 1], without negative zeros"""
    import torch
    return torch.round((torch.rand(shape, generator=gen) * 2 - 1) * 16) / 16 + 0.0


def dyadic_case(hw, out, align_corners, n=2, c=3):
    """x, dy, dx0 on the grid and torch's float32 forward and gradient (CPU) for one DYADIC row"""
    import torch
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(hw[0] * 1000 + hw[1] * 10 + out[0])
    x = grid(gen, (n, c) + tuple(hw)).requires_grad_(True)
    y = F.interpolate(x, size=tuple(out), mode="bilinear", align_corners=align_corners)
    dy = grid(gen, y.shape)
    y.backward(dy)
    return dict(x=x.detach(), y=y.detach(), dy=dy, grad=x.grad.clone(), dx0=grid(gen, x.shape))
