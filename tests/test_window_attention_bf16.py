"""ops.window_attention_forward_bf16 (attention_window_bf16.hip) against a float64 numpy evaluation written here: roll by -shift,
partition into ws x ws windows, S = scale Q^T K + B from the table, pairs of different shift regions excluded, P = softmax S,
O = V P^T, reverse, roll back. q, k and v are uniform(-2, 2) with the low 16 bits cleared, so the kernel's rounding of its inputs
to bf16 is exact; what is left is the rounding of the exponentials (each weight off by at most 2^-9 relative, the weights
summing to one: 2^-9 max|v|) and fp32 terms: the bar is 3 * 2^-9 * max|v|. The other checks compare bits.

Shapes beside those of tests/test_window_attention.py: a window row of 5 windows under a band of 4 (a ragged last band, the
roll's wrap inside a band); W % 4 == 0 with ws 4 in three bands (16-byte loads off the band's start); the d, c <= 64 instance,
band of 2, two bands and a shift that takes the element route; the d <= 32 < c instance, whose band is 3 windows (7 windows:
3 + 3 + 1); the 32 < d instance with 3 windows under its band of 2."""
import ctypes
import functools

import numpy as np
import pytest
import torch

DEV = "cuda:0"
# (N, heads, d, c, H, W, ws, shift, rel_bias)
SHAPES = [(1, 1, 1, 1, 1, 1, 1, 0, 0), (2, 2, 3, 5, 4, 6, 2, 1, 1), (1, 2, 8, 8, 14, 7, 7, 3, 1), (2, 1, 32, 32, 14, 21, 7, 0, 1),
          (1, 3, 16, 24, 16, 8, 8, 4, 1), (1, 2, 33, 31, 10, 5, 5, 2, 1), (1, 1, 64, 64, 8, 8, 8, 0, 0),
          (1, 1, 8, 8, 7, 35, 7, 3, 1), (2, 2, 16, 16, 8, 48, 4, 2, 1), (1, 1, 40, 48, 8, 32, 8, 5, 1),
          (1, 1, 8, 40, 4, 28, 4, 1, 1), (1, 1, 36, 8, 7, 21, 7, 3, 0)]
LARGE_SCORES = (1, 2, 8, 8, 14, 7, 7, 3, 1)
MISALIGNED = [(2, 2, 16, 16, 8, 48, 4, 2, 1), (1, 3, 16, 24, 16, 8, 8, 4, 1)]


def _bf16_exact(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & 0xFFFF0000).view(np.float32)


def _windows(x, ws, shift):
    """[N][heads][ch][H][W] -> [N][heads][windows][ch][L] of the map rolled by -shift"""
    n, heads, ch, h, w = x.shape
    x = np.roll(x, (-shift, -shift), (3, 4)).reshape(n, heads, ch, h // ws, ws, w // ws, ws)
    return x.transpose(0, 1, 3, 5, 2, 4, 6).reshape(n, heads, (h // ws) * (w // ws), ch, ws * ws)


def _reference(q, k, v, table, ws, shift, scale):
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    n, heads, c, h, w = v.shape
    s = scale * np.einsum("nhwti,nhwtj->nhwij", _windows(q, ws, shift), _windows(k, ws, shift))
    if table is not None:
        yy, xx = np.divmod(np.arange(ws * ws), ws)
        rel = (yy[:, None] - yy[None, :] + ws - 1) * (2 * ws - 1) + xx[:, None] - xx[None, :] + ws - 1
        s = s + table.astype(np.float64)[None, :, None][..., rel]
    if shift:
        region = lambda e: np.where(np.arange(e) < e - ws, 0, np.where(np.arange(e) < e - shift, 1, 2))
        code = (3 * region(h)[:, None] + region(w)[None, :]).astype(np.float64)   # in the rolled frame
        code = _windows(code[None, None, None], ws, 0)[0, 0, :, 0]
        s = np.where((code[:, :, None] == code[:, None, :])[None, None], s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    o = np.einsum("nhwrj,nhwij->nhwri", _windows(v, ws, shift), p)
    o = o.reshape(n, heads, h // ws, w // ws, c, ws, ws).transpose(0, 1, 4, 2, 5, 3, 6).reshape(v.shape)
    return np.roll(o, (shift, shift), (3, 4)), np.abs(s[np.isfinite(s)]).max()


@functools.lru_cache(maxsize=None)
def _case(shape, gain=1.0):
    """inputs and the float64 result of one shape, made once and left unchanged"""
    n, heads, d, c, h, w, ws, shift, rel_bias = shape
    rs = np.random.RandomState(sum(shape) + 7 * d)
    q, k, v = (_bf16_exact(rs.uniform(-2, 2, (n, heads, ch, h, w))) for ch in (d, d, c))
    q, k = q * np.float32(gain), k * np.float32(gain)
    table = rs.standard_normal((heads, (2 * ws - 1) ** 2)).astype(np.float32) if rel_bias else None
    return (q, k, v, table) + _reference(q, k, v, table, ws, shift, 1.0 / np.sqrt(d))


def _dev(a, off):
    """a on the device as [N][C][H][W] (a table flat), `off` floats past an allocation's (16-byte aligned) start"""
    buf = torch.empty(a.size + off, dtype=torch.float32, device=DEV)
    buf[off:] = torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel())
    return buf[off:].view(a.shape[0], -1, *a.shape[3:]) if a.ndim == 5 else buf[off:]


def _run(q, k, v, table, ws, shift, off=0, fn="window_attention_forward_bf16"):
    from bcnn_amd import ops
    o = _dev(np.full(v.shape, 7.0, np.float32), off)
    getattr(ops, fn)(_dev(q, off), _dev(k, off), _dev(v, off), None if table is None else _dev(table, off), o, v.shape[1], ws, shift)
    torch.cuda.synchronize()
    return o.cpu().numpy().reshape(v.shape)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,gain", [(s, 1.0) for s in SHAPES] + [(LARGE_SCORES, 8.0)], ids=str)
def test_against_float64(shape, gain):
    q, k, v, table, ref, smax = _case(shape, gain)
    o = _run(q, k, v, table, shape[6], shape[7])
    err, bar = np.abs(o - ref).max(), 3 * 2.0 ** -9 * np.abs(v).max()
    print("o: max error %.3g, bar %.3g, largest score %.3g" % (err, bar, smax))
    assert gain == 1.0 or smax > 100
    assert err <= bar, (err, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MISALIGNED, ids=str)
def test_pointers_off_the_16_byte_grid_give_the_same_bits(shape):
    q, k, v, table = _case(shape)[:4]
    assert _same_bits(_run(q, k, v, table, shape[6], shape[7], off=1), _run(q, k, v, table, shape[6], shape[7]))


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 4])
def test_uniform_weights_over_small_integers_are_exact(shift):
    """q = 0, no table: every weight is 2^-6, or 2^-5 and 2^-4 in the regions of 32 and 16 positions of a shifted border window"""
    rs = np.random.RandomState(11 + shift)
    q = np.zeros((1, 2, 8, 16, 16), np.float32)
    k = _bf16_exact(rs.uniform(-2, 2, q.shape))
    v = rs.randint(-8, 9, (1, 2, 16, 16, 16)).astype(np.float32)
    o = _run(q, k, v, None, 8, shift)
    ref = _reference(q, k, v, None, 8, shift, 1.0)[0]
    assert _same_bits(o, ref) and _same_bits(o, _run(q, k, v, None, 8, shift, fn="window_attention_forward")) and o.any()


@pytest.mark.gpu
def test_a_window_of_one_position_returns_v():
    q, k, v, table = _case((2, 2, 4, 5, 3, 3, 1, 0, 1))[:4]
    assert _same_bits(_run(q, k, v, table, 1, 0), v)


@pytest.mark.gpu
def test_two_calls_give_the_same_bits():
    q, k, v, table = _case((1, 1, 8, 8, 7, 35, 7, 3, 1))[:4]
    assert _same_bits(_run(q, k, v, table, 7, 3), _run(q, k, v, table, 7, 3))


def test_the_entry_point_is_declared_listed_and_exported():
    from bcnn_amd import _lib
    name = "bcnn_hip_window_attention_forward_bf16"
    assert name in _lib.SIGNATURES and name in _lib.declared_symbols()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
