"""ops.attention_forward_bf16 (attention_bf16.hip) against float64 softmax attention. The inputs are float32 values that are
exact in bf16, so the rounding of q, k and v is exact and the only bf16 rounding left is that of the weights P: at most 2^-9
relative each, and they sum to one, so o moves by at most 2^-9 max|v| (the kernel's l adds the unrounded exponentials); the bar
is 3 * 2^-9 max|v|. lse is an fp32 quantity: 1e-5 absolute. The other checks compare bits. Without a GPU: the entry point is
declared, listed and exported."""
import ctypes
import functools

import numpy as np
import pytest
import torch

DEV = "cuda:0"
# (N, heads, d, c, Lq, Lk)
SHAPES = [(1, 1, 1, 1, 1, 1), (2, 2, 3, 5, 31, 1), (1, 2, 8, 8, 64, 65), (2, 1, 20, 12, 65, 129), (1, 1, 17, 33, 130, 47),
          (1, 3, 32, 32, 196, 196), (1, 1, 128, 128, 129, 257), (1, 1, 64, 64, 1, 203)]
EXACT = (1, 2, 16, 40, 33, 64)


def _bf16_exact(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    n, heads, d, c, lq, lk = shape
    rs = np.random.RandomState(sum(shape))
    return tuple(_bf16_exact(rs.uniform(-2, 2, (n, heads, ch, length))) for ch, length in ((d, lq), (d, lk), (c, lk)))


def _reference(q, k, v):
    """(o, lse) in float64, scale 1 / sqrt(d)"""
    s = np.einsum("nhti,nhtj->nhij", q.astype(np.float64), k.astype(np.float64)) / np.sqrt(q.shape[2])
    m = s.max(-1, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    return np.einsum("nhrj,nhij->nhri", v.astype(np.float64), p / l), (m + np.log(l))[..., 0]


def _dev(a, off):
    """a on the device as [N][C][1][L] float32, `off` floats past an allocation's (16-byte aligned) start"""
    n, heads, ch, length = a.shape
    buf = torch.empty(a.size + off, dtype=torch.float32, device=DEV)
    buf[off:] = torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel())
    return buf[off:].view(n, heads * ch, 1, length)


def _run(q, k, v, off=0, op="attention_forward_bf16"):
    from bcnn_amd import ops
    n, heads, c, lq = q.shape[0], q.shape[1], v.shape[2], q.shape[3]
    o = torch.full((n, heads * c, 1, lq), 7.0, dtype=torch.float32, device=DEV)
    lse = torch.zeros(n * heads * lq, dtype=torch.float32, device=DEV)
    getattr(ops, op)(_dev(q, off), _dev(k, off), _dev(v, off), o, lse, heads)
    torch.cuda.synchronize()
    return o.cpu().numpy().reshape(n, heads, c, lq), lse.cpu().numpy().reshape(n, heads, lq)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,off", [(s, 0) for s in SHAPES] + [((2, 1, 20, 12, 65, 129), 1), ((1, 2, 8, 8, 64, 64), 1)], ids=str)
def test_against_float64(shape, off):
    q, k, v = _inputs(shape)
    o, lse = _run(q, k, v, off)
    ref_o, ref_lse = _reference(q, k, v)
    err, bar = np.abs(o - ref_o).max(), 3 * 2.0 ** -9 * np.abs(v).max()
    err_lse = np.abs(lse - ref_lse).max()
    print("o: max error %.3g, bar %.3g; lse: max error %.3g" % (err, bar, err_lse))
    assert err <= bar, (err, bar)
    assert err_lse <= 1e-5, err_lse


@pytest.mark.gpu
def test_one_key_returns_its_value_column():
    q, k, v = _inputs((2, 2, 3, 5, 31, 1))
    o, _ = _run(q, k, v)
    assert _same_bits(o, np.broadcast_to(v, o.shape))


@pytest.mark.gpu
def test_uniform_weights_over_small_integers_are_exact():
    n, heads, d, c, lq, lk = EXACT
    rs = np.random.RandomState(11)
    q = np.zeros((n, heads, d, lq), np.float32)
    k = _bf16_exact(rs.uniform(-2, 2, (n, heads, d, lk)))
    v = rs.randint(-8, 9, (n, heads, c, lk)).astype(np.float32)
    o, _ = _run(q, k, v)
    want = np.broadcast_to(v.astype(np.float64).sum(-1, keepdims=True) / lk, o.shape).astype(np.float32)
    assert _same_bits(o, want)
    assert _same_bits(o, _run(q, k, v, op="attention_forward")[0])


@pytest.mark.gpu
def test_two_calls_give_the_same_bits():
    q, k, v = _inputs((1, 3, 32, 32, 196, 196))
    (o1, l1), (o2, l2) = _run(q, k, v), _run(q, k, v)
    assert _same_bits(o1, o2) and _same_bits(l1, l2)


def test_the_entry_point_is_declared_listed_and_exported():
    from bcnn_amd import _lib
    name = "bcnn_hip_attention_forward_bf16"
    assert name in _lib.SIGNATURES and name in _lib.declared_symbols()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
