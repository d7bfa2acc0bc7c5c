"""ops.attention_forward / ops.attention_backward (attention.hip) against a float64 numpy evaluation of
    S = scale Q^T K, P = softmax_j S, O = V P^T;  Dl = sum_r dO O, dP = dO^T V, dS = P (dP - Dl), dV = dO P, dQ = scale K dS^T,
    dK = scale Q dS
per image and head. Every tensor is within 1e-5 max|reference| (the plain float32 evaluation of the same formulas sits at
8.4e-7 on these shapes; the factor covers another summation order and the hardware exponential). The shapes cross every tile
edge: one key, one query, one key past a tile, ragged on both axes, the 128-channel limit. The other checks compare bits."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
# (N, heads, d, c, Lq, Lk)
SHAPES = [(1, 1, 1, 1, 1, 1), (2, 2, 3, 5, 31, 1), (1, 2, 8, 8, 64, 65), (2, 1, 20, 12, 65, 129), (1, 3, 32, 32, 196, 196),
          (1, 1, 128, 128, 129, 257), (2, 4, 16, 24, 257, 31), (1, 1, 64, 64, 1, 203)]
OVERFLOW = (1, 2, 32, 16, 65, 129)
CHECKS = ["float64", "rerun", "accumulate", "null", "misaligned", "lse_null"]
# one tensor for q, k and v, one buffer for the three gradients: where d == c and Lq == Lk
CASES = [(s, c) for s in SHAPES + [OVERFLOW + ("overflow",)] for c in CHECKS] + \
        [(s, "aliased") for s in SHAPES if s[2] == s[3] and s[4] == s[5]]


def reference(q, k, v, do, scale):
    """the formulas of the module's docstring on float64 [N][heads][channels][L] arrays; also the largest score"""
    s = scale * np.einsum("nhti,nhtj->nhij", q, k)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = np.einsum("nhrj,nhij->nhri", v, p)
    ds = p * (np.einsum("nhri,nhrj->nhij", do, v) - np.einsum("nhri,nhri->nhi", do, o)[..., None])
    return dict(o=o, dq=scale * np.einsum("nhtj,nhij->nhti", k, ds), dk=scale * np.einsum("nhti,nhij->nhtj", q, ds),
                dv=np.einsum("nhri,nhij->nhrj", do, p)), s.max()


@functools.lru_cache(maxsize=None)
def _case(shape, overflow=False):
    """inputs (float32 values) and the float64 reference of one shape, made once"""
    n, heads, d, c, lq, lk = shape
    rs = np.random.RandomState(sum(shape) + 7 * d)
    draw = (lambda s: rs.randint(-4, 5, s).astype(np.float64)) if overflow else rs.standard_normal
    q, k = draw((n, heads, d, lq)), draw((n, heads, d, lk))
    v, do = rs.standard_normal((n, heads, c, lk)), rs.standard_normal((n, heads, c, lq))
    q, k, v, do = [a.astype(np.float32).astype(np.float64) for a in (q, k, v, do)]
    ref, smax = reference(q, k, v, do, 1.0 if overflow else 1.0 / np.sqrt(d))
    return dict(q=q, k=k, v=v, do=do), ref, smax


def _dev(a, off):
    """a on the device as [N][C][1][L] float32, `off` floats past an allocation's (16-byte aligned) start"""
    n, heads, ch, length = a.shape
    buf = torch.empty(a.size + off, dtype=torch.float32, device=DEV)
    buf[off:] = torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel())
    return buf[off:].view(n, heads * ch, 1, length)


def _run(shape, overflow=False, start=None, null=(), off=0, lse=True, aliased=False):
    """forward and backward through ops; start: the gradients' start values (they accumulate), else they are assigned;
    aliased: q is k and v too, and the three gradients add up in one zero-filled buffer (returned as dq)"""
    from bcnn_amd import ops
    heads = shape[1]
    x, ref, _ = _case(shape, overflow)
    scale = 1.0 if overflow else 0.0
    t = {name: _dev(a, off) for name, a in x.items()}
    if aliased:
        t["k"] = t["v"] = t["q"]
    o = _dev(np.zeros_like(ref["o"]), off)
    tl = torch.zeros(shape[0] * heads * shape[4], dtype=torch.float32, device=DEV)
    ops.attention_forward(t["q"], t["k"], t["v"], o, tl if lse else None, heads, scale)
    out = {"o": o}
    if lse:
        g = {name: None if name in null else _dev(np.full_like(ref[name], 7.0) if start is None else start[name], off)
             for name in ("dq", "dk", "dv")}
        if aliased:
            g["dq"].zero_()
            g["dk"] = g["dv"] = g["dq"]
        ops.attention_backward(t["q"], t["k"], t["v"], o, tl, t["do"], g["dq"], g["dk"], g["dv"], heads, scale,
                               overwrite=(start is None and not aliased,) * 3)
        out.update({name: a for name, a in g.items() if a is not None})
    torch.cuda.synchronize()
    return {name: a.cpu().numpy().reshape(ref[name].shape) for name, a in out.items()}


@functools.lru_cache(maxsize=None)
def _base(shape, overflow):
    """the plain run of a shape (gradients assigned over a fill of 7), made once and left unchanged"""
    return _run(shape, overflow)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_bits(a, b, names):
    for name in names:
        assert np.array_equal(_bits(a[name]), _bits(b[name])), name


def _close(got, ref, names):
    for name in names:
        err, bar = np.abs(got[name] - ref[name]).max(), TOL * np.abs(ref[name]).max()
        print("%s: max error %.3g, bar %.3g" % (name, err, bar))
        assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("shape,check", CASES, ids=str)
def test_attention(shape, check):
    overflow, shape = len(shape) == 7, shape[:6]
    x, ref, smax = _case(shape, overflow)
    base = _base(shape, overflow)
    grads = ("dq", "dk", "dv")
    if check == "float64":
        if overflow:   # a condition on the inputs: exp without the maximum subtracted overflows float32 here
            assert smax > 89
        _close(base, ref, ("o",) + grads)
    elif check == "rerun":
        _same_bits(_run(shape, overflow), base, ("o",) + grads)
    elif check == "accumulate":
        rs = np.random.RandomState(5)
        start = {name: rs.standard_normal(ref[name].shape).astype(np.float32) for name in grads}
        got = _run(shape, overflow, start=start)
        _same_bits(got, {name: start[name] + base[name].astype(np.float32) for name in grads}, grads)
    elif check == "null":
        for name in grads:
            _same_bits(_run(shape, overflow, null=(name,)), base, [g for g in grads if g != name])
    elif check == "misaligned":
        _same_bits(_run(shape, overflow, off=1), base, ("o",) + grads)
    elif check == "lse_null":
        _same_bits(_run(shape, overflow, lse=False), base, ("o",))
    else:   # aliased: the buffer holds the float64 sum of the three gradients of attention(x, x, x)
        want, _ = reference(x["q"], x["q"], x["q"], x["do"], 1.0 / np.sqrt(shape[2]))
        _close({"dx": _run(shape, aliased=True)["dq"]}, {"dx": want["dq"] + want["dk"] + want["dv"]}, ("dx",))
