"""ops.window_attention_forward / _backward (attention_window.hip) against a float64 numpy evaluation: roll by -shift,
partition into ws x ws windows, S = scale Q^T K + B with the pairs of different shift regions excluded, P = softmax_j S,
O = V P^T; dS = P (dO^T V - sum_j P dP), dV = dO P, dQ = scale K dS^T, dK = scale Q dS; reverse, roll back; dtable by np.add.at
over the relative index. o, dq, dk, dv are within 1e-5 max|reference| (the bar of tests/test_attention.py for the same
arithmetic). dtable sums over images and windows as well: its bar is the larger of 1e-5 and eight times the worst error of the
same formulas in plain float32 numpy on these shapes, DTABLE_F32_ERR = 7.35e-7 (measured on the CPU, at the overflow shape; relative to max|reference dtable|;
the factor covers another summation order and the hardware exponential), so the bar is 1e-5. The other checks compare bits."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
DTABLE_F32_ERR = 7.35e-7  # worst of reference(..., dtype=np.float32) against float64 over SHAPES and OVERFLOW
DTABLE_TOL = max(TOL, 8 * DTABLE_F32_ERR)
# (N, heads, d, c, H, W, ws, shift, rel_bias)
SHAPES = [(1, 1, 1, 1, 1, 1, 1, 0, 0), (2, 2, 3, 5, 4, 6, 2, 1, 1), (1, 2, 8, 8, 14, 7, 7, 3, 1), (2, 1, 32, 32, 14, 21, 7, 0, 1),
          (1, 3, 16, 24, 16, 8, 8, 4, 1), (1, 2, 33, 31, 10, 5, 5, 2, 1), (1, 1, 64, 64, 8, 8, 8, 0, 0)]
OVERFLOW = (1, 2, 32, 16, 14, 14, 7, 3, 1)
CHECKS = ["float64", "rerun", "accumulate", "null", "misaligned"]
CASES = [(s, c) for s in SHAPES + [OVERFLOW + ("overflow",)] for c in CHECKS]
GRADS = ("dq", "dk", "dv", "dtable")


def _windows(x, ws, shift):
    """[N][heads][ch][H][W] -> [N][heads][windows][ch][L] of the map rolled by -shift"""
    n, heads, ch, h, w = x.shape
    x = np.roll(x, (-shift, -shift), (3, 4)).reshape(n, heads, ch, h // ws, ws, w // ws, ws)
    return x.transpose(0, 1, 3, 5, 2, 4, 6).reshape(n, heads, (h // ws) * (w // ws), ch, ws * ws)


def _map(x, shape, ws, shift):
    """the inverse of _windows"""
    n, heads, ch, h, w = shape
    x = x.reshape(n, heads, h // ws, w // ws, ch, ws, ws).transpose(0, 1, 4, 2, 5, 3, 6).reshape(shape)
    return np.roll(x, (shift, shift), (3, 4))


def _regions(extent, ws, shift):
    return np.where(np.arange(extent) < extent - ws, 0, np.where(np.arange(extent) < extent - shift, 1, 2))


def reference(q, k, v, do, table, ws, shift, scale, dtype=np.float64):
    """the module docstring's formulas in `dtype`; also the largest score"""
    q, k, v, do = (a.astype(dtype) for a in (q, k, v, do))
    h, w = q.shape[3:]
    qw, kw, vw, dow = (_windows(a, ws, shift) for a in (q, k, v, do))
    s = dtype(scale) * np.einsum("nhwti,nhwtj->nhwij", qw, kw)
    yy, xx = np.divmod(np.arange(ws * ws), ws)
    rel = (yy[:, None] - yy[None, :] + ws - 1) * (2 * ws - 1) + xx[:, None] - xx[None, :] + ws - 1
    if table is not None:
        s = s + table.astype(dtype)[None, :, None][..., rel]
    if shift:
        code = (3 * _regions(h, ws, shift)[:, None] + _regions(w, ws, shift)[None, :])[None, None, None].astype(dtype)
        code = _windows(np.broadcast_to(code, (1, 1, 1, h, w)), ws, 0)[0, 0, :, 0]   # [windows][L], already the rolled frame
        s = np.where((code[:, :, None] == code[:, None, :])[None, None], s, -np.inf)
    smax = s[np.isfinite(s)].max()
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    ds = p * np.einsum("nhwri,nhwrj->nhwij", dow, vw)
    ds = ds - p * (ds.sum(-1, keepdims=True))
    out = dict(o=_map(np.einsum("nhwrj,nhwij->nhwri", vw, p), v.shape, ws, shift),
               dq=_map(dtype(scale) * np.einsum("nhwtj,nhwij->nhwti", kw, ds), q.shape, ws, shift),
               dk=_map(dtype(scale) * np.einsum("nhwti,nhwij->nhwtj", qw, ds), q.shape, ws, shift),
               dv=_map(np.einsum("nhwri,nhwij->nhwrj", dow, p), v.shape, ws, shift))
    if table is not None:
        out["dtable"] = np.zeros(table.shape, dtype)
        for head in range(table.shape[0]):
            np.add.at(out["dtable"][head], rel, ds[:, head].sum((0, 1)))
    return out, smax


@functools.lru_cache(maxsize=None)
def _case(shape, overflow=False):
    """inputs (float32 values) and the float64 reference of one shape, made once"""
    n, heads, d, c, h, w, ws, shift, rel_bias = shape
    rs = np.random.RandomState(sum(shape) + 7 * d)
    draw = (lambda s: rs.randint(-4, 5, s).astype(np.float64)) if overflow else rs.standard_normal
    x = dict(q=draw((n, heads, d, h, w)), k=draw((n, heads, d, h, w)), v=rs.standard_normal((n, heads, c, h, w)),
             do=rs.standard_normal((n, heads, c, h, w)))
    x["table"] = rs.standard_normal((heads, (2 * ws - 1) ** 2)) if rel_bias else None
    x = {name: None if a is None else a.astype(np.float32).astype(np.float64) for name, a in x.items()}
    ref, smax = reference(x["q"], x["k"], x["v"], x["do"], x["table"], ws, shift, 1.0 if overflow else 1.0 / np.sqrt(d))
    return x, ref, smax


def _dev(a, off):
    """a on the device as [N][C][H][W] float32 (a table flat), `off` floats past an allocation's (16-byte aligned) start"""
    buf = torch.empty(a.size + off, dtype=torch.float32, device=DEV)
    buf[off:] = torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel())
    return buf[off:].view(a.shape[0], -1, *a.shape[3:]) if a.ndim == 5 else buf[off:]


def _run(shape, overflow=False, start=None, null=(), off=0):
    """forward and backward through ops; start: the gradients' start values (they accumulate), else dq, dk, dv are assigned
    over a fill of 7 and dtable starts at zero"""
    from bcnn_amd import ops
    heads, ws, shift = shape[1], shape[6], shape[7]
    x, ref, _ = _case(shape, overflow)
    scale = 1.0 if overflow else 0.0
    t = {name: None if a is None else _dev(a, off) for name, a in x.items()}
    o = _dev(np.zeros_like(ref["o"]), off)
    ops.window_attention_forward(t["q"], t["k"], t["v"], t["table"], o, heads, ws, shift, scale)
    fill = {name: np.zeros_like(ref[name]) if name == "dtable" else np.full_like(ref[name], 7.0) for name in ref if name != "o"}
    g = {name: None if name in null or name not in ref else _dev(fill[name] if start is None else start[name], off)
         for name in GRADS}
    ops.window_attention_backward(t["q"], t["k"], t["v"], t["table"], t["do"], g["dq"], g["dk"], g["dv"], g["dtable"], heads,
                                  ws, shift, scale, overwrite=(start is None,) * 3)
    torch.cuda.synchronize()
    out = dict(g, o=o)
    return {name: a.cpu().numpy().reshape(ref[name].shape) for name, a in out.items() if a is not None}


@functools.lru_cache(maxsize=None)
def _base(shape, overflow):
    """the plain run of a shape, made once and left unchanged"""
    return _run(shape, overflow)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_bits(a, b, names):
    for name in names:
        assert np.array_equal(_bits(a[name]), _bits(b[name])), name


@pytest.mark.parametrize("shape,check", CASES, ids=str)
def test_window_attention(shape, check):
    overflow, shape = len(shape) == 10, shape[:9]
    x, ref, smax = _case(shape, overflow)
    base = _base(shape, overflow)
    grads = [name for name in GRADS if name in ref]
    if check == "float64":
        if overflow:   # a condition on the inputs: exp without the maximum subtracted overflows float32 here
            assert smax > 89
        for name in ["o"] + grads:
            err, bar = np.abs(base[name] - ref[name]).max(), (DTABLE_TOL if name == "dtable" else TOL) * np.abs(ref[name]).max()
            print("%s: max error %.3g, bar %.3g" % (name, err, bar))
            assert err <= bar, (name, err, bar)
    elif check == "rerun":
        _same_bits(_run(shape, overflow), base, ["o"] + grads)
    elif check == "accumulate":
        rs = np.random.RandomState(5)
        start = {name: rs.standard_normal(ref[name].shape).astype(np.float32) for name in grads}
        got = _run(shape, overflow, start=start)
        _same_bits(got, {name: start[name] + base[name].astype(np.float32) for name in grads}, grads)
    elif check == "null":
        for name in grads:
            _same_bits(_run(shape, overflow, null=(name,)), base, [g for g in grads if g != name])
    else:   # misaligned
        _same_bits(_run(shape, overflow, off=1), base, ["o"] + grads)
