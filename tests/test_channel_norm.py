"""The channel-norm kernels (bcnn_amd/csrc/channel_norm.hip) through bcnn_amd.ops, against float64 numpy. A row is one
position (n, p): its m = C channel values. The bounds are those of tests/test_group_norm.py (derived in its docstring) with
m = C: what every summation order of the float32 terms satisfies, not what the kernels were seen to give."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_group_norm import _bits, _dev, _trace

pytestmark = pytest.mark.gpu
F32 = np.float32
U = 2.0 ** -23
EPS = 1e-5
SHAPES = [(1, 1, 1, 1),        # variance 0: rstd = 1 / sqrt(eps)
          (2, 3, 1, 1), (2, 5, 3, 3),
          (3, 8, 5, 13),       # 65 positions per image: a wave spans two images; the backward's column limit ...
          (3, 9, 5, 13),       # ... and past it
          (1, 16, 7, 7), (1, 17, 7, 7),                     # the forward's column limit
          (2, 64, 8, 8),       # 16-byte route, several waves per tile
          (1, 96, 14, 14),     # a ragged last tile
          (1, 238, 4, 16), (1, 239, 4, 16),                 # the forward's resident limit
          (1, 768, 7, 7),      # stream over flattened positions; three passes of per-channel sums in the backward
          (2, 520, 2, 2),      # stream with fewer positions than lanes
          # more tiles than persistent workgroups (512 of one tile list each; a column workgroup is four lists)
          (1, 34, 182, 182), (1, 4, 363, 363)]
# a column, a resident / stream and a stream shape again with every buffer one float past a 16-byte boundary
CASES = [(s, 0) for s in SHAPES] + [((3, 8, 5, 13), 1), ((2, 64, 8, 8), 1), ((2, 520, 2, 2), 1)]
BWD_CASES = CASES + [((1, 260, 182, 182), 0)]   # a tile list of two entries in the passes past the first 256 channels


def reference(x, scales, dy, eps=EPS, stats=None):
    """float64 statistics, bounds and gradients of [N, C, HW] arrays; the backward from `stats` or their float32 roundings"""
    n, m, hw = x.shape
    d = {}
    d["mean64"] = x.mean(axis=1)
    d["rstd64"] = 1.0 / np.sqrt(((x - d["mean64"][:, None]) ** 2).mean(axis=1) + eps)
    dm = U * np.abs(x).sum(axis=1) + U * np.abs(d["mean64"])
    dv = (m + 1) * U * (x * x).sum(axis=1) / m + 2 * np.abs(d["mean64"]) * dm + dm * dm
    d["mean_bound"], d["rstd_bound"] = dm, 0.505 * d["rstd64"] ** 3 * dv + U * d["rstd64"]
    d["mean32"], d["rstd32"] = stats if stats is not None else (d["mean64"].astype(F32), d["rstd64"].astype(F32))
    mu, rstd = d["mean32"].astype(np.float64)[:, None], d["rstd32"].astype(np.float64)[:, None]
    xh = (x - mu) * rstd
    t = dy * scales[None, :, None]
    ds, db = (t * xh).sum(axis=1, keepdims=True), t.sum(axis=1, keepdims=True)
    d["dx64"] = (t - (xh * ds + db) / m) * rstd
    e_ds, e_db = m * U * np.abs(t * xh).sum(axis=1, keepdims=True), m * U * np.abs(t).sum(axis=1, keepdims=True)
    d["dx_bound"] = (rstd * (np.abs(xh) * e_ds + e_db) / m +
                     8 * 2.0 ** -24 * rstd * (np.abs(t) + (np.abs(xh) * np.abs(ds) + np.abs(db)) / m))
    d["dscales64"], d["db64"] = (dy * xh).sum(axis=(0, 2)), dy.sum(axis=(0, 2))
    d["dscales_bound"] = (n * hw + 2) * U * np.abs(dy * xh).sum(axis=(0, 2))
    d["db_bound"] = (n * hw + 2) * U * np.abs(dy).sum(axis=(0, 2))
    return d


@functools.lru_cache(maxsize=None)
def _case(shape):
    n, c, h, w = shape
    rs = np.random.RandomState(n * 100000 + c * 1000 + h * 10 + w)
    d = dict(x=(rs.uniform(-2, 2, shape) + 0.5).astype(F32), scales=rs.uniform(0.5, 1.5, c).astype(F32),
             b=rs.uniform(-1, 1, c).astype(F32), dy=rs.uniform(-1, 1, shape).astype(F32),
             dx0=rs.uniform(-1, 1, shape).astype(F32), ds0=rs.uniform(-1, 1, c).astype(F32),
             db0=rs.uniform(-1, 1, c).astype(F32))
    d.update(reference(d["x"].reshape(n, c, -1).astype(np.float64), d["scales"].astype(np.float64),
                       d["dy"].reshape(n, c, -1).astype(np.float64)))
    for v in d.values():
        v.setflags(write=False)
    return d


def _forward(d, shape, offset, stats=True, eps=EPS):
    from bcnn_amd import ops
    n, c, h, w = shape
    tx, ts, tb = _dev(d["x"], offset), _dev(d["scales"], offset), _dev(d["b"], offset)
    ty = _dev(np.full(shape, 3.0, F32), offset)
    tm = _dev(np.full(n * h * w, 7.0, F32), offset) if stats else None
    tr = _dev(np.full(n * h * w, 7.0, F32), offset) if stats else None
    ops.channel_norm_forward(tx, ts, tb, ty, tm, tr, eps)
    torch.cuda.synchronize()
    for t, a in ((tx, d["x"]), (ts, d["scales"]), (tb, d["b"])):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a)), "the forward writes y and the statistics only"
    return ty.cpu().numpy(), (tm.cpu().numpy().reshape(n, -1) if stats else None), (tr.cpu().numpy().reshape(n, -1) if stats else None)


def _backward(d, shape, offset, dx0, ds0, db0, overwrite):
    from bcnn_amd import ops
    tx, ts, tdy = _dev(d["x"], offset), _dev(d["scales"], offset), _dev(d["dy"], offset)
    tm, tr = _dev(d["mean32"], offset), _dev(d["rstd32"], offset)
    out = [None if a is None else _dev(a, offset) for a in (dx0, ds0, db0)]
    ops.channel_norm_backward(tx, ts, tm, tr, tdy, out[0], out[1], out[2], overwrite)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


@pytest.mark.parametrize("shape,offset", CASES)
def test_forward(shape, offset):
    from bcnn_amd import ops
    n, c, h, w = shape
    d = _case(shape)
    path = ops.CHANNEL_NORM_PATHS[ops.channel_norm_path(n, c, h * w)]
    _trace(True)
    y, mean, rstd = _forward(d, shape, offset)
    ran = _trace(False)
    assert ran == ["channel_norm_fwd:" + path], ran
    err_m, err_r = np.abs(mean.astype(np.float64) - d["mean64"]), np.abs(rstd.astype(np.float64) - d["rstd64"])
    assert (err_m <= d["mean_bound"]).all() and (err_r <= d["rstd_bound"]).all()
    xh = (d["x"].reshape(n, c, -1) - mean[:, None, :]) * rstd[:, None, :]
    want = xh * d["scales"][None, :, None] + d["b"][None, :, None]
    assert want.dtype == F32 and np.array_equal(_bits(y), _bits(want.reshape(shape))), "y"
    y2, none_m, none_r = _forward(d, shape, offset, stats=False)
    assert none_m is None and none_r is None and np.array_equal(_bits(y2), _bits(y)), "mean = rstd = None"
    y3, mean3, rstd3 = _forward(d, shape, offset, eps=0.0)   # eps <= 0 selects 1e-5
    assert np.array_equal(_bits(y3), _bits(y)) and np.array_equal(_bits(mean3), _bits(mean)) and \
        np.array_equal(_bits(rstd3), _bits(rstd)), "two runs, same bits"


@pytest.mark.parametrize("shape,offset", BWD_CASES)
def test_backward(shape, offset):
    from bcnn_amd import ops
    n, c, h, w = shape
    d = _case(shape)
    path = ops.CHANNEL_NORM_PATHS[ops.channel_norm_path(n, c, h * w, True)]
    _trace(True)
    dxv, ds_z, db_z = _backward(d, shape, offset, d["dx0"], np.zeros(c, F32), np.zeros(c, F32), True)
    ran = _trace(False)
    assert ran == ["channel_norm_bwd:" + path, "channel_norm_bwd:params"], ran
    err = np.abs(dxv.reshape(n, c, -1).astype(np.float64) - d["dx64"])
    err_s, err_b = np.abs(ds_z.astype(np.float64) - d["dscales64"]), np.abs(db_z.astype(np.float64) - d["db64"])
    assert (err <= d["dx_bound"]).all(), "dx (overwrite)"
    assert (err_s <= d["dscales_bound"]).all() and (err_b <= d["db_bound"]).all(), "dscales, db from a zero start"
    dx, ds, db = _backward(d, shape, offset, d["dx0"], d["ds0"], d["db0"], False)
    assert np.array_equal(_bits(dx), _bits(d["dx0"] + dxv)), "dx = dx0 + dxv"
    assert np.array_equal(_bits(ds), _bits(d["ds0"] + ds_z)) and np.array_equal(_bits(db), _bits(d["db0"] + db_z))
    again = _backward(d, shape, offset, d["dx0"], d["ds0"], d["db0"], False)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, (dx, ds, db))), "two runs, same bits"
    for absent in range(3):
        starts = [d["dx0"], d["ds0"], d["db0"]]
        starts[absent] = None
        got = _backward(d, shape, offset, starts[0], starts[1], starts[2], False)
        for k, full in enumerate((dx, ds, db)):
            assert (got[k] is None) if k == absent else np.array_equal(_bits(got[k]), _bits(full)), (absent, k)
    dx4, _, _ = _backward(d, shape, offset, d["dx0"], None, None, True)
    assert np.array_equal(_bits(dx4), _bits(dxv)), "no parameter gradient asked for: the same data gradient"


@pytest.mark.parametrize("shape", [(3, 8, 5, 13), (2, 64, 8, 8)])
def test_the_float64_formulas_are_torchs_layer_norm(shape):
    """the references above in full float64 against torch's CPU layer_norm on the permuted tensor, forward and autograd"""
    n, c, h, w = shape
    d = _case(shape)
    x, g, b = (torch.tensor(d[k], dtype=torch.float64, requires_grad=True) for k in ("x", "scales", "b"))
    y = F.layer_norm(x.permute(0, 2, 3, 1), (c,), g, b, EPS).permute(0, 3, 1, 2)
    y.backward(torch.tensor(d["dy"], dtype=torch.float64))
    x64, g64 = d["x"].reshape(n, c, -1).astype(np.float64), d["scales"].astype(np.float64)
    r = reference(x64, g64, d["dy"].reshape(n, c, -1).astype(np.float64), stats=(d["mean64"], d["rstd64"]))
    y64 = (x64 - d["mean64"][:, None]) * d["rstd64"][:, None] * g64[None, :, None] + d["b"][None, :, None]
    for ours, torchs in ((y64, y.detach()), (r["dx64"], x.grad), (r["dscales64"], g.grad), (r["db64"], b.grad)):
        assert np.abs(ours.reshape(torchs.shape) - torchs.numpy()).max() <= 1e-12
