"""The group-normalisation kernels (bcnn_amd/csrc/group_norm.hip) through bcnn_amd.ops.

A row is one (image, group): m = (C / G) * H * W contiguous floats. With u = 2^-23 and float64 references whose sums run over
the m elements of a row:
  statistics  |mean - mean64| <= dm,  dm = u sum|x| + u |mean64|
              |rstd - rstd64| <= 0.505 rstd64^3 dv + u rstd64,  dv = (m + 1) u sum x^2 / m + 2 |mean64| dm + dm^2
              -- what every summation order of the float32 terms satisfies, propagated to first order;
  forward     y is the bits of the numpy float32 expression ((x - mean) * rstd) * gamma[ch] + beta[ch] on the kernel's own
              float32 mean and rstd; x, gamma, beta are not written; mean = rstd = None gives the same y;
  dx          from mean, rstd = the float32 roundings of the float64 statistics (the reference uses the same float32 values):
              overwrite: |dx - dx64| <= rstd (|xh| E_ds + E_db) / m + 8 2^-24 rstd (|t| + (|xh| |ds| + |db|) / m) per element,
              E_ds = m u sum|t xh|, E_db = m u sum|t|; accumulate: the bits of dx0 + (what the overwrite call returned);
  dgamma, dbeta  from a zero start |got - ref64| <= (N HW + 2) u sum_{n,hw}|term| per channel; from dg0 / db0 the bits of
              start + (zero-start result); each of dx, dgamma, dbeta = None leaves the others' bits as they are;
  two runs give the same bits; the dispatch trace names the path bcnn_hip_group_norm_path reports, once per launch, within
  the launch budget (forward 1, split 3; backward 2, split 4); the shapes reach all three paths in both directions.
The float64 formulas themselves are held to torch's CPU group_norm in float64, forward and autograd backward, to 1e-12."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
U = 2.0 ** -23
EPS = 1e-5
SHAPES = [(1, 1, 1, 1, 1), (2, 4, 1, 1, 2), (2, 6, 3, 3, 3), (2, 6, 7, 7, 6), (3, 8, 7, 7, 2), (4, 130, 2, 2, 65),
          (2, 32, 14, 14, 32), (2, 32, 14, 14, 1), (2, 6, 33, 35, 2), (2, 16, 40, 40, 1), (1, 4, 112, 112, 2),
          (1, 64, 56, 56, 2),
          # the branches below the path rule (one trace tag each, so the list has to name them):
          (1, 48, 14, 14, 1),   # m = 9408: backward split with planes below 1024 floats (a unit of lanes per plane)
          (1, 8, 21, 21, 2),    # m = 1764, HW = 441: resident float4s that straddle a channel boundary
          (1, 40, 21, 21, 1)]   # m = 17640, HW = 441: the same in the split map sweeps; small odd planes in the backward
# a lanes, a resident and a split shape again, one float past a 16-byte boundary; and the small-plane split backward
CASES = [(s, 0) for s in SHAPES] + [((3, 8, 7, 7, 2), 1), ((2, 32, 14, 14, 1), 1), ((2, 16, 40, 40, 1), 1),
                                    ((1, 48, 14, 14, 1), 1)]
FWD_BUDGET = {"lanes": 1, "resident": 1, "split": 3}
BWD_BUDGET = {"lanes": 2, "resident": 2, "split": 4}


def _dev(a, offset=0):
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + a.size]
    view.copy_(torch.from_numpy(np.array(a, F32).ravel()))   # (a copy: the shared case arrays are read-only)
    return view.view(a.shape)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


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


def _rows(a, n, g):
    return np.asarray(a).reshape(n, g, -1)


def _per_channel(c, g, hw):
    """index of gamma / beta for every element of a row-shaped [N, G, m] array: ch = g (C / G) + i / HW"""
    cg = c // g
    return (np.arange(g)[:, None] * cg + np.arange(cg * hw)[None, :] // hw)[None, :, :]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """data and float64 references of a shape, made once and shared (nothing below writes into them)"""
    n, c, h, w, g = shape
    hw, m = h * w, (c // g) * h * w
    rs = np.random.RandomState(n * 100000 + c * 1000 + h * 10 + g)
    d = dict(x=(rs.uniform(-2, 2, (n, c, h, w)) + 0.5).astype(F32), gamma=rs.uniform(0.5, 1.5, c).astype(F32),
             beta=rs.uniform(-1, 1, c).astype(F32), dy=rs.uniform(-1, 1, (n, c, h, w)).astype(F32),
             dx0=rs.uniform(-1, 1, (n, c, h, w)).astype(F32), dg0=rs.uniform(-1, 1, c).astype(F32),
             db0=rs.uniform(-1, 1, c).astype(F32))
    x = _rows(d["x"], n, g).astype(np.float64)
    d["mean64"] = x.mean(axis=2)
    d["var64"] = ((x - d["mean64"][:, :, None]) ** 2).mean(axis=2)
    d["rstd64"] = 1.0 / np.sqrt(d["var64"] + EPS)
    dm = U * np.abs(x).sum(axis=2) + U * np.abs(d["mean64"])
    dv = (m + 1) * U * (x * x).sum(axis=2) / m + 2 * np.abs(d["mean64"]) * dm + dm * dm
    d["mean_bound"] = dm
    d["rstd_bound"] = 0.505 * d["rstd64"] ** 3 * dv + U * d["rstd64"]
    # backward, from the float32 roundings of the statistics
    d["mean32"], d["rstd32"] = d["mean64"].astype(F32), d["rstd64"].astype(F32)
    mu, rstd = d["mean32"].astype(np.float64)[:, :, None], d["rstd32"].astype(np.float64)[:, :, None]
    ch = _per_channel(c, g, hw)
    xh = (x - mu) * rstd
    dy = _rows(d["dy"], n, g).astype(np.float64)
    t = dy * d["gamma"].astype(np.float64)[ch]
    ds, db = (t * xh).sum(axis=2, keepdims=True), t.sum(axis=2, keepdims=True)
    d["dx64"] = ((t - (xh * ds + db) / m) * rstd).reshape(n, c, h, w)
    e_ds = m * U * np.abs(t * xh).sum(axis=2, keepdims=True)
    e_db = m * U * np.abs(t).sum(axis=2, keepdims=True)
    d["dx_bound"] = (rstd * (np.abs(xh) * e_ds + e_db) / m +
                     8 * 2.0 ** -24 * rstd * (np.abs(t) + (np.abs(xh) * np.abs(ds) + np.abs(db)) / m)).reshape(n, c, h, w)
    term_g = (dy * xh).reshape(n, c, hw)
    term_b = dy.reshape(n, c, hw)
    d["dgamma64"], d["dbeta64"] = term_g.sum(axis=(0, 2)), term_b.sum(axis=(0, 2))
    d["dgamma_bound"] = (n * hw + 2) * U * np.abs(term_g).sum(axis=(0, 2))
    d["dbeta_bound"] = (n * hw + 2) * U * np.abs(term_b).sum(axis=(0, 2))
    for v in d.values():
        v.setflags(write=False)
    return d


def _forward(d, shape, offset, stats=True):
    from bcnn_amd import ops
    n, c, h, w, g = shape
    tx, tg, tb = _dev(d["x"], offset), _dev(d["gamma"], offset), _dev(d["beta"], offset)
    ty = _dev(np.full((n, c, h, w), 3.0, F32), offset)
    tm = _dev(np.full(n * g, 7.0, F32), offset) if stats else None
    tr = _dev(np.full(n * g, 7.0, F32), offset) if stats else None
    ops.group_norm_forward(tx, tg, tb, ty, tm, tr, g, EPS)
    torch.cuda.synchronize()
    for t, a in ((tx, d["x"]), (tg, d["gamma"]), (tb, d["beta"])):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a)), "the forward writes y and the statistics only"
    return ty.cpu().numpy(), (tm.cpu().numpy().reshape(n, g) if stats else None), (tr.cpu().numpy().reshape(n, g) if stats else None)


def _backward(d, shape, offset, dx0, dg0, db0, overwrite):
    from bcnn_amd import ops
    n, c, h, w, g = shape
    tx, tg, tdy = _dev(d["x"], offset), _dev(d["gamma"], offset), _dev(d["dy"], offset)
    tm, tr = _dev(d["mean32"], offset), _dev(d["rstd32"], offset)
    tdx = None if dx0 is None else _dev(dx0, offset)
    tdg = None if dg0 is None else _dev(dg0, offset)
    tdb = None if db0 is None else _dev(db0, offset)
    ops.group_norm_backward(tx, tg, tm, tr, tdy, tdx, tdg, tdb, g, overwrite)
    torch.cuda.synchronize()
    for t, a in ((tx, d["x"]), (tg, d["gamma"]), (tdy, d["dy"]), (tm, d["mean32"]), (tr, d["rstd32"])):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a)), "the backward reads x, gamma, dy, mean and rstd only"
    return tuple(None if t is None else t.cpu().numpy() for t in (tdx, tdg, tdb))


def _worst(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("shape,offset", CASES)
def test_forward(shape, offset):
    from bcnn_amd import ops
    n, c, h, w, g = shape
    d = _case(shape)
    path = ops.GROUP_NORM_PATHS[ops.group_norm_path(n, c, h * w, g)]
    _trace(True)
    y, mean, rstd = _forward(d, shape, offset)
    ran = _trace(False)
    assert ran and set(ran) == {"group_norm_fwd:" + path} and len(ran) <= FWD_BUDGET[path], ran
    err_m, err_r = np.abs(mean.astype(np.float64) - d["mean64"]), np.abs(rstd.astype(np.float64) - d["rstd64"])
    print("mean err / bound %.3g, rstd err / bound %.3g" % (_worst(err_m, d["mean_bound"]), _worst(err_r, d["rstd_bound"])))
    assert (err_m <= d["mean_bound"]).all() and (err_r <= d["rstd_bound"]).all()
    # y: the float32 expression on the kernel's own statistics, bit for bit
    ch = _per_channel(c, g, h * w)
    xh = (_rows(d["x"], n, g) - mean[:, :, None]) * rstd[:, :, None]
    want = (xh * d["gamma"][ch] + d["beta"][ch]).astype(F32)
    assert xh.dtype == F32 and np.array_equal(_bits(y), _bits(want.reshape(n, c, h, w))), "y"
    # no statistics asked for: the same y; and run to run
    y2, none_m, none_r = _forward(d, shape, offset, stats=False)
    assert none_m is None and none_r is None and np.array_equal(_bits(y2), _bits(y)), "mean = rstd = None"
    y3, mean3, rstd3 = _forward(d, shape, offset)
    assert np.array_equal(_bits(y3), _bits(y)) and np.array_equal(_bits(mean3), _bits(mean)) and \
        np.array_equal(_bits(rstd3), _bits(rstd)), "two runs, same bits"


@pytest.mark.parametrize("shape,offset", CASES)
def test_backward(shape, offset):
    from bcnn_amd import ops
    n, c, h, w, g = shape
    d = _case(shape)
    path = ops.GROUP_NORM_PATHS[ops.group_norm_path(n, c, h * w, g, True)]
    zeros_c = np.zeros(c, F32)
    _trace(True)
    dxv, dg_z, db_z = _backward(d, shape, offset, d["dx0"], zeros_c, zeros_c, True)
    ran = _trace(False)
    assert set(ran) == {"group_norm_bwd:" + path, "group_norm_bwd:params"} and ran.count("group_norm_bwd:params") == 1, ran
    assert len(ran) <= BWD_BUDGET[path], ran
    err = np.abs(dxv.astype(np.float64) - d["dx64"])
    err_g, err_b = np.abs(dg_z.astype(np.float64) - d["dgamma64"]), np.abs(db_z.astype(np.float64) - d["dbeta64"])
    print("dx err / bound %.3g, dgamma %.3g, dbeta %.3g" % (_worst(err, d["dx_bound"]), _worst(err_g, d["dgamma_bound"]),
                                                          _worst(err_b, d["dbeta_bound"])))
    assert (err <= d["dx_bound"]).all(), "dx (overwrite)"
    assert (err_g <= d["dgamma_bound"]).all() and (err_b <= d["dbeta_bound"]).all(), "dgamma, dbeta from a zero start"
    # accumulate: one float32 addition onto the start values
    dx, dg, db = _backward(d, shape, offset, d["dx0"], d["dg0"], d["db0"], False)
    assert np.array_equal(_bits(dx), _bits(d["dx0"] + dxv)), "dx = dx0 + dxv"
    assert np.array_equal(_bits(dg), _bits(d["dg0"] + dg_z)) and np.array_equal(_bits(db), _bits(d["db0"] + db_z))
    # run to run
    again = _backward(d, shape, offset, d["dx0"], d["dg0"], d["db0"], False)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, (dx, dg, db))), "two runs, same bits"
    # each output absent: the others unchanged
    none_x, dg1, db1 = _backward(d, shape, offset, None, d["dg0"], d["db0"], False)
    assert none_x is None and np.array_equal(_bits(dg1), _bits(dg)) and np.array_equal(_bits(db1), _bits(db)), "dx = None"
    dx2, none_g, db2 = _backward(d, shape, offset, d["dx0"], None, d["db0"], False)
    assert none_g is None and np.array_equal(_bits(dx2), _bits(dx)) and np.array_equal(_bits(db2), _bits(db)), "dgamma = None"
    dx3, dg3, none_b = _backward(d, shape, offset, d["dx0"], d["dg0"], None, False)
    assert none_b is None and np.array_equal(_bits(dx3), _bits(dx)) and np.array_equal(_bits(dg3), _bits(dg)), "dbeta = None"
    # no parameter gradient asked for: the data gradient alone, one launch fewer
    _trace(True)
    dx4, _, _ = _backward(d, shape, offset, d["dx0"], None, None, True)
    ran = _trace(False)
    assert set(ran) == {"group_norm_bwd:" + path} and len(ran) <= BWD_BUDGET[path] - 1, ran
    assert np.array_equal(_bits(dx4), _bits(dxv))


def test_shapes_reach_every_path():
    """if the thresholds move, move the shapes, not this assertion"""
    from bcnn_amd import ops
    for backward in (False, True):
        seen = {ops.GROUP_NORM_PATHS[ops.group_norm_path(n, c, h * w, g, backward)] for n, c, h, w, g in SHAPES}
        assert seen == {"lanes", "resident", "split"}, (backward, seen)


@pytest.mark.parametrize("shape", [(3, 8, 7, 7, 2), (2, 6, 33, 35, 2)])
def test_the_float64_formulas_are_torchs_group_norm(shape):
    """the references above against torch.nn.functional.group_norm in float64 on the CPU, forward and autograd backward"""
    n, c, h, w, g = shape
    d = _case(shape)
    m = (c // g) * h * w
    x = torch.tensor(d["x"], dtype=torch.float64, requires_grad=True)
    gamma = torch.tensor(d["gamma"], dtype=torch.float64, requires_grad=True)
    beta = torch.tensor(d["beta"], dtype=torch.float64, requires_grad=True)
    y = F.group_norm(x, g, gamma, beta, EPS)
    y.backward(torch.tensor(d["dy"], dtype=torch.float64))
    # the formulas of this file in full float64 (statistics included)
    ch = _per_channel(c, g, h * w)
    xr = _rows(d["x"], n, g).astype(np.float64)
    xh = (xr - d["mean64"][:, :, None]) * d["rstd64"][:, :, None]
    g64, b64 = d["gamma"].astype(np.float64), d["beta"].astype(np.float64)
    assert np.abs((xh * g64[ch] + b64[ch]).reshape(n, c, h, w) - y.detach().numpy()).max() <= 1e-12
    dy = _rows(d["dy"], n, g).astype(np.float64)
    t = dy * g64[ch]
    ds, db = (t * xh).sum(axis=2, keepdims=True), t.sum(axis=2, keepdims=True)
    dx = (t - (xh * ds + db) / m) * d["rstd64"][:, :, None]
    assert np.abs(dx.reshape(n, c, h, w) - x.grad.numpy()).max() <= 1e-12
    assert np.abs((dy * xh).reshape(n, c, -1).sum(axis=(0, 2)) - gamma.grad.numpy()).max() <= 1e-12
    assert np.abs(dy.reshape(n, c, -1).sum(axis=(0, 2)) - beta.grad.numpy()).max() <= 1e-12
