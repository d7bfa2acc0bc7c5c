"""The patch-expanding kernels (bcnn_amd/csrc/patch_expand.hip) through bcnn_amd.ops, against float64 numpy: the rearrangement
done with reshape / transpose, fed to reference() of tests/test_channel_norm.py with m = c. Its bounds are derived ones (what
every summation order of the float32 terms satisfies), not what the kernels were seen to give. norm = 0 is compared bit for
bit, order = channels against torch's pixel_shuffle on the CPU."""
import functools

import numpy as np
import pytest
import torch

from tests.test_channel_norm import reference
from tests.test_group_norm import _bits, _dev, _trace

pytestmark = pytest.mark.gpu
F32 = np.float32
EPS = 1e-5
# (N, c, H, W) of the input grid, c the OUTPUT channels; c may name a path limit of ops.patch_expand_limits(block) or what
# the backward keeps per workgroup (ops.PATCH_EXPAND_BWD_*), resolved when the test runs
SHAPES = [(1, 1, 1, 1),                  # one input position, variance 0
          (2, 3, 2, 3),                  # odd c, odd W
          (3, 2, 5, 13),                 # 65 positions per image: a wave spans two images
          (1, "column", 1, 3), (1, "column+1", 1, 3), (1, "split", 1, 3), (1, "split+1", 1, 3),
          (2, 130, 1, 1),                # wide, fewer positions than lanes
          (1, "hold+1", 1, 3),           # the backward re-reads x and dy
          (1, "lds+1", 1, 1),            # the backward's per-channel accumulators leave LDS
          (1, 2, 182, 182)]              # 518 tiles: more than persistent workgroups
# every shape at both blocks in the order `blocks`; three of them in the order `channels`; three again with every buffer one
# float past a 16-byte boundary (no wide access)
CASES = [(s, p, "blocks", 0) for s in SHAPES for p in (2, 4)]
CASES += [(s, p, "channels", 0) for s in ((2, 3, 2, 3), (3, 2, 5, 13), (1, "split", 1, 3)) for p in (2, 4)]
CASES += [((2, 3, 2, 3), 2, "blocks", 1), ((3, 2, 5, 13), 4, "channels", 1), ((2, 130, 1, 1), 4, "blocks", 1)]


def _shape(spec, p):
    from bcnn_amd import ops
    n, c, h, w = spec
    if isinstance(c, str):
        limits = dict(zip(("column", "split"), ops.patch_expand_limits(p)), hold=ops.PATCH_EXPAND_BWD_HOLD_MAX_C,
                      lds=ops.PATCH_EXPAND_BWD_LDS_MAX_C)
        c = limits[c.split("+")[0]] + c.count("+1")
    return n, c, h, w


def expand(x, p, order):
    """[N,p^2 c,H,W] -> [N,c,pH,pW]; source plane (p1 p + p2) c + ch (blocks) or ch p^2 + p1 p + p2 (channels)"""
    n, c_in, h, w = x.shape
    c = c_in // (p * p)
    v = x.reshape(n, p, p, c, h, w).transpose(0, 3, 4, 1, 5, 2) if order == "blocks" else x.reshape(n, c, p, p, h, w).transpose(0, 1, 4, 2, 5, 3)
    return np.ascontiguousarray(v).reshape(n, c, p * h, p * w)


def unexpand(g, p, order):
    n, c, ph, pw = g.shape
    v = g.reshape(n, c, ph // p, p, pw // p, p)   # n, ch, h, p1, w, p2
    v = v.transpose(0, 3, 5, 1, 2, 4) if order == "blocks" else v.transpose(0, 1, 3, 5, 2, 4)
    return np.ascontiguousarray(v).reshape(n, c * p * p, ph // p, pw // p)


@functools.lru_cache(maxsize=None)
def _case(shape, p, order):
    n, c, h, w = shape
    src, out = (n, p * p * c, h, w), (n, c, p * h, p * w)
    rs = np.random.RandomState(n * 100000 + c * 1000 + h * 10 + w + p)
    d = dict(x=(rs.uniform(-2, 2, src) + 0.5).astype(F32), scales=rs.uniform(0.5, 1.5, c).astype(F32),
             b=rs.uniform(-1, 1, c).astype(F32), dy=rs.uniform(-1, 1, out).astype(F32),
             dx0=rs.uniform(-1, 1, src).astype(F32), ds0=rs.uniform(-1, 1, c).astype(F32), db0=rs.uniform(-1, 1, c).astype(F32))
    d["expanded"] = expand(d["x"], p, order)
    d.update(reference(d["expanded"].reshape(n, c, -1).astype(np.float64), d["scales"].astype(np.float64),
                       d["dy"].reshape(n, c, -1).astype(np.float64)))
    for v in d.values():
        v.setflags(write=False)
    return d


def _forward(d, p, order, offset, norm=True, stats=True, eps=EPS):
    from bcnn_amd import ops
    n, rows = d["dy"].shape[0], d["dy"].size // d["dy"].shape[1]
    tx, ts, tb = _dev(d["x"], offset), _dev(d["scales"], offset), _dev(d["b"], offset)
    ty = _dev(np.full(d["dy"].shape, 3.0, F32), offset)
    tm, tr = (_dev(np.full(rows, 7.0, F32), offset), _dev(np.full(rows, 7.0, F32), offset)) if stats else (None, None)
    ops.patch_expand_forward(tx, ts if norm else None, tb if norm else None, ty, tm, tr, p, order, eps)
    torch.cuda.synchronize()
    for t, a in ((tx, d["x"]), (ts, d["scales"]), (tb, d["b"])):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a)), "the forward writes y and the statistics only"
    return ty.cpu().numpy(), (tm.cpu().numpy().reshape(n, -1) if stats else None), (tr.cpu().numpy().reshape(n, -1) if stats else None)


def _backward(d, p, order, offset, dx0, ds0, db0, overwrite, norm=True):
    from bcnn_amd import ops
    tx, ts, tdy = _dev(d["x"], offset), _dev(d["scales"], offset), _dev(d["dy"], offset)
    tm, tr = _dev(d["mean32"], offset), _dev(d["rstd32"], offset)
    out = [None if a is None else _dev(a, offset) for a in (dx0, ds0, db0)]
    if norm:
        ops.patch_expand_backward(tx, ts, tm, tr, tdy, out[0], out[1], out[2], p, order, overwrite)
    else:
        ops.patch_expand_backward(None, None, None, None, tdy, out[0], None, None, p, order, overwrite)
    torch.cuda.synchronize()
    for t, a in ((tx, d["x"]), (tdy, d["dy"]), (ts, d["scales"])):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a)), "the backward writes the gradients only"
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _path(shape, p):
    from bcnn_amd import ops
    n, c, h, w = shape
    return ops.PATCH_EXPAND_PATHS[ops.patch_expand_path(n, p * p * c, h, w, p)]


@pytest.mark.parametrize("spec,p,order,offset", CASES)
def test_forward(spec, p, order, offset):
    shape = _shape(spec, p)
    n, c = shape[:2]
    d = _case(shape, p, order)
    _trace(True)
    y, mean, rstd = _forward(d, p, order, offset)
    ran = _trace(False)
    assert ran == ["patch_expand_fwd:" + _path(shape, p)], ran
    err_m, err_r = np.abs(mean.astype(np.float64) - d["mean64"]), np.abs(rstd.astype(np.float64) - d["rstd64"])
    print("mean / bound %.3g, rstd / bound %.3g" % ((err_m / d["mean_bound"]).max(), (err_r / d["rstd_bound"]).max()))
    assert (err_m <= d["mean_bound"]).all() and (err_r <= d["rstd_bound"]).all()
    xh = (d["expanded"].reshape(n, c, -1) - mean[:, None, :]) * rstd[:, None, :]
    want = xh * d["scales"][None, :, None] + d["b"][None, :, None]
    assert want.dtype == F32 and np.array_equal(_bits(y), _bits(want.reshape(y.shape))), "y"
    y2, none_m, none_r = _forward(d, p, order, offset, stats=False)
    assert none_m is None and none_r is None and np.array_equal(_bits(y2), _bits(y)), "mean = rstd = None"
    y3, mean3, rstd3 = _forward(d, p, order, offset, eps=0.0)   # eps <= 0 selects 1e-5
    assert np.array_equal(_bits(y3), _bits(y)) and np.array_equal(_bits(mean3), _bits(mean)) and \
        np.array_equal(_bits(rstd3), _bits(rstd)), "two runs, same bits"


@pytest.mark.parametrize("spec,p,order,offset", CASES)
def test_backward(spec, p, order, offset):
    shape = _shape(spec, p)
    n, c = shape[:2]
    d = _case(shape, p, order)
    zeros = np.zeros(c, F32)
    _trace(True)
    dxv, ds_z, db_z = _backward(d, p, order, offset, d["dx0"], zeros, zeros, True)
    ran = _trace(False)
    assert ran == ["patch_expand_bwd:" + _path(shape, p), "patch_expand_finalize"], ran
    err = np.abs(expand(dxv, p, order).reshape(n, c, -1).astype(np.float64) - d["dx64"])
    err_s, err_b = np.abs(ds_z.astype(np.float64) - d["dscales64"]), np.abs(db_z.astype(np.float64) - d["db64"])
    print("dx / bound %.3g, dscales / bound %.3g, db / bound %.3g" % tuple(
        (e / np.maximum(b, 1e-300)).max() for e, b in ((err, d["dx_bound"]), (err_s, d["dscales_bound"]), (err_b, d["db_bound"]))))
    assert (err <= d["dx_bound"]).all(), "dx (overwrite)"
    assert (err_s <= d["dscales_bound"]).all() and (err_b <= d["db_bound"]).all(), "dscales, db from a zero start"
    dx, ds, db = _backward(d, p, order, offset, d["dx0"], d["ds0"], d["db0"], False)
    assert np.array_equal(_bits(dx), _bits(d["dx0"] + dxv)), "dx = dx0 + dxv"
    assert np.array_equal(_bits(ds), _bits(d["ds0"] + ds_z)) and np.array_equal(_bits(db), _bits(d["db0"] + db_z))
    again = _backward(d, p, order, offset, d["dx0"], d["ds0"], d["db0"], False)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, (dx, ds, db))), "two runs, same bits"
    for absent in range(3):
        starts = [d["dx0"], d["ds0"], d["db0"]]
        starts[absent] = None
        got = _backward(d, p, order, offset, starts[0], starts[1], starts[2], False)
        for k, full in enumerate((dx, ds, db)):
            assert (got[k] is None) if k == absent else np.array_equal(_bits(got[k]), _bits(full)), (absent, k)


@pytest.mark.parametrize("spec,p,order,offset", [(s, p, o, off) for s, p, _, off in CASES[:2 * len(SHAPES)] + CASES[-3:]
                                                 for o in ("blocks", "channels")])
def test_rearrangement_alone_is_bit_exact(spec, p, order, offset):
    shape = _shape(spec, p)
    d = _case(shape, p, order)
    _trace(True)
    y, _, _ = _forward(d, p, order, offset, norm=False, stats=False)
    dx, _, _ = _backward(d, p, order, offset, d["dx0"], None, None, True, norm=False)
    assert _trace(False) == ["patch_expand_fwd:copy", "patch_expand_bwd:copy"]
    want = torch.nn.functional.pixel_shuffle(torch.from_numpy(d["x"].copy()), p).numpy() if order == "channels" else d["expanded"]
    assert np.array_equal(_bits(y), _bits(want)) and np.array_equal(_bits(dx), _bits(unexpand(d["dy"], p, order)))
    dx_add, _, _ = _backward(d, p, order, offset, d["dx0"], None, None, False, norm=False)
    assert np.array_equal(_bits(dx_add), _bits(d["dx0"] + unexpand(d["dy"], p, order)))


@pytest.mark.parametrize("p,order", [(2, 2), (4, -1)])
def test_an_unknown_order_launches_nothing_and_writes_nothing(p, order):
    d = _case((2, 3, 2, 3), p, "blocks")
    _trace(True)
    y, mean, rstd = _forward(d, p, order, 0)
    got = _backward(d, p, order, 0, d["dx0"], d["ds0"], d["db0"], True)
    assert _trace(False) == []
    assert (y == 3.0).all() and (mean == 7.0).all() and (rstd == 7.0).all()
    assert all(np.array_equal(_bits(a), _bits(d[k])) for a, k in zip(got, ("dx0", "ds0", "db0")))
