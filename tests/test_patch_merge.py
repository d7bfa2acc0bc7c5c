"""The patch-merging kernels (bcnn_amd/csrc/patch_merge.hip) through bcnn_amd.ops, against float64 numpy: the rearrangement
done in numpy, fed to reference() of tests/test_channel_norm.py with m = 4C. Its bounds are derived ones (what every summation
order of the float32 terms satisfies), not what the kernels were seen to give. norm = 0 is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests.test_channel_norm import reference
from tests.test_group_norm import _bits, _dev, _trace

pytestmark = pytest.mark.gpu
F32 = np.float32
EPS = 1e-5
# C may name a path limit of ops.patch_merge_limits() (column, split), resolved when the test runs
SHAPES = [(1, 1, 2, 2),                  # one output position
          (2, 3, 4, 6),                  # odd C; W/2 = 3: the 8-byte pairs are never 16-byte aligned
          (3, 2, 10, 26),                # 65 output positions per image: a wave spans two images
          (1, "column", 2, 6), (1, "column+1", 2, 6), (1, "split", 2, 2), (1, "split+1", 2, 2),
          (1, 40, 4, 2),                 # four channels per wave
          (1, 96, 14, 14),               # Swin-T's last transition: 4C = 384, 49 positions
          (2, 130, 2, 2),                # wide, fewer positions than lanes; the backward re-reads; 4C = 520 > 256
          (1, 513, 2, 2),                # 4C past the backward's LDS accumulators
          (1, 2, 364, 364)]              # 518 tiles: more than persistent workgroups
# three of them again with every buffer one float past a 16-byte boundary (no 8-byte pairs)
CASES = [(s, 0) for s in SHAPES] + [((2, 3, 4, 6), 1), ((1, 96, 14, 14), 1), ((2, 130, 2, 2), 1)]


def _shape(spec):
    from bcnn_amd import ops
    n, c, h, w = spec
    if isinstance(c, str):
        limits = dict(zip(("column", "split"), ops.patch_merge_limits()))
        c = limits[c.split("+")[0]] + c.count("+1")
    return n, c, h, w


def merge(x):
    """[N,C,H,W] -> [N,4C,H/2,W/2], output channel (2 dx + dy) C + c"""
    return np.concatenate([x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]], axis=1)


def unmerge(g):
    n, c4, oh, ow = g.shape
    c = c4 // 4
    x = np.zeros((n, c, 2 * oh, 2 * ow), g.dtype)
    for k, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        x[:, :, dy::2, dx::2] = g[:, k * c:(k + 1) * c]
    return x


@functools.lru_cache(maxsize=None)
def _case(shape):
    n, c, h, w = shape
    out = (n, 4 * c, h // 2, w // 2)
    rs = np.random.RandomState(n * 100000 + c * 1000 + h * 10 + w)
    d = dict(x=(rs.uniform(-2, 2, shape) + 0.5).astype(F32), scales=rs.uniform(0.5, 1.5, 4 * c).astype(F32),
             b=rs.uniform(-1, 1, 4 * c).astype(F32), dy=rs.uniform(-1, 1, out).astype(F32),
             dx0=rs.uniform(-1, 1, shape).astype(F32), ds0=rs.uniform(-1, 1, 4 * c).astype(F32),
             db0=rs.uniform(-1, 1, 4 * c).astype(F32))
    d["merged"] = merge(d["x"])
    d.update(reference(d["merged"].reshape(n, 4 * c, -1).astype(np.float64), d["scales"].astype(np.float64),
                       d["dy"].reshape(n, 4 * c, -1).astype(np.float64)))
    for v in d.values():
        v.setflags(write=False)
    return d


def _forward(d, shape, offset, norm=True, stats=True, eps=EPS):
    from bcnn_amd import ops
    n, c, h, w = shape
    rows = n * (h // 2) * (w // 2)
    tx, ts, tb = _dev(d["x"], offset), _dev(d["scales"], offset), _dev(d["b"], offset)
    ty = _dev(np.full(d["dy"].shape, 3.0, F32), offset)
    tm, tr = (_dev(np.full(rows, 7.0, F32), offset), _dev(np.full(rows, 7.0, F32), offset)) if stats else (None, None)
    ops.patch_merge_forward(tx, ts if norm else None, tb if norm else None, ty, tm, tr, eps)
    torch.cuda.synchronize()
    for t, a in ((tx, d["x"]), (ts, d["scales"]), (tb, d["b"])):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a)), "the forward writes y and the statistics only"
    return ty.cpu().numpy(), (tm.cpu().numpy().reshape(n, -1) if stats else None), (tr.cpu().numpy().reshape(n, -1) if stats else None)


def _backward(d, shape, offset, dx0, ds0, db0, overwrite, norm=True):
    from bcnn_amd import ops
    tx, ts, tdy = _dev(d["x"], offset), _dev(d["scales"], offset), _dev(d["dy"], offset)
    tm, tr = _dev(d["mean32"], offset), _dev(d["rstd32"], offset)
    out = [None if a is None else _dev(a, offset) for a in (dx0, ds0, db0)]
    if norm:
        ops.patch_merge_backward(tx, ts, tm, tr, tdy, out[0], out[1], out[2], overwrite)
    else:
        ops.patch_merge_backward(None, None, None, None, tdy, out[0], None, None, overwrite)
    torch.cuda.synchronize()
    for t, a in ((tx, d["x"]), (tdy, d["dy"]), (ts, d["scales"])):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a)), "the backward writes the gradients only"
    return tuple(None if t is None else t.cpu().numpy() for t in out)


@pytest.mark.parametrize("spec,offset", CASES)
def test_forward(spec, offset):
    from bcnn_amd import ops
    shape = _shape(spec)
    n, c, h, w = shape
    d = _case(shape)
    _trace(True)
    y, mean, rstd = _forward(d, shape, offset)
    ran = _trace(False)
    assert ran == ["patch_merge_fwd:" + ops.PATCH_MERGE_PATHS[ops.patch_merge_path(n, c, h, w)]], ran
    err_m, err_r = np.abs(mean.astype(np.float64) - d["mean64"]), np.abs(rstd.astype(np.float64) - d["rstd64"])
    assert (err_m <= d["mean_bound"]).all() and (err_r <= d["rstd_bound"]).all()
    xh = (d["merged"].reshape(n, 4 * c, -1) - mean[:, None, :]) * rstd[:, None, :]
    want = xh * d["scales"][None, :, None] + d["b"][None, :, None]
    assert want.dtype == F32 and np.array_equal(_bits(y), _bits(want.reshape(y.shape))), "y"
    y2, none_m, none_r = _forward(d, shape, offset, stats=False)
    assert none_m is None and none_r is None and np.array_equal(_bits(y2), _bits(y)), "mean = rstd = None"
    y3, mean3, rstd3 = _forward(d, shape, offset, eps=0.0)   # eps <= 0 selects 1e-5
    assert np.array_equal(_bits(y3), _bits(y)) and np.array_equal(_bits(mean3), _bits(mean)) and \
        np.array_equal(_bits(rstd3), _bits(rstd)), "two runs, same bits"


@pytest.mark.parametrize("spec,offset", CASES)
def test_backward(spec, offset):
    from bcnn_amd import ops
    shape = _shape(spec)
    n, c, h, w = shape
    d = _case(shape)
    zeros = np.zeros(4 * c, F32)
    _trace(True)
    dxv, ds_z, db_z = _backward(d, shape, offset, d["dx0"], zeros, zeros, True)
    ran = _trace(False)
    assert ran == ["patch_merge_bwd:" + ops.PATCH_MERGE_PATHS[ops.patch_merge_path(n, c, h, w)], "patch_merge_finalize"], ran
    err = np.abs(merge(dxv).reshape(n, 4 * c, -1).astype(np.float64) - d["dx64"])
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


@pytest.mark.parametrize("spec,offset", CASES)
def test_rearrangement_alone_is_bit_exact(spec, offset):
    shape = _shape(spec)
    d = _case(shape)
    _trace(True)
    y, _, _ = _forward(d, shape, offset, norm=False, stats=False)
    dx, _, _ = _backward(d, shape, offset, d["dx0"], None, None, True, norm=False)
    assert _trace(False) == ["patch_merge_fwd:copy", "patch_merge_bwd:copy"]
    assert np.array_equal(_bits(y), _bits(d["merged"])) and np.array_equal(_bits(dx), _bits(unmerge(d["dy"])))
    dx_add, _, _ = _backward(d, shape, offset, d["dx0"], None, None, False, norm=False)
    assert np.array_equal(_bits(dx_add), _bits(d["dx0"] + unmerge(d["dy"])))

