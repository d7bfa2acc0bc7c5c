"""The softmax-loss kernels (bcnn_amd/csrc/softmax_loss.hip) at operator level, on every dispatch branch, against the
float64 restatement tests/_softmax_loss_ref.py (pinned to torch by tests/test_softmax_loss_ref_pinning.py).

Logits: tests/_next_ref.softmax_inputs (uniform rows, all-equal rows, a +60 spike, +-1e4 offsets, the maximum last / at
channel 64). Label patterns cycle over the cases: all valid, every pixel ignored (V = 0), ignore runs that straddle wave
and workgroup boundaries, one class only, out-of-range values (C, -1, ignore_label - 1, 1.5, +-inf, NaN, 3e9) and
ignore_label = -1 with -1 in the map; the all-equal rows get label 0 and must count as correct (the first maximum wins).
The normaliser and the scale cycle too. Every output lives inside a buffer of 7.0 whose margins must keep their bits.

Bounds, with B = tests/_next_ref.softmax_bound(x) (relative for p, absolute for x - lse), D the denominator, g = scale / D:
    p     check_softmax: |p - p64| <= B * p64 per element, |sum_c p - 1| <= C * max_c B per pixel
    loss  |loss - loss64| <= sum over valid pixels of B[b, t, i] / D + 2^-24 * |loss64|
    dx    |dx - dx64| <= g * (B * p64 + 2^-23 * |p64 - y|) + 2^-24 * |dx64| on valid pixels: the kernel computes
          fl(gf * fl(p - y)) with gf = fl(scale / D), one rounding each for the subtraction, the product and the stored
          factor, on a p that is within B * p64. Pixels that are not valid: +0.0 bit for bit in the overwrite form; in the
          add form they keep the bits of dx0 and the bound of the others widens by 2^-24 * |dx0 + dx64|.
    counts (valid, ignored, out_of_range, correct) and the confusion matrix are exact; its trace is `correct`, its total
    `valid`. A second run gives the same bits everywhere, record included.

Each case asserts the kernels the dispatch trace names; the table below writes them out."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _next_ref as N
from tests import _softmax_loss_ref as R

gpu = pytest.mark.gpu
DEV = "cuda:0"
BAND = 64        # floats of 7.0 on both sides of every output (a multiple of 4: views keep their alignment)
C_REG = 32       # bcnn_hip_softmax_loss_c_reg(), asserted below

ROWS = "softmax_loss_fwd_rows"
REG, REG_V4 = "softmax_loss_fwd_pixels_reg", "softmax_loss_fwd_pixels_reg:v4"
STREAM, STREAM_V4 = "softmax_loss_fwd_pixels_stream", "softmax_loss_fwd_pixels_stream:v4"
FINAL = "softmax_loss_finalize"
BWD, BWD_V4 = "softmax_loss_bwd", "softmax_loss_bwd:v4"
CONF_LDS, CONF = "softmax_loss_confusion:lds", "softmax_loss_confusion"

# the forward kernel of a pixel case: by class count (registers up to C_REG, streaming past it) and by HW (16-byte form
# when HW % 4 == 0 and everything is aligned)
PIXEL_C = {1: (REG, REG_V4), 2: (REG, REG_V4), 5: (REG, REG_V4), 21: (REG, REG_V4), 32: (REG, REG_V4),
           33: (STREAM, STREAM_V4), 150: (STREAM, STREAM_V4)}
PIXEL_HW = {2: 0, 5: 0, 49: 0, 63: 0, 64: 1, 65: 0, 259: 0, 260: 1}   # 1: the 16-byte form
PIXEL_CASES = [(2, C, HW, PIXEL_C[C][PIXEL_HW[HW]], (BWD, BWD_V4)[PIXEL_HW[HW]]) for C in PIXEL_C for HW in PIXEL_HW]
ROW_CASES = [(n, C, 1, ROWS, BWD) for C in (1, 2, 63, 64, 65, 130, 1000) for n in (1, 3)]
ROW_CASES.append((8200, 3, 1, ROWS, BWD))   # more rows than the capped grid has waves (2048 workgroups x 4)
# pixel counts past the grid cap of 2048 x 256 lanes, so the grid-stride loops turn over: 570 000 pixels in the scalar form
# (the label starts 4 bytes off), 525 000 four-pixel items in the 16-byte form; the aligned 190 000 runs one pass of :v4
BIG_CASES = [(3, 2, 190000, REG_V4, BWD_V4, ()), (3, 2, 190000, REG, BWD, ("label",)), (3, 2, 700000, REG_V4, BWD_V4, ())]
NORMS = [R.NORM_VALID_PER_IMAGE, R.NORM_VALID, R.NORM_NONE]
SCALES = [1.0, 0.5, 3.0]


def _id(case):
    return "n%d_c%d_hw%d" % case[:3]


def _trace_start():
    from bcnn_amd import _lib
    _lib.load().bcnn_hip_trace_enable(1)


def _trace_stop():
    from bcnn_amd import _lib
    L = _lib.load()
    n = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return buf.value.decode().split()


class _Guarded:
    """a device tensor of `shape` inside a buffer of 7.0, starting `off` floats past a 16-byte boundary"""

    def __init__(self, shape, off=0, values=None, dtype=torch.float32):
        numel = int(np.prod(shape))
        self.buf = torch.full((numel + 2 * BAND + off,), 7.0, dtype=torch.float32, device=DEV)
        self.lo, self.hi = BAND + off, BAND + off + numel
        self.t = self.buf[self.lo:self.hi].view(shape)
        assert self.t.data_ptr() % 16 == 4 * off
        if values is not None:
            self.t.copy_(torch.tensor(np.asarray(values), dtype=torch.float32))

    def margins_intact(self):
        seven = np.float32(7.0).view(np.int32)
        edge = torch.cat([self.buf[:self.lo], self.buf[self.hi:]]).cpu().numpy().view(np.int32)
        return bool((edge == seven).all())


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(n, C, HW, k):
    """inputs and float64 results of case number k (k selects the label pattern, the normaliser and the scale)"""
    x = N.softmax_inputs(n, C, HW, seed=1000 + 7 * C + HW + n)
    pattern = R.PATTERNS[k % len(R.PATTERNS)]
    lab, ignore = R.labels(pattern, n, C, HW, seed=k + C, x=x)
    norm, scale = NORMS[k % len(NORMS)], SCALES[(k // 2) % len(SCALES)]
    ref = R.reference(x, lab, ignore, norm, scale)
    dx0 = np.random.RandomState(k).uniform(-1, 1, x.shape).astype(np.float32)
    for a in (x, lab, dx0):
        a.setflags(write=False)
    return dict(x=x, lab=lab, ignore=ignore, norm=norm, scale=scale, ref=ref, dx0=dx0, bound=N.softmax_bound(x),
                pattern=pattern)


def _run(case, fwd, bwd, off=()):
    """forward, both backward forms and the confusion matrix; returns host copies and asserts trace and margins"""
    from bcnn_amd import ops
    o = lambda name: 1 if name in off else 0
    x, lab = case["x"], case["lab"]
    n, C, HW = x.shape
    kw = dict(ignore_label=case["ignore"], normalize=case["norm"], scale=case["scale"])
    xd = _Guarded(x.shape, o("x"), x)
    ld = _Guarded((n, 1, HW), o("label"), lab.reshape(n, 1, HW))
    pd = _Guarded(x.shape, o("p"))
    over = _Guarded(x.shape, o("dx"))
    add = _Guarded(x.shape, o("dx"), case["dx0"])
    rec = ops.softmax_loss_record()
    _trace_start()
    ops.softmax_loss_forward(xd.t, ld.t, pd.t, rec, **kw)
    ops.softmax_loss_backward(pd.t, ld.t, rec, over.t, overwrite=True, **kw)
    ops.softmax_loss_backward(pd.t, ld.t, rec, add.t, overwrite=False, **kw)
    conf = ops.softmax_loss_confusion(pd.t, ld.t, ignore_label=case["ignore"])
    torch.cuda.synchronize()
    names = _trace_stop()
    assert names == [fwd, FINAL, bwd + ":overwrite", bwd, CONF_LDS if C <= 64 else CONF], names
    for g in (xd, ld, pd, over, add):
        assert g.margins_intact()
    assert np.array_equal(_bits(xd.t.cpu().numpy()), _bits(x)) and np.array_equal(_bits(ld.t.cpu().numpy().reshape(n, HW)), _bits(lab))
    return dict(p=pd.t.cpu().numpy(), over=over.t.cpu().numpy(), add=add.t.cpu().numpy(), conf=conf,
                rec=ops.softmax_loss_read_record(rec), rec_bits=rec.cpu().numpy().copy())


def _check(n, C, HW, k, fwd, bwd, off=()):
    case = _reference(n, C, HW, k)
    ref, x, B = case["ref"], case["x"], case["bound"]
    got = _run(case, fwd, bwd, off)
    tag = "n%d c%d hw%d %s norm %d scale %g off %s" % (n, C, HW, case["pattern"], case["norm"], case["scale"], off)
    worst = N.check_softmax(got["p"], x, tag)
    # counts and the confusion matrix: exact
    rec = got["rec"]
    for name in ("valid", "ignored", "out_of_range", "correct"):
        assert rec[name] == ref[name], (tag, name, rec[name], ref[name])
    assert np.array_equal(got["conf"], ref["confusion"]), tag
    assert got["conf"].trace() == rec["correct"] and got["conf"].sum() == rec["valid"]
    if case["pattern"] == "all_ignored":
        assert rec["valid"] == 0 and rec["loss"] == 0.0
    if case["pattern"] == "out_of_range":
        assert rec["out_of_range"] > 0
    if case["pattern"] == "minus_one_no_ignore":
        assert rec["ignored"] == 0 and rec["out_of_range"] > 0
    # the all-equal rows have label 0 where they are valid, and count as correct: the first maximum wins
    equal = np.all(x == x[:, :1, :], axis=1) & (ref["kind"] == R.VALID)
    assert np.array_equal(ref["arg"][equal], np.zeros(int(equal.sum()), np.int64))
    # loss
    D, g = ref["D"], float(np.float32(case["scale"])) / ref["D"]
    valid = ref["kind"] == R.VALID
    safe = np.where(valid, ref["cls"], 0)
    Bt = np.take_along_axis(B, safe[:, None, :], axis=1)[:, 0, :]
    loss_bound = float(np.where(valid, Bt, 0.0).sum()) / D + 2.0 ** -24 * abs(ref["loss"])
    loss_err = abs(float(rec["loss"]) - ref["loss"])
    assert abs(float(rec["grad_factor"]) - g) <= 2.0 ** -24 * g, tag
    # gradient
    v3 = np.broadcast_to(valid[:, None, :], x.shape)
    dx64, p64 = ref["dx"], ref["p"]
    gbound = g * (B * p64 + 2.0 ** -23 * np.abs(p64 - ref["onehot"])) + 2.0 ** -24 * np.abs(dx64)
    err_over = np.abs(got["over"].astype(np.float64) - dx64)
    dx0 = case["dx0"].astype(np.float64)
    err_add = np.abs(got["add"].astype(np.float64) - (dx0 + dx64))
    abound = gbound + 2.0 ** -24 * np.abs(dx0 + dx64)
    print("%s: p %.3f of its bound, loss err %.3e (bound %.3e), dx %.3f / %.3f of the bounds" % (
        tag, worst, loss_err, loss_bound, float((err_over[v3] / gbound[v3]).max()) if v3.any() else 0.0,
        float((err_add[v3] / abound[v3]).max()) if v3.any() else 0.0))
    assert loss_err <= loss_bound, (tag, rec["loss"], ref["loss"], loss_bound)
    assert bool((err_over[v3] <= gbound[v3]).all()), tag
    assert bool((err_add[v3] <= abound[v3]).all()), tag
    assert bool((_bits(got["over"])[~v3] == 0).all()), tag                               # +0.0
    assert np.array_equal(_bits(got["add"])[~v3], _bits(case["dx0"])[~v3]), tag           # untouched, bit for bit
    # the same bits on a second run, record included
    again = _run(case, fwd, bwd, off)
    for name in ("p", "over", "add", "rec_bits"):
        assert np.array_equal(_bits(got[name]) if name != "rec_bits" else got[name],
                              _bits(again[name]) if name != "rec_bits" else again[name]), (tag, name)
    assert np.array_equal(got["conf"], again["conf"])


@gpu
def test_c_reg_is_what_the_tables_assume():
    from bcnn_amd import ops
    assert ops.softmax_loss_c_reg() == C_REG >= 21


@gpu
@pytest.mark.parametrize("k,case", list(enumerate(ROW_CASES)), ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_rows(k, case):
    n, C, HW, fwd, bwd = case
    _check(n, C, HW, k, fwd, bwd)


@gpu
@pytest.mark.parametrize("k,case", list(enumerate(PIXEL_CASES)), ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_pixels(k, case):
    n, C, HW, fwd, bwd = case
    _check(n, C, HW, k, fwd, bwd)


@gpu
@pytest.mark.parametrize("k,C", list(enumerate(PIXEL_C)))
@pytest.mark.parametrize("HW", [64, 260])
def test_pixels_unaligned_tensors_take_the_scalar_form(k, C, HW):
    """x, p or the label 4 bytes past a 16-byte boundary: the forward leaves the 16-byte form; the backward leaves it for
    p, dx or the label (x is no operand of it)"""
    scalar_fwd = PIXEL_C[C][0]
    for j, (off, fwd, bwd) in enumerate([(("x",), scalar_fwd, BWD_V4), (("p",), scalar_fwd, BWD), (("label",), scalar_fwd, BWD),
                                         (("dx",), PIXEL_C[C][1], BWD)]):
        _check(2, C, HW, 3 * k + j, fwd, bwd, off)


@gpu
@pytest.mark.parametrize("k,case", list(enumerate(BIG_CASES)), ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_pixels_past_the_grid_cap(k, case):
    n, C, HW, fwd, bwd, off = case
    _check(n, C, HW, 2 * k + 2, fwd, bwd, off)   # ignore runs, all valid, out of range


@gpu
def test_forward_without_a_label_writes_the_probabilities_only():
    from bcnn_amd import ops
    for n, C, HW, fwd in ((3, 10, 1, ROWS), (2, 21, 260, REG_V4), (2, 21, 65, REG), (2, 150, 64, STREAM_V4), (2, 33, 5, STREAM)):
        case = _reference(n, C, HW, 0)
        xd, pd, p2 = _Guarded(case["x"].shape, 0, case["x"]), _Guarded(case["x"].shape), _Guarded(case["x"].shape)
        ld = _Guarded((n, 1, HW), 0, case["lab"].reshape(n, 1, HW))
        rec = ops.softmax_loss_record()
        _trace_start()
        ops.softmax_loss_forward(xd.t, None, pd.t, None)
        ops.softmax_loss_forward(xd.t, ld.t, p2.t, rec, ignore_label=case["ignore"])
        torch.cuda.synchronize()
        assert _trace_stop() == [fwd, fwd, FINAL]
        assert pd.margins_intact() and p2.margins_intact()
        N.check_softmax(pd.t.cpu().numpy(), case["x"], "no label")
        assert np.array_equal(_bits(pd.t.cpu().numpy()), _bits(p2.t.cpu().numpy()))   # the label does not touch p
