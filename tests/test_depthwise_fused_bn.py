"""The fused depthwise entry points of the MobileNet block -- bcnn_hip_depthwise_forward_bnin, _backward_bn, _backward_bnin,
_backward_bn_bnin, _backward_bnin_sums (and the statistics of _forward_stats through _forward_bnin) -- against an independent
statement of what they compute: tests/_dw_fused_ref.py, a composition of the pinned batch-norm / activation restatements and
the C oracle's depthwise layer (tests/test_dw_fused_ref_pinning.py holds it on the CPU). "bn": the backward of a batch-norm
node behind the layer is applied to the incoming gradient; "bnin": the producer's batch-norm and activation are applied to the
input on load.

Every tensor is a view inside a larger allocation with sentinel bands (_next_ref.Guarded); every case asserts the bands, that
the inputs are unchanged, the kernel the dispatch trace names, y / the written-back dy / dx equal BY VALUE to the float32
composition (the kernels promise the reference's tap order with separate multiply and add and a correctly rounded division;
bits are not compared because bn_math.h documents -0 / d = +0), dw / db / statistics / producer sums within a forward-error
bound of the float64 sums, bit-identical reruns, and what the size queries and too-small buffers promise.

The sums' bound is (k + 2) 2^-24 sum |terms| per channel (_dw_fused_ref.sum_bound), k = the terms one partial's float32 chain
adds. A slot is one band of one image's plane, bands are even cuts of the rows in both families (dwm_plan: len = ceil(OH /
BPP); dwl_plan: BR = ceil(OH / NB)) and `splits` = N * bands is what a call returns, so k = ceil(OH / (splits / N)) * OW
outputs for the statistics, dw and db, and min(H, stride * those rows) * W inputs for the producer sums. The backward entries
without sums return no count: forward and backward of a family cut the planes by one plan, so the forward's count on the same
tensors is used (the sums entry, where it emits, is asserted to return the same).

Shapes (n, c, h, w, stride) and the branch each reaches. Marching family (depthwise_march.hip, dwm_plan: lanes of V = 4 / 2 / 1
columns by W % 4 / W % 2, L = W / V <= 64 lanes per row, G = 64 / L bands per wave, 7 rows per band -- 14 for stride-1 planes of
56 rows and more -- evened out; stride 2 needs an even W):
  (2,5,9,12,1)   V 4, L 3, 21 bands per wave, 2 bands per plane of 5 + 4 rows (even wave down, odd wave up)
  (2,5,9,12,2)   V 4, one band of 5 output rows, 8-byte y accesses
  (2,3,17,10,1)  V 2, L 5, 3 bands per plane of 6 + 6 + 5 rows: two march down, one up, last band ragged
  (2,3,17,10,2)  V 2, 2 bands of 5 + 4 output rows, 4-byte y accesses
  (3,5,15,7,1)   V 1, L 7, 3 bands of 5
  (1,2,57,8,1)   the 14-row plan: 5 bands of 12, last of 9
  (1,2,8,256,1)  L 64: a row fills the wave, one band per wave, 2 bands of 4
  (2,3,1,1,1)    single pixel, 6 of 64 lane groups at work
LDS family (depthwise_lds.hip, dwl_plan: planes above 4096 floats are cut into row bands, planes below 1024 floats go several
per tile, a multiple of 4 sized by their padded image); the marching family refuses each: odd W at stride 2, or L > 64:
  (2,11,9,13,2)  20 planes per tile, 22 planes: second tile ragged; stride 2: the g image (1376 floats) is enlarged to hold a dx
                 piece (2340) for the producer sums
  (1,2,3,130,2)  4 planes per tile, 2 present; W % 4 == 2 with L = 65; stride 2 with sums, g image 1176 < dx piece 1560: its
                 pairs (LRELU, NONE) and (ABS, RELU) emit and compare S1 / S2 on the half-empty enlarged tile
  (1,2,20,67,1)  odd W > 64, one whole plane per workgroup
  (1,3,33,35,2)  one whole plane per workgroup, stride 2
  (1,2,65,67,1)  bands of 33 + 32 rows that read each other's halo rows
  (1,2,65,67,2)  bands of 17 + 16 output rows
  (1,2,4,260,1)  W > 256
  (2,3,2,3,2)    tiny planes, 168 per tile
  (2,5,9,12,1) with raw / x and dx one float off a 16-byte boundary: the marching family refuses misaligned tensors, the LDS
                 family takes the shape with per-element scatter and copy-out
Branches and a case that reaches each (all asserted through the trace):
  dwm_fwd_kernel:bnin / dwl_fwd_kernel:bnin, both strides, non-ReLU pairs (the generic instantiation, relu == false): every shape
  dw{m,l}_bwd_kernel:bnin, :bn+bnin, :bn at both strides with non-ReLU pairs: every shape; the ReLU instantiation: the
    (RELU, RELU) pairs of PAIRS (both families, both strides)
  the producer sums emitted and compared: the first pair of EVERY shape (producer NONE or RELU), so also on each stride-2 LDS
    shape: (2,11,9,13,2) and (1,2,3,130,2) enlarged g image, (1,3,33,35,2) whole plane, (1,2,65,67,2) bands, (2,3,2,3,2) 168 planes
  the derivative pre-pass with `in` (leaky ReLU written back: the fused kernel then runs with no activation): (LRELU, .) pairs
  backward_bn with tanh / logistic (cheap backward, not cheap forward): test_backward_behind_a_batchnorm_node, acts by shape
  the bn_one quirks on the input path (scale 0 / 1, bias 0 / 1) and bn_bwd_one's (scale 0 / 1): _dw_fused_ref.make_case channels
  forward_bnin with a statistics buffer; buffers one float short; the sums entry accumulating and with a leaky producer
No comparison of y, dy or dx needed anything but equality: tanh's 1 - y * y and logistic's (1 - y) * y too are a separate
multiply and subtract on both sides.
What the assertions can and cannot see (reference perturbed, kernels unchanged): the two eps swapped, the bias-1 quirk dropped
and a tap moved fail `y` / `dx`; the producer's derivative left out of S2 fails `S1, S2`. Multiplying by a scale of 1, and by a
scale of 0 while everything is finite, gives the same VALUES as the quirks' selects, and a derivative of 0 or 1 -- the only
kind the sums are emitted for -- applied twice is applied once: those variations are the same function, nothing to catch."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _dw_fused_ref as D
from tests import _next_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, TANH, RELU, LRELU, ABS, CLAMP, LOGISTIC = (R.ACT_NONE, R.ACT_TANH, R.ACT_RELU, R.ACT_LRELU, R.ACT_ABS, R.ACT_CLAMP,
                                                 R.ACT_LOGISTIC)

SHIFTED = ((2, 5, 9, 12, 1), "dwl")
ALL = [(sh, fam, 0) for sh, fam in D.SHAPES] + [SHIFTED + (1,)]
# (layer activation, producer activation) per shape, written out. The FIRST pair of every shape has a producer whose derivative
# is 0 or 1 (NONE, RELU), so every shape -- each stride-2 LDS shape with its enlarged or half-empty tile among them -- emits the
# producer's sums and has them compared at least once; a LATER pair has a leaky producer (the sums entry returns 0) or is
# (RELU, RELU), the compiled-in ReLU instantiation. Shapes with c < 5 run their later pairs without quirk channels
# (_dw_fused_ref.make_case): every vector random.
PAIRS = {
    ((2, 5, 9, 12, 1), 0): [(LRELU, NONE), (RELU, RELU), (NONE, LRELU)],
    ((2, 5, 9, 12, 2), 0): [(CLAMP, RELU), (NONE, LRELU)],
    ((2, 3, 17, 10, 1), 0): [(RELU, NONE), (ABS, LRELU)],
    ((2, 3, 17, 10, 2), 0): [(NONE, RELU), (RELU, RELU), (LRELU, LRELU)],
    ((3, 5, 15, 7, 1), 0): [(ABS, NONE), (CLAMP, LRELU)],
    ((1, 2, 57, 8, 1), 0): [(LRELU, RELU), (NONE, LRELU)],
    ((1, 2, 8, 256, 1), 0): [(CLAMP, NONE), (RELU, LRELU)],
    ((2, 3, 1, 1, 1), 0): [(NONE, RELU), (ABS, LRELU)],
    ((2, 11, 9, 13, 2), 0): [(CLAMP, RELU), (RELU, RELU), (NONE, LRELU)],
    ((1, 2, 3, 130, 2), 0): [(LRELU, NONE), (ABS, RELU), (ABS, LRELU)],
    ((1, 2, 20, 67, 1), 0): [(RELU, NONE), (CLAMP, LRELU)],
    ((1, 3, 33, 35, 2), 0): [(NONE, RELU), (LRELU, LRELU)],
    ((1, 2, 65, 67, 1), 0): [(LRELU, NONE), (RELU, RELU), (NONE, LRELU)],
    ((1, 2, 65, 67, 2), 0): [(ABS, RELU), (LRELU, NONE), (NONE, LRELU)],
    ((1, 2, 4, 260, 1), 0): [(CLAMP, RELU), (RELU, LRELU)],
    ((2, 3, 2, 3, 2), 0): [(LRELU, NONE), (NONE, RELU), (ABS, LRELU)],
    ((2, 5, 9, 12, 1), 1): [(NONE, RELU), (LRELU, LRELU)],
}
assert set(PAIRS) == {(sh, shift) for sh, _, shift in ALL} and all(pr[0][1] in (NONE, RELU) for pr in PAIRS.values())
# (shape, family, shift, pair, quirk channels)
IN_CASES = [(sh, fam, shift, pair, i == 0 or sh[1] >= 5) for sh, fam, shift in ALL for i, pair in enumerate(PAIRS[(sh, shift)])]
BN_ACTS = [TANH, LOGISTIC, LRELU, NONE, CLAMP, ABS, RELU]
BN_CASES = [(sh, fam, shift, BN_ACTS[i % len(BN_ACTS)], True) for i, (sh, fam, shift) in enumerate(ALL)]
BN_CASES += [((2, 3, 17, 10, 2), "dwm", 0, TANH, False), ((1, 2, 65, 67, 1), "dwl", 0, LOGISTIC, False),
             ((2, 11, 9, 13, 2), "dwl", 0, TANH, True), ((1, 2, 65, 67, 2), "dwl", 0, LRELU, False),
             ((1, 2, 57, 8, 1), "dwm", 0, CLAMP, False)]


def _id(sh, fam, shift, acts, quirks):
    acts = acts if isinstance(acts, tuple) else (acts,)
    return ("n%d_c%d_%dx%d_s%d_" % sh + fam + ("_shift" if shift else "") + "".join("_" + R.ACT_NAMES[a] for a in acts) +
            ("" if quirks else "_random"))


def _lib():
    from bcnn_amd import _lib as lib
    return lib.load()


def _traced(fn):
    """(fn(), the kernels the dispatch named meanwhile)"""
    L = _lib()
    L.bcnn_hip_trace_enable(1)
    try:
        r = fn()
        n = L.bcnn_hip_trace_read(None, 0)
        buf = ctypes.create_string_buffer(n + 1)
        L.bcnn_hip_trace_read(buf, n + 1)
    finally:
        L.bcnn_hip_trace_enable(0)
    L.bcnn_hip_sync()
    return r, buf.value.decode().split()


# ---- the reference of a case, computed once and shared (read-only) -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(shape, act, in_act, quirks=True):
    p = D.make_case(*shape, act=act, in_act=in_act, seed=sum(shape) + 10 * act + in_act, quirks=quirks)
    p.xin = D.case_input32(p)
    p.y, p.stats, p.stats_mag = D.forward(p, p.xin)
    p.bwd = {}
    for bn in (False, True):
        for ow in (0, 1):
            o = D.backward(p, p.xin, bn, bool(ow))                      # g, dx: float32, the oracle's order
            w64 = D.grads64(p.xin, o["g"], p.wt, p.s, np.zeros_like(p.dx0) if ow else p.dx0, p.dw0, p.db0)
            o.update({k: w64[k] for k in ("dw", "dw_mag", "db", "db_mag")})   # dw, db: float64
            o["sums"], o["sums_mag"] = D.in_sums64(o["dx"], p.xin, p.raw, p.in_mean, p.in_act)
            p.bwd[(bn, ow)] = o
    for v in vars(p).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


class _Inputs:
    """the tensors no call may write, uploaded once per case"""

    def __init__(self, p, shift):
        G = R.Guarded
        self.t = dict(raw=G(p.raw, shift), xin=G(p.xin, shift), wt=G(p.wt), bias=G(p.bias), y=G(p.y), dz=G(p.dz),
                      in_mean=G(p.in_mean), in_var=G(p.in_var), in_scale=G(p.in_scale), in_bias=G(p.in_bias),
                      bn_mean=G(p.bn_mean), bn_var=G(p.bn_var), bn_scale=G(p.bn_scale), bn_dmean=G(p.bn_dmean),
                      bn_dvar=G(p.bn_dvar))

    def ptr(self, *names):
        return [self.t[k].ptr for k in names]

    def assert_unchanged(self):
        for k, g in self.t.items():
            g.assert_unchanged(k)


IN_VECS = ("in_mean", "in_var", "in_scale", "in_bias")
BN_VECS = ("bn_mean", "bn_var", "bn_scale", "bn_dmean", "bn_dvar")


def _nan(count):
    return R.Guarded(np.full(count, np.nan, F32))


def _slots(buf, c, splits):
    """float64 [C][2] sums over the `splits` slots of a [(channel * splits + i) * 2 + {0, 1}] buffer; what lies behind stays NaN"""
    v = buf.read()
    used = c * splits * 2
    assert np.isfinite(v[:used]).all() and np.isnan(v[used:]).all()
    return v[:used].astype(F64).reshape(c, splits, 2).sum(axis=1), v[:used].copy()


def _within(tag, got, want, bound):
    ratio = np.abs(np.asarray(got, F64) - want) / np.maximum(bound, 1e-300)
    print("%s: worst error %.3g x its bound" % (tag, ratio.max()))
    assert np.isfinite(np.asarray(got, F64)).all() and ratio.max() <= 1.0, (
        "%s: %.3g x its bound at %s" % (tag, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape)))


def _rows(p, splits):
    bands = splits // p.n
    assert bands * p.n == splits and bands >= 1
    return -(-p.oh // bands)


def _equal(tag, got, want):
    """by value: -0.0 == 0.0 (bn_math.h: -0 / d gives +0), everything else bit for bit"""
    got = np.asarray(got, F32).reshape(np.shape(want))
    bad = np.flatnonzero((got != want).ravel())
    assert bad.size == 0, "%s: %d of %d values differ, first at %d: got %r want %r" % (
        tag, bad.size, got.size, bad[0], got.ravel()[bad[0]], np.asarray(want).ravel()[bad[0]])


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def _forward_bnin(p, inp, stats_floats):
    L = _lib()
    y = _nan(p.y.size)
    stats = _nan(stats_floats) if stats_floats else None
    splits, trace = _traced(lambda: L.bcnn_hip_depthwise_forward_bnin(
        *inp.ptr("raw", "wt", "bias"), y.ptr, p.n, p.c, p.h, p.w, 3, p.s, 1, p.act, stats.ptr if stats else 0, stats_floats,
        *inp.ptr(*IN_VECS), p.in_act))
    return splits, y, stats, trace


def _backward(p, inp, entry, overwrite, shift, sums_floats=0, x="raw"):
    """entry: bn (no `in`, x is the layer's input itself), bnin, bn_bnin, sums, sums_bn. Returns what the call left."""
    L = _lib()
    bn = entry in ("bn", "bn_bnin", "sums_bn")
    dy = inp.t["dz"] if bn else R.Guarded(p.dz)
    dx, dw, db = R.Guarded(p.dx0, shift), R.Guarded(p.dw0), R.Guarded(p.db0)
    sums = _nan(sums_floats) if sums_floats else None
    head = inp.ptr(x, "wt", "y") + [dy.ptr, dx.ptr, dw.ptr, db.ptr, p.n, p.c, p.h, p.w, 3, p.s, 1, p.act, overwrite]
    if entry == "bn":
        call = lambda: L.bcnn_hip_depthwise_backward_bn(*head, *inp.ptr(*BN_VECS))
    elif entry == "bnin":
        call = lambda: L.bcnn_hip_depthwise_backward_bnin(*head, *inp.ptr(*IN_VECS), p.in_act)
    elif entry == "bn_bnin":
        call = lambda: L.bcnn_hip_depthwise_backward_bn_bnin(*head, *inp.ptr(*BN_VECS), *inp.ptr(*IN_VECS), p.in_act)
    else:
        bnp = inp.ptr(*BN_VECS) if bn else [0] * 5
        call = lambda: L.bcnn_hip_depthwise_backward_bnin_sums(*head, *bnp, *inp.ptr(*IN_VECS), p.in_act,
                                                               sums.ptr if sums else 0, sums_floats)
    ret, trace = _traced(call)
    return dict(ret=ret, trace=trace, dy=dy.read(), dx=dx.read(), dw=dw.read(), db=db.read(), sums=sums)


def _forward_splits(p, inp, fam, x):
    """The split count of the family that takes this call, from the plain forward with statistics on the same tensors (no
    activation: the count is the plan's, N * bands, and the backward kernels of a family cut the planes by the same plan)"""
    L = _lib()
    y, stats = _nan(p.y.size), _nan(L.bcnn_hip_depthwise_stats_size(p.n, p.c, p.h, p.w, 3, p.s, 1))
    splits, trace = _traced(lambda: L.bcnn_hip_depthwise_forward_stats(*inp.ptr(x, "wt", "bias"), y.ptr, p.n, p.c, p.h, p.w, 3,
                                                                       p.s, 1, NONE, stats.ptr, stats.n))
    assert trace == [fam + "_fwd_kernel"] and splits > 0, (trace, splits)
    return splits


def _check_backward(tag, p, got, bn, overwrite, fam, suffix, splits):
    """`splits`: N * bands of the family `fam` on this shape; one partial of dw / db adds a band's outputs"""
    want = p.bwd[(bn, overwrite)]
    assert got["trace"] == ["%s_bwd_kernel:%s" % (fam, suffix)], (tag, got["trace"])
    if bn:
        R.assert_bits(tag + " dz", got["dy"], p.dz)                 # neither dz nor the layer's output gradient is written
    else:
        _equal(tag + " dy", got["dy"], want["g"])                   # g = dy * act'(y) written back
    _equal(tag + " dx", got["dx"], want["dx"])
    k = _rows(p, splits) * p.ow
    _within(tag + " dw", got["dw"], want["dw"], D.sum_bound(k, want["dw_mag"]))
    _within(tag + " db", got["db"], want["db"], D.sum_bound(k, want["db_mag"]))


def _same_bits(tag, a, b, keys=("dx", "dw", "db", "dy")):
    for k in keys:
        R.assert_bits("%s %s" % (tag, k), a[k], b[k])


# ---- the layer behind a batch-normalised producer -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,fam,shift,pair,quirks", IN_CASES, ids=[_id(*c) for c in IN_CASES])
def test_input_normalised_on_load(shape, fam, shift, pair, quirks):
    L = _lib()
    n, c, h, w, s = shape
    act, in_act = pair
    assert L.bcnn_hip_depthwise_bnin_fusable(n, c, h, w, 3, s, 1, act, in_act)
    assert L.bcnn_hip_depthwise_bn_fusable(n, c, h, w, 3, s, 1, act)
    p = _reference(shape, act, in_act, quirks)
    inp = _Inputs(p, shift)

    # forward, with the statistics a batch-norm node behind the layer starts from
    size = L.bcnn_hip_depthwise_stats_size(n, c, h, w, 3, s, 1)
    splits, y, stats, trace = _forward_bnin(p, inp, size)
    assert trace == [fam + "_fwd_kernel:bnin"], trace
    assert splits > 0 and size >= c * splits * 2, (splits, size)
    _equal("y", y.read(), p.y)
    st, raw_stats = _slots(stats, c, splits)
    _within("statistics", st, p.stats, D.sum_bound(_rows(p, splits) * p.ow, p.stats_mag))
    splits2, y2, stats2, _ = _forward_bnin(p, inp, size)
    assert splits2 == splits
    R.assert_bits("y again", y2.read(), y.read())
    R.assert_bits("statistics again", _slots(stats2, c, splits)[1], raw_stats)
    short = c * splits * 2 - 1                                   # one float short: no statistics, nothing written, y all the same
    splits3, y3, stats3, trace3 = _forward_bnin(p, inp, short)
    assert splits3 == 0 and trace3 == trace and np.isnan(stats3.read()).all()
    _equal("y without statistics", y3.read(), p.y)
    assert _forward_bnin(p, inp, 0)[0] == 0

    # backward: the three entries and the one that also leaves the producer's sums
    need = L.bcnn_hip_depthwise_insums_size(n, c, h, w, 3, s, 1)
    wanted = in_act in (NONE, RELU)                              # dw_in_sums_wanted: a derivative of 0 or 1
    for ow in (0, 1):
        plain = _backward(p, inp, "bnin", ow, shift)
        _check_backward("bnin ow%d" % ow, p, plain, False, ow, fam, "bnin", splits)
        both = _backward(p, inp, "bn_bnin", ow, shift)
        _check_backward("bn+bnin ow%d" % ow, p, both, True, ow, fam, "bn+bnin", splits)
        for entry, other, bn, suffix in (("sums", plain, False, "bnin"), ("sums_bn", both, True, "bn+bnin")):
            got = _backward(p, inp, entry, ow, shift, need)
            tag = "%s ow%d" % (entry, ow)
            assert got["trace"] == ["%s_bwd_kernel:%s" % (fam, suffix)], (tag, got["trace"])
            _same_bits(tag + " against the entry without sums", got, other)
            if ow and wanted:
                sp = got["ret"]
                assert sp == splits and need >= c * sp * 2, (tag, sp, splits, need)   # one plan, forward and backward
                sums, raw_sums = _slots(got["sums"], c, sp)
                ref = p.bwd[(bn, 1)]
                k = min(p.h, p.s * _rows(p, sp)) * p.w
                _within(tag + " S1, S2", sums, ref["sums"], D.sum_bound(k, ref["sums_mag"]))
                again = _backward(p, inp, entry, ow, shift, need)
                assert again["ret"] == sp
                R.assert_bits(tag + " sums again", _slots(again["sums"], c, sp)[1], raw_sums)
                _same_bits(tag + " again", again, got)
                if not bn:
                    few = _backward(p, inp, entry, ow, shift, c * sp * 2 - 1)
                    assert few["ret"] == 0 and np.isnan(few["sums"].read()).all(), tag
                    _same_bits(tag + " with a short buffer", few, other)
            else:  # dx accumulates, or the producer's derivative is not 0 or 1: no sums, the buffer is left alone
                assert got["ret"] == 0 and np.isnan(got["sums"].read()).all(), tag
    inp.assert_unchanged()


# ---- the layer in front of a batch-norm node, its input given as it is ------------------------------------------------------------
@pytest.mark.parametrize("shape,fam,shift,act,quirks", BN_CASES, ids=[_id(*c) for c in BN_CASES])
def test_backward_behind_a_batchnorm_node(shape, fam, shift, act, quirks):
    L = _lib()
    n, c, h, w, s = shape
    assert L.bcnn_hip_depthwise_bn_fusable(n, c, h, w, 3, s, 1, act)
    p = _reference(shape, act, RELU, quirks)
    inp = _Inputs(p, shift)
    splits = _forward_splits(p, inp, fam, "xin")
    for ow in (0, 1):
        got = _backward(p, inp, "bn", ow, shift, x="xin")
        _check_backward("bn ow%d" % ow, p, got, True, ow, fam, "bn", splits)
        again = _backward(p, inp, "bn", ow, shift, x="xin")
        _same_bits("bn ow%d again" % ow, again, got)
    inp.assert_unchanged()


# ---- what the predicates promise ------------------------------------------------------------------------------------------------
PAIR_SHAPES = [(4, 8, 112, 112, 1), (4, 8, 112, 112, 2), (3, 6, 56, 56, 1), (5, 7, 28, 28, 2), (6, 37, 14, 14, 1),
               (6, 37, 14, 14, 2), (8, 50, 7, 7, 1), (2, 3, 33, 35, 1), (2, 5, 9, 13, 2), (300, 100, 7, 7, 1)]   # test_depthwise_lds
INSUMS = [(3, 40, 7, 7, 1), (2, 36, 14, 14, 1), (2, 18, 28, 28, 2), (1, 6, 112, 112, 1), (2, 5, 112, 112, 2), (3, 10, 9, 9, 1),
          (2, 3, 56, 56, 1)]                                                                                      # test_dw_insums
# H = 2 at stride 1: below 1024 floats a tile holds at least four padded planes, and from W = 476 the backward workgroup's two
# images of 4 * 3 + 5 rows of W + 4 floats pass 64 KiB; W = 512 is a plane of 1024 floats and goes one per tile again
EDGE_W = (472, 476, 480, 500, 512)
EDGE_FUSABLE = {(472, 1): 1, (476, 1): 0, (480, 1): 0, (500, 1): 0, (512, 1): 1,
                (472, 2): 1, (476, 2): 1, (480, 2): 1, (500, 2): 1, (512, 2): 1}


def test_predicates_answer_what_dispatch_will_do():
    L = _lib()
    for act in (NONE, RELU, LRELU, CLAMP, ABS, TANH, LOGISTIC):
        for sh in ((1, 2, 2, 500), (1, 3, 2, 508)):
            assert not L.bcnn_hip_depthwise_bn_fusable(*sh, 3, 1, 1, act), (sh, act)
            for in_act in (NONE, RELU, LRELU):
                assert not L.bcnn_hip_depthwise_bnin_fusable(*sh, 3, 1, 1, act, in_act), (sh, act, in_act)
    for (wd, s), yes in EDGE_FUSABLE.items():
        assert bool(L.bcnn_hip_depthwise_bn_fusable(1, 2, 2, wd, 3, s, 1, RELU)) == bool(yes), (wd, s)
        assert bool(L.bcnn_hip_depthwise_bnin_fusable(1, 2, 2, wd, 3, s, 1, RELU, RELU)) == bool(yes), (wd, s)
        if not yes:  # no sums buffer for a layer that is not fusable
            assert L.bcnn_hip_depthwise_insums_size(1, 2, 2, wd, 3, s, 1) == 0
    # planes of two columns and 500 rows: only the kernels that want aligned tensors could take them
    assert not L.bcnn_hip_depthwise_bn_fusable(1, 2, 500, 2, 3, 1, 1, RELU)
    assert L.bcnn_hip_depthwise_insums_size(1, 2, 500, 2, 3, 1, 1) > 0   # a size is room for whichever kernel may run, not a yes
    for n, c, h, w, s in [sh for sh, _ in D.SHAPES] + PAIR_SHAPES + INSUMS:
        assert L.bcnn_hip_depthwise_bn_fusable(n, c, h, w, 3, s, 1, RELU), (n, c, h, w, s)
        assert L.bcnn_hip_depthwise_bnin_fusable(n, c, h, w, 3, s, 1, RELU, RELU), (n, c, h, w, s)
        assert L.bcnn_hip_depthwise_insums_size(n, c, h, w, 3, s, 1) >= 2 * c * n
        assert L.bcnn_hip_depthwise_stats_size(n, c, h, w, 3, s, 1) >= 2 * c * n


def _child():
    """Runs in a process of its own (an entry point that the predicate wrongly admits ends the process): backward_bn on planes of
    2 x W wherever the predicate says yes, against the reference. One line per shape; exit status 0 only if all of it held."""
    L = _lib()
    for s in (1, 2):
        for wd in EDGE_W:
            shape = (1, 2, 2, wd, s)
            yes = L.bcnn_hip_depthwise_bn_fusable(1, 2, 2, wd, 3, s, 1, RELU)
            print("W %d stride %d fusable %d" % (wd, s, yes), flush=True)
            if not yes:
                continue
            p = _reference(shape, RELU, RELU)
            inp = _Inputs(p, 0)
            got = _backward(p, inp, "bn", 1, 0, x="xin")
            # more than 64 column groups: never marching
            _check_backward("2x%d s%d" % (wd, s), p, got, True, 1, "dwl", "bn", _forward_splits(p, inp, "dwl", "xin"))
            inp.assert_unchanged()
    print("child done", flush=True)


def test_backward_bn_runs_wherever_the_predicate_admits_two_row_planes():
    r = subprocess.run([sys.executable, "-c", "from tests.test_depthwise_fused_bn import _child; _child()"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("W ")]
    assert lines == ["W %d stride %d fusable %d" % (wd, s, EDGE_FUSABLE[(wd, s)]) for s in (1, 2) for wd in EDGE_W], r.stdout
    assert r.stdout.rstrip().endswith("child done")
