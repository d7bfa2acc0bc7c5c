"""The conv + eltwise residual fusion at the C ABI: bcnn_hip_conv_residual_fusable, bcnn_hip_conv_forward_residual and
bcnn_hip_conv_backward_residual (include/bcnn_hip.h:227-258, csrc/conv.hip:561-578 and :661-675), which fold the eltwise node
behind a conv + batch-norm node into the batch-norm's sweeps (csrc/batchnorm.hip: BnApplyBody :164-213, bn_recompute_y
:220-227, BwdSumsF :229-277, BnBwdApplyBody :370-418, bn_residual_grad_kernel :557-561). The graph-level tests run this pair
with RELU, operands of the same depth and res_count = one image on planes whose size is a multiple of four; here every branch
of the residual part of those bodies is reached with the smallest shape that does (tests/_residual_ref.py: SHAPES, CASES).

Cases: conv (n, c, h, w) -> f, k/stride/pad; HW the output plane, rc = res_count
  A (2,3,8,8)->8 3/1/1, HW 64, total 1024: flat_map_kernel (chan_reduce.h:143-166), every call a whole float4 group
      rc 512            one image, what the host passes
      rc 320            five of eight channels: the boundary inside image 0 (min_c < f)
      rc 511, 510, 509  the partial-float4 branch of BnApplyBody (batchnorm.hip:192-196), all three remainders
      rc 0              nothing added (:192 false everywhere; bn_residual_grad_kernel not launched, :581)
      rc 1024, 1031     the whole tensor; clamped to it (:435, :580)
  B (2,4,7,7)->3 3/1/1, HW 49, total 294: groups that straddle a plane edge go through the body one element at a time
      (chan_reduce.h:154-160 -> batchnorm.hip:202-210, :408-415); chan_reduce_partial takes its scalar loop (:67-80)
      rc 147            one image;  rc 98  two planes
  C (4,2,5,5)->6 1/1/0, HW 25: planes straddle float4 groups; rc 150 (one image), 75
  D (2,4,8,8)->8 1/2/0, HW 16: the down-sampling projection (1x1, stride 2: the raw-view convolution); rc 128
  E (1,3,32,32)->4 3/1/1, HW 1024: the smallest plane on plane_map_kernel (chan_reduce.h:113-122, :171); rc 4096 (= total
      with n = 1), 2048
  F (2,2,65,64)->3 3/1/1, HW 4160: two chunks per plane, the second 64 elements; three splits in the backward reduction
      (chan_splits, chan_reduce.h:21-30, restated and asserted below); rc 12480 (one image), 8257 (inside the second chunk of
      a plane, ending mid-group)
  activations: RELU everywhere; NONE, RAMP, LRELU, ABS and CLAMP too on A (rc 512, 510) and on B.

What is compared and how
  against the float64 restatement (tests/_residual_ref.py: chain64), every output of both passes: tests._golden.assert_close
      at tests.test_hip_parity.REL_TOL; saved_var, run_var and dvar as test_hip_parity treats its VAR_KEYS.
  against the unfused pair on the GPU (bcnn_hip_conv_forward + bcnn_hip_eltwise_forward; bcnn_hip_eltwise_backward +
      bcnn_hip_conv_backward):
      forward   IN BITS: out, saved_mean, saved_var, run_mean, run_var, bn_workspace; and bcnn_hip_batchnorm_apply on the fused
                call's bn_workspace reproduces the unfused conv output in bits (the header's promise). Both routes run the same
                convolution, the same statistics, bn_one, one add, act_fwd_cheap; the library is built without contraction.
      backward  IN BITS: dres. bn_residual_grad_kernel (:559-560) and eltwise_bwd_kernel (next.hip:62-84) both form
                dout * act_bwd_cheap(out) in one multiply from the same two stored values and add it to dres once.
                AT REL_TOL: dscales, dbias, dmean, dvar (VAR_KEYS rule), dy, dw, dx. The fused sweeps multiply dout by act' of a
                RECOMPUTED output inside the reduction, the unfused ones read the product back from memory: the same values
                as long as the compiler keeps the multiply and the adds apart, which a test should not rely on.
  behaviour (A rc 320 RELU, B rc 98 RELU, B rc 147 LRELU): dres accumulates onto finite garbage and is untouched behind rc;
      dres == NULL and dx == NULL leave every other output the same in bits; the backward leaves dres_out, res, res_out, x, w
      unchanged and never reads res_out behind rc (NaN there changes nothing); forward writes every element of res_out and
      backward every element of dy (a sentinel pre-fill is gone); two runs give equal bits.
  every tensor is a tests._next_ref.Guarded view (sentinel bands either side, checked by every read).

Worst figures observed on an MI355X over all cases (tests._golden.WORST: per-tensor relative error; the worst element as a
fraction of its own bound), printed again at the end of every GPU run of this module:
  against float64, forward    out 4.8e-07 / 0.016   bn_workspace 1.8e-07 / 0.009   saved_mean 2.1e-07 / 0.017
                              run_mean 6.9e-08 / 0.001
  against float64, backward   dres 4.4e-08 / 0.001  dscales 3.6e-07 / 0.021  dbias 4.2e-07 / 0.028  dmean 4.1e-07 / 0.007
                              dy 1.6e-07 / 0.003    dw 1.4e-06 / 0.028       dx 3.2e-07 / 0.014
  float32 restatement (CPU)   out 6.3e-07 / 0.023   dw 7.5e-07 / 0.021 the largest; every other tensor below them
  against the unfused pair    0 for every tensor of the backward pass (equal in bits on this compiler; only dres is asserted so)
  the host-linked graph       0: the whole pass and the node-by-node walk agree in bits"""
import functools
import types

import numpy as np
import pytest

from tests import _bn_ref as B
from tests import _golden as G
from tests import _next_ref as R
from tests import _residual_ref as RR
from tests.test_hip_parity import REL_TOL, VAR_KEYS

gpu = pytest.mark.gpu
F32, F64 = np.float32, np.float64
TRAIN, VALID, PREDICT = B.MODE_TRAIN, B.MODE_VALID, B.MODE_PREDICT
ACT_RELU6 = 10                                      # include/bcnn_hip.h: the first id behind the reference's ten
STALE = F32(-7777.25)                               # finite pre-fill of out / dy / bn_workspace: none of it may remain
BEHAVIOUR_CASES = [("A", 320, R.ACT_RELU), ("B", 98, R.ACT_RELU), ("B", 147, R.ACT_LRELU)]

case_ids = [RR.case_id(c) for c in RR.CASES]
behaviour_ids = [RR.case_id(c) for c in BEHAVIOUR_CASES]


def close(tag, got, want64):
    """the bars of test_hip_parity.py: REL_TOL through G.assert_close; rtol 1e-4 / atol 1e-6 for the variance keys"""
    got, want64 = np.asarray(got).ravel(), np.asarray(want64, F64).ravel()
    assert got.shape == want64.shape, (tag, got.shape, want64.shape)
    assert np.all(np.isfinite(got)), tag
    if tag.split(":")[-1] in VAR_KEYS:
        assert np.allclose(got, want64, rtol=1e-4, atol=1e-6), (tag, np.abs(got - want64).max())
    else:
        G.assert_close(tag, got, want64, REL_TOL, rtol=REL_TOL, afrac=REL_TOL / 10)


# ---- CPU: the arithmetic of the cases, the inputs, and the reference against itself ------------------------------------------
def chan_splits(channels, per_channel):
    """csrc/chan_reduce.h:21-30 with CHAN_WG_PER_CU = 4, kCUs = 256, CHAN_MIN_ELEMS = 4096"""
    want = (4 * 256 + channels - 1) // channels
    want = min(want, (per_channel + 4095) // 4096)
    return min(max(want, 1), 1024)


def test_shapes_reach_the_branches_they_are_named_for():
    geo = {s: RR.geometry(s) for s in RR.SHAPES}
    assert [(geo[s].hw, geo[s].total) for s in "ABCDEF"] == [(64, 1024), (49, 294), (25, 600), (16, 256), (1024, 4096),
                                                              (4160, 24960)]
    # A: whole groups everywhere (HW % 4 == 0), and the three remainders of the partial group
    assert geo["A"].hw % 4 == 0 and sorted(rc % 4 for rc in (511, 510, 509)) == [1, 2, 3]
    assert 320 == 5 * geo["A"].hw and 512 == geo["A"].f * geo["A"].hw and 1031 > geo["A"].total
    # B, C: planes that are no multiple of four, so groups straddle plane edges; rc values are whole planes or images
    for s, per_image in (("B", 147), ("C", 150)):
        g = geo[s]
        assert g.hw % 4 != 0 and g.hw < 1024 and g.f * g.hw == per_image and all(rc % g.hw == 0 for rc in RR.RC[s])
    assert geo["D"].hw == 16 and geo["D"].k == 1 and geo["D"].s == 2 and RR.RC["D"] == [geo["D"].f * 16]
    # E: the threshold of launch_chan_map (HW >= 1024 -> plane_map_kernel), one chunk per plane
    assert geo["E"].hw == 1024 and geo["E"].n == 1 and RR.RC["E"][0] == geo["E"].total
    # F: two 4096-element chunks per plane, the second 64 long; rc 8257 = plane 1 + 4097: in that chunk, one element into a group
    g = geo["F"]
    assert (g.hw + 4095) // 4096 == 2 and g.hw - 4096 == 64 and RR.RC["F"] == [g.f * g.hw, g.hw + 4097] and 8257 % 4 == 1
    assert chan_splits(g.f, g.M) == 3
    assert [chan_splits(geo[s].f, geo[s].M) for s in "ABCDE"] == [1] * 5
    # every case the issue lists, once
    assert len(set(RR.CASES)) == len(RR.CASES) == 37


@pytest.mark.parametrize("case", RR.CASES, ids=case_ids)
def test_inputs_make_the_case_bite(case):
    """act' depends on res inside [0, rc), in the last four elements before rc, and would in the four behind it; out[rc - 1]
    depends on res and out[rc] would; nothing sits on a kink (tests/_residual_ref.py: preconditions)"""
    assert RR.preconditions(*case) == []


@pytest.mark.parametrize("case", RR.CASES, ids=case_ids)
def test_float32_restatement_meets_the_bar(case):
    """float32 arithmetic alone (one rounding per operation) is inside the bar the kernels are held to, at every shape"""
    want, got = RR.chain64(*case), RR.chain32(*case)
    for k in RR.FWD_KEYS + RR.BWD_KEYS:
        close("%s/residual_f32:%s" % (RR.case_id(case), k), got[k], want[k])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401
    from bcnn_amd import _lib
    yield _lib.load()
    mine = {k: v for k, v in G.WORST.items() if k.startswith("residual_")}
    for k in sorted(mine):
        print("worst %-28s rel %.3e, element %.3f of its bound" % (k, mine[k][0], mine[k][1]))


def filled(size, value=STALE, shift=0):
    return R.Guarded(np.full(size, value, F32), shift)


def ptr(g):
    return None if g is None else g.ptr


def conv_dims(g):
    return [g.n, g.c, g.h, g.w, g.f, g.k, g.s, g.p, 1]


def forward_buffers(p):
    g = p.g
    t = types.SimpleNamespace()
    t.x, t.w, t.bias, t.scales, t.res = (R.Guarded(v) for v in (p.x, p.w, p.bias, p.scales, p.res))
    t.run_mean, t.run_var = R.Guarded(p.run_mean0), R.Guarded(p.run_var0)
    t.saved_mean, t.saved_var = filled(g.f), filled(g.f)
    t.bn_workspace, t.out = filled(g.total), filled(g.total)
    return t


def forward_outputs(t):
    return {k: getattr(t, k).read() for k in RR.FWD_KEYS}


def fused_forward(L, shape, rc, act):
    p = RR.inputs(shape)
    t = forward_buffers(p)
    L.bcnn_hip_conv_forward_residual(t.x.ptr, t.w.ptr, t.bias.ptr, *conv_dims(p.g), t.run_mean.ptr, t.run_var.ptr, t.scales.ptr,
                                     t.saved_mean.ptr, t.saved_var.ptr, t.bn_workspace.ptr, t.res.ptr, rc, act, t.out.ptr)
    L.bcnn_hip_sync()
    return t


def unfused_forward(L, shape, rc, act):
    p = RR.inputs(shape)
    t = forward_buffers(p)
    t.y = filled(p.g.total)
    L.bcnn_hip_conv_forward(t.x.ptr, t.w.ptr, t.bias.ptr, t.y.ptr, *conv_dims(p.g), R.ACT_NONE, None, 1, t.run_mean.ptr,
                            t.run_var.ptr, t.scales.ptr, t.saved_mean.ptr, t.saved_var.ptr, None, t.bn_workspace.ptr, TRAIN)
    L.bcnn_hip_eltwise_forward(t.y.ptr, t.res.ptr, t.out.ptr, p.g.total, rc, act)
    L.bcnn_hip_sync()
    return t


def backward_buffers(L, p, dres=True, dx=True):
    g = p.g
    b = types.SimpleNamespace()
    b.dout = R.Guarded(p.dout)
    b.dy = filled(g.total)
    b.dx = filled(p.x.size) if dx else None
    b.dw, b.dscales, b.dbias = R.Guarded(p.dw0), R.Guarded(p.dscales0), R.Guarded(p.dbias0)
    b.dmean, b.dvar = filled(g.f), filled(g.f)
    b.dres = R.Guarded(p.dres0) if dres else None
    b.ws_elems = int(L.bcnn_hip_conv_workspace_size(*conv_dims(g)))
    b.workspace = filled(max(b.ws_elems, 4))
    return b


def backward_outputs(b):
    return {k: getattr(b, k).read() for k in RR.BWD_KEYS if getattr(b, k) is not None}


def fused_backward(L, shape, rc, act, t, dres=True, dx=True, res_out=None):
    """t: the tensors a fused forward left; res_out: another tensor to pass as the eltwise output"""
    p = RR.inputs(shape)
    b = backward_buffers(L, p, dres, dx)
    L.bcnn_hip_conv_backward_residual(t.x.ptr, t.w.ptr, t.bias.ptr, b.dy.ptr, ptr(b.dx), b.dw.ptr, b.dbias.ptr, *conv_dims(p.g),
                                      t.scales.ptr, b.dscales.ptr, t.saved_mean.ptr, t.saved_var.ptr, b.dmean.ptr, b.dvar.ptr,
                                      t.bn_workspace.ptr, b.workspace.ptr, b.ws_elems, (res_out or t.out).ptr, b.dout.ptr, act,
                                      t.res.ptr, ptr(b.dres), rc)
    L.bcnn_hip_sync()
    return b


def unfused_backward(L, shape, rc, act, t):
    """t: the tensors an unfused forward left. The eltwise backward stores g over its dy: it gets a copy of dout"""
    p = RR.inputs(shape)
    b = backward_buffers(L, p)
    L.bcnn_hip_eltwise_backward(t.out.ptr, b.dout.ptr, b.dy.ptr, b.dres.ptr, p.g.total, rc, act, 1)
    L.bcnn_hip_conv_backward(t.x.ptr, t.w.ptr, t.bias.ptr, t.y.ptr, b.dy.ptr, b.dx.ptr, b.dw.ptr, b.dbias.ptr, *conv_dims(p.g),
                             R.ACT_NONE, None, None, 1, t.scales.ptr, b.dscales.ptr, t.saved_mean.ptr, t.saved_var.ptr,
                             b.dmean.ptr, b.dvar.ptr, None, t.bn_workspace.ptr, b.workspace.ptr, b.ws_elems)
    L.bcnn_hip_sync()
    return b


@functools.lru_cache(maxsize=None)
def run(L, case):
    """both routes, both passes, once per case; the tests below read what they need"""
    r = types.SimpleNamespace()
    r.fused, r.unfused = fused_forward(L, *case), unfused_forward(L, *case)
    r.forward_state = forward_outputs(r.fused)
    r.fused_bwd = fused_backward(L, *case, r.fused)
    r.unfused_bwd = unfused_backward(L, *case, r.unfused)
    return r


def no_stale(tag, values):
    left = np.flatnonzero(R.bits(values) == R.bits(STALE))
    assert left.size == 0, "%s: %d elements were never written, first at %d" % (tag, left.size, left[0])


@gpu
@pytest.mark.parametrize("case", RR.CASES, ids=case_ids)
def test_forward_equals_the_unfused_pair_in_bits(L, case):
    shape, rc, act = case
    p, tag = RR.inputs(shape), RR.case_id(case)
    r = run(L, case)
    got, want = forward_outputs(r.fused), forward_outputs(r.unfused)
    for k in RR.FWD_KEYS:
        no_stale(tag + "/" + k, got[k])
        R.assert_bits("%s/%s fused against unfused" % (tag, k), got[k], want[k])
    for k in ("x", "w", "bias", "scales", "res"):
        getattr(r.fused, k).assert_unchanged(tag + "/" + k)
    # the conv node's own output, on demand, from what the fused call kept
    y = filled(p.g.total)
    L.bcnn_hip_batchnorm_apply(r.fused.bn_workspace.ptr, y.ptr, r.fused.scales.ptr, r.fused.bias.ptr, r.fused.saved_mean.ptr,
                               r.fused.saved_var.ptr, p.g.n, p.g.f, p.g.hw, R.ACT_NONE)
    L.bcnn_hip_sync()
    R.assert_bits(tag + "/batchnorm_apply on the fused workspace against the unfused conv output", y.read(), r.unfused.y.read())


@gpu
@pytest.mark.parametrize("case", RR.CASES, ids=case_ids)
def test_forward_against_float64(L, case):
    want, got = RR.chain64(*case), forward_outputs(run(L, case).fused)
    for k in RR.FWD_KEYS:
        close("%s/residual_fwd:%s" % (RR.case_id(case), k), got[k], want[k])


def check_untouched_parts(tag, p, rc, b, want):
    """dres behind rc and dx behind the prefix the convolution defines keep their pre-fill, in bits"""
    rcc = min(rc, p.g.total)
    if b.dres is not None:
        R.assert_bits(tag + "/dres behind rc", b.dres.read()[rcc:], p.dres0[rcc:])
    if b.dx is not None:
        rest = b.dx.read().reshape(p.g.n, -1)[:, want["dx_prefix"]:]
        R.assert_bits(tag + "/dx behind the prefix", rest, np.full(rest.shape, STALE, F32))


@gpu
@pytest.mark.parametrize("case", RR.CASES, ids=case_ids)
def test_backward_against_float64(L, case):
    shape, rc, act = case
    p, tag, want = RR.inputs(shape), RR.case_id(case), RR.chain64(*case)
    r = run(L, case)
    got = backward_outputs(r.fused_bwd)
    no_stale(tag + "/dy", got["dy"])
    for k in RR.BWD_KEYS:
        a, b = got[k], want[k]
        if k == "dx":
            a, b = a.reshape(p.g.n, -1)[:, :want["dx_prefix"]], b[:, :want["dx_prefix"]]
        close("%s/residual_bwd:%s" % (tag, k), a, b)
    check_untouched_parts(tag, p, rc, r.fused_bwd, want)
    r.fused_bwd.dout.assert_unchanged(tag + "/dres_out")
    for k in ("x", "w", "bias", "scales", "res"):
        getattr(r.fused, k).assert_unchanged(tag + "/" + k + " after the backward")
    after = forward_outputs(r.fused)
    for k in RR.FWD_KEYS:  # res_out and the state the forward left
        R.assert_bits(tag + "/" + k + " after the backward", after[k], r.forward_state[k])


@gpu
@pytest.mark.parametrize("case", RR.CASES, ids=case_ids)
def test_backward_against_the_unfused_pair(L, case):
    """dres in bits, the rest at the bar (the module docstring says why)"""
    shape, rc, act = case
    p, tag, want64 = RR.inputs(shape), RR.case_id(case), RR.chain64(*case)
    r = run(L, case)
    got, want = backward_outputs(r.fused_bwd), backward_outputs(r.unfused_bwd)
    R.assert_bits(tag + "/dres fused against unfused", got["dres"], want["dres"])
    for k in RR.BWD_KEYS:
        a, b = got[k], want[k]
        if k == "dx":
            a, b = (v.reshape(p.g.n, -1)[:, :want64["dx_prefix"]] for v in (a, b))
        close("%s/residual_unfused:%s" % (tag, k), a, b)


@gpu
@pytest.mark.parametrize("case", BEHAVIOUR_CASES, ids=behaviour_ids)
def test_backward_optional_outputs_and_what_it_reads(L, case):
    shape, rc, act = case
    p, tag = RR.inputs(shape), RR.case_id(case)
    r = run(L, case)
    base = backward_outputs(r.fused_bwd)
    # dres accumulates onto what it held, in one float32 add of the float32 product
    g32 = B.act_grad32(p.dout, r.fused.out.read(), act)
    R.assert_bits(tag + "/dres = garbage + g", base["dres"][:rc], (p.dres0[:rc] + g32[:rc]).astype(F32))
    R.assert_bits(tag + "/dres behind rc", base["dres"][rc:], p.dres0[rc:])
    # determinism
    again = backward_outputs(fused_backward(L, *case, r.fused))
    for k in RR.BWD_KEYS:
        R.assert_bits(tag + "/second run/" + k, again[k], base[k])
    # dres == NULL, dx == NULL: the other outputs do not move
    for what, kw in (("dres NULL", dict(dres=False)), ("dx NULL", dict(dx=False))):
        got = backward_outputs(fused_backward(L, *case, r.fused, **kw))
        assert set(base) - set(got) == {what.split()[0]}
        for k in got:
            R.assert_bits("%s/%s/%s" % (tag, what, k), got[k], base[k])
    # of res_out only the first rc elements are read: NaN behind them changes nothing
    poisoned = r.fused.out.read()
    poisoned[rc:] = np.nan
    assert rc < p.g.total
    b = fused_backward(L, *case, r.fused, res_out=R.Guarded(poisoned))
    got = backward_outputs(b)
    for k in RR.BWD_KEYS:
        R.assert_bits("%s/res_out poisoned behind rc/%s" % (tag, k), got[k], base[k])
    b.dout.assert_unchanged(tag + "/dres_out")


@gpu
@pytest.mark.parametrize("case", BEHAVIOUR_CASES, ids=behaviour_ids)
def test_forward_is_deterministic(L, case):
    first, second = forward_outputs(run(L, case).fused), forward_outputs(fused_forward(L, *case))
    for k in RR.FWD_KEYS:
        R.assert_bits(RR.case_id(case) + "/second run/" + k, second[k], first[k])


@gpu
def test_fusable_truth_table(L):
    """launches nothing: the pointers are only looked at"""
    ok, off = filled(16), filled(16, shift=1)
    fusable = lambda bn=1, act=R.ACT_NONE, res_act=R.ACT_RELU, mode=TRAIN, ws=ok, res=ok, out=ok: bool(
        L.bcnn_hip_conv_residual_fusable(bn, act, res_act, mode, ptr(ws), ptr(res), ptr(out)))
    for a in RR.CHEAP_ACTS:
        assert fusable(res_act=a), R.ACT_NAMES[a]
    for a in (R.ACT_TANH, R.ACT_SOFTPLUS, R.ACT_LOGISTIC, R.ACT_PRELU, ACT_RELU6):
        assert not fusable(res_act=a), a
    assert not fusable(bn=0)
    for a in (R.ACT_RELU, R.ACT_LRELU, R.ACT_TANH, R.ACT_PRELU):
        assert not fusable(act=a), R.ACT_NAMES[a]
    assert not fusable(mode=VALID) and not fusable(mode=PREDICT)
    assert not fusable(ws=None)
    assert not fusable(res=off) and not fusable(out=off) and not fusable(ws=off)
    for g in (ok, off):
        g.assert_unchanged("fusable")


# ---- one small graph through the host linking (bcnn_link_conv_eltwise, host/bcnn_layers_hot.c:206-275) ------------------------
@gpu
def test_host_links_the_pair_when_the_second_operand_is_shallower():
    """input (n = 3, 6 x 7 x 7) -> conv 4 ch 3x3 + BN relu "a" -> conv 6 ch 3x3 + BN "b" -> eltwise(LRELU, "a", "b"): "b", created
    later, becomes the first operand (bcnn_layers_next.c:33-36), so min_c = 4 < 6 on 49-element planes and res_count = 196 ends
    inside image 0. The whole bcnn_forward / bcnn_backward pass against the node-by-node walk of the same state, as step 3 of
    test_product_dispatch_parity.py does it, with that file's checker and bar. (What the eltwise node adds to d(a) does not
    survive either route: the convolution "b", which runs behind it in a backward pass, overwrites d(a) as the reference's
    does. d(res) itself is pinned by the op tests above.)"""
    import ctypes
    from bcnn_amd import _lib, capi
    from tests.test_product_dispatch_parity import _Checker
    H = _lib.load()
    ctypes.CDLL(None).srand(20240607)
    net = capi.Net(mode=capi.MODE_TRAIN, w=7, h=7, c=6, n=3)
    net.conv(4, 3, 1, 1, 1, 1, capi.ACT_RELU, "input", "a")
    conv_b = net.conv(6, 3, 1, 1, 1, 1, capi.ACT_NONE, "a", "b")
    elt = net.eltwise(capi.ACT_LRELU, "a", "b", "out")
    net.compile()
    ta, tb, tout = net.index("a"), net.index("b"), net.index("out")
    assert (net.node_src(elt, 0), net.node_src(elt, 1), net.node_dst(elt)) == (tb, ta, tout)
    assert net.shape(ta) == (3, 4, 7, 7) and net.shape(tb) == net.shape(tout) == (3, 6, 7, 7)
    nt = 0
    while net.L.bcnn_peek_tensor(net.net, nt):
        nt += 1
    names = [(net.tensor(t).name or b"").decode() for t in range(nt)]
    rs = np.random.RandomState(11)
    for t in range(2, nt):  # batch-norm parameters that matter; the convolution weights keep their Xavier draw
        if not net.tensor(t).data:
            continue
        if names[t].endswith("_scales"):
            net.data(t)[...] = rs.uniform(0.5, 1.5, net.shape(t))
        elif names[t].endswith("_b"):
            net.data(t)[...] = rs.uniform(-0.5, 0.5, net.shape(t))
        net.upload(t)
    net.data(0)[...] = rs.uniform(-1, 1, net.shape(0)).astype(F32)
    net.upload(0)
    dy = rs.uniform(-1, 1, net.shape(tout)).astype(F32)
    size = int(np.prod(net.shape(tout)))

    def device(t, grad=False):
        """the tensor's device memory as it is, without the on-demand production of bcnn_download_tensor"""
        v = np.empty(size, F32)
        H.bcnn_hip_sync()
        H.bcnn_hip_memcpy_d2h(v.ctypes.data, net.tensor(t).grad_data_gpu if grad else net.tensor(t).data_gpu, v.nbytes)
        return v

    grad_ids = [t for t in range(nt) if net.grad(t) is not None and net.tensor(t).data]

    def set_grads():
        for t in grad_ids:
            net.grad(t)[...] = dy if t == tout else 0
            net.upload(t, True)

    # the pair is linked: a whole forward pass writes `out` and leaves the convolution's own output tensor alone
    for t in (tb, tout):
        H.bcnn_hip_fill_f32(net.tensor(t).data_gpu, size, float(STALE))
    net.forward()
    R.assert_bits("the conv node's own output after a whole pass", device(tb), np.full(size, STALE, F32))
    no_stale("out", device(tout))
    fused_out = device(tout)
    for t in range(nt):
        if net.tensor(t).data:
            net.download(t, False)  # host copies = device state (produces "b" on demand), so that uploads below change nothing
    set_grads()  # behind the forward pass, whose first act is the zero fill of the output gradients
    net.backward()
    # ... and in the backward pass: the fused call reads the eltwise node's output gradient and does not rewrite it, where the
    # eltwise worker stores dout * act'(out) over it (produced on demand by the download below)
    R.assert_bits("d(out) on the device after a whole backward pass", device(tout, True), dy)
    fused = {}
    for t in grad_ids:
        net.download(t, True)
        fused[t] = net.grad(t).copy()
    # the same state, node by node
    set_grads()
    for i in range(net.num_nodes - 1, -1, -1):
        net.backward_node(i)
    chk = _Checker()
    for t in grad_ids:
        net.download(t, True)
        assert np.all(np.isfinite(fused[t])), names[t]
        chk(fused[t], net.grad(t), "d(%s)" % names[t])
    assert not np.array_equal(fused[tout], dy)  # LRELU: the gradient behind the activation backward is another tensor
    assert float(np.abs(fused[ta]).max()) > 0 and float(np.abs(fused[net.node_src(conv_b, 1)]).max()) > 0
    # and the forward: every node alone reproduces what the fused pass wrote
    for i in range(net.num_nodes):
        net.forward_node(i)
    chk(fused_out, device(tout), "out")
    print("host-linked pair, min_c < f: worst deviation %.2e (%s), worst element %.3f of its bound (%s)"
          % (chk.worst[0], chk.worst[1], chk.worst_elem[0], chk.worst_elem[1]))
    net.close()
