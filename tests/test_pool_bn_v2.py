"""The stem's two pooling kernels, second generation (pool.hip: maxpool_fwd_s2_bn_v2_kernel, maxpool_bwd_pair_bn_v2_kernel).
They do the first generation's arithmetic with fewer instructions -- the fifth window column over a wave shift, the
bcnn_scal / bcnn_add_scalar quirks and the activation classified once instead of per element, a scatter that tests only
the (window, component) pairs that can hit -- so every result has to stay bit for bit:

* forward against bcnn_hip_batchnorm_apply + bcnn_hip_maxpool_forward (as tests/test_pool_bn.py), values compared as int32
  patterns, with and without the kept raw values, at the shapes where the thread mapping changes;
* both kernels against the first generation, which the experiment build keeps behind BCNN_HIP_POOL_PAIR_V1, in one child
  process on that build;
* the backward also against the separate calls at the 1e-5 of tests/test_pool_bn_backward.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = {"none": 0, "relu": 2, "lrelu": 5, "clamp": 7}

# (n, c, h, w, size): one float4 per row and no neighbour; odd height; waves spanning rows and planes with OH = 17 ragged
# for 4 and 8 rows per thread; size 2 (no fifth column); 66 output pairs per row (a wave's last lane has its right
# neighbour in the next wave)
FWD_SHAPES = [(1, 3, 3, 4, 3), (2, 4, 7, 8, 3), (2, 3, 33, 36, 3), (2, 3, 34, 36, 2), (3, 5, 20, 264, 3)]
# (n, c, h, w): 16 x 16; 18 x 20; odd height; W / 4 == 1 (no multiply-high division); a row longer than a wave
BWD_SHAPES = [(2, 8, 16, 16), (3, 6, 18, 20), (1, 5, 7, 8), (2, 3, 6, 4), (2, 4, 10, 264)]


def _channels(rs, c, quirks):
    """scale / bias per channel; with `quirks`: channel 0 scale 0, channel 1 scale 1 and bias 0, channel 2 bias 1 (the
    bcnn_scal / bcnn_add_scalar special cases), channel 4 bias 0; without: none, so that whole waves take the plain path"""
    sc = rs.uniform(0.5, 1.5, c).astype(np.float32)
    b = rs.uniform(-0.2, 0.2, c).astype(np.float32)
    if quirks:
        sc[0] = 0.0
        sc[1] = 1.0
        b[1] = 0.0
        b[2] = 1.0
        if c > 4:
            b[4] = 0.0
    return sc, b


def _fwd_input(rs, n, c, h, w):
    x = rs.uniform(-2, 2, (n, c, h, w)).astype(np.float32)
    flat = x.reshape(-1)
    for val in (np.nan, np.inf, -np.inf, -0.0):
        flat[rs.choice(flat.size, max(1, flat.size // 37), replace=False)] = val
    x[0, c - 1] = -30.0     # a plane ReLU turns into zeros: every window is a tie, the first index wins
    x[n - 1, 0] = 0.75      # a constant plane
    return x


@pytest.mark.parametrize("quirks", [True, False], ids=["quirk_channels", "plain_channels"])
@pytest.mark.parametrize("act", sorted(ACTS), ids=str)
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "n%d_c%d_%dx%d_k%d" % s)
def test_forward_equals_apply_then_pool_bit_for_bit(shape, act, quirks):
    from bcnn_amd import _lib, ops
    L = _lib.load()
    n, c, h, w, size = shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    rs = np.random.RandomState(31)
    x = torch.from_numpy(_fwd_input(rs, n, c, h, w)).to(DEV)
    sc, b = (torch.from_numpy(a).to(DEV) for a in _channels(rs, c, quirks))
    mean = torch.from_numpy(rs.uniform(-0.3, 0.3, c).astype(np.float32)).to(DEV)
    var = torch.from_numpy(rs.uniform(0.2, 2.0, c).astype(np.float32)).to(DEV)
    a = ACTS[act]
    assert ops.maxpool_bn_fusable(x, oh, ow, size, 2, a)
    y = torch.empty_like(x)
    ops.batchnorm_apply(x, y, sc, b, mean, var, a)
    p1 = torch.empty((n, c, oh, ow), device=DEV)
    i1 = torch.empty((n, c, oh, ow), device=DEV, dtype=torch.int32)
    ops.maxpool_forward(y, p1, i1, size, 2)
    P = lambda t: t.data_ptr()
    for keep in (False, True):
        p2, i2, ram = torch.full_like(p1, 7.0), torch.full_like(i1, -7), torch.full_like(p1, 9.0)
        L.bcnn_hip_maxpool_forward_bn_keep(P(x), P(p2), P(i2), n, c, h, w, oh, ow, size, 2, P(sc), P(b), P(mean), P(var), a,
                                           P(ram) if keep else 0)
        torch.cuda.synchronize()
        assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)), "values, keep=%d" % keep
        assert torch.equal(i1, i2), "indexes, keep=%d" % keep
        if keep:
            won = i2.flatten() >= 0
            want = torch.where(won, x.flatten()[i2.flatten().clamp(min=0).long()], torch.zeros((), device=DEV))
            assert torch.equal(ram.flatten().view(torch.int32), want.view(torch.int32)), "kept raw values"


# ---- against the first generation, on the experiment build -----------------------------------------------------------------------
_CHILD = r"""
import ctypes, json, os, sys
sys.path.insert(0, %r)
import numpy as np, torch
from bcnn_amd import _lib
sys.path.insert(0, os.path.join(%r, "tests"))
import test_pool_bn_v2 as T
L = _lib.load()
DEV = "cuda:0"
P = lambda t: t.data_ptr()
out = {}
def both(fn):
    res = []
    for v1 in (False, True):
        if v1: os.environ["BCNN_HIP_POOL_PAIR_V1"] = "1"
        else: os.environ.pop("BCNN_HIP_POOL_PAIR_V1", None)
        L.bcnn_hip_trace_enable(1)  # clears the log
        res.append(fn())
        torch.cuda.synchronize()
        k = L.bcnn_hip_trace_read(None, 0)
        buf = ctypes.create_string_buffer(k + 1)
        L.bcnn_hip_trace_read(buf, k + 1)
        L.bcnn_hip_trace_enable(0)
        ran = set(buf.value.decode().split())  # the switch has to select the other generation, or the comparison says nothing
        want = {"maxpool_fwd_s2_bn_kernel" + (":v1" if v1 else ""), "maxpool_bwd_pair_bn_kernel" + (":v1" if v1 else "")}
        assert want <= ran and not ({"maxpool_fwd_s2_bn_kernel", "maxpool_fwd_s2_bn_kernel:v1", "maxpool_bwd_pair_bn_kernel",
                                     "maxpool_bwd_pair_bn_kernel:v1"} - want) & ran, sorted(ran)
    return res
for shape in T.BWD_SHAPES:
    for act in sorted(T.ACTS):
        n, c, h, w = shape
        a = T.ACTS[act]
        oh, ow = (h + 1) // 2, w // 2
        rs = np.random.RandomState(41)
        x = rs.uniform(-2, 2, (n, c, h, w)).astype(np.float32)
        x[n - 1, c - 1] = 0.75  # a constant plane: all windows over a source element select the same one
        x = torch.from_numpy(x).to(DEV)
        sc, b = (torch.from_numpy(t).to(DEV) for t in T._channels(rs, c, True))
        mean = torch.from_numpy(rs.uniform(-0.3, 0.3, c).astype(np.float32)).to(DEV)
        var = torch.from_numpy(rs.uniform(0.2, 2.0, c).astype(np.float32)).to(DEV)
        dpool = torch.from_numpy(rs.uniform(-0.1, 0.1, (n, c, oh, ow)).astype(np.float32)).to(DEV)
        def run():
            yp = torch.full((n, c, oh, ow), 7.0, device=DEV)
            idx = torch.full((n, c, oh, ow), -7, device=DEV, dtype=torch.int32)
            ram = torch.full((n, c, oh, ow), 9.0, device=DEV)
            L.bcnn_hip_maxpool_forward_bn_keep(P(x), P(yp), P(idx), n, c, h, w, oh, ow, 3, 2, P(sc), P(b), P(mean), P(var), a, P(ram))
            g = torch.full((n, c, h, w), float("nan"), device=DEV)
            z = [torch.zeros(c, device=DEV) for _ in range(4)]
            assert L.bcnn_hip_maxpool_bn_backward_fusable(n, c, h, w, oh, ow, 3, 2, a, P(x), P(dpool), P(idx), P(g))
            L.bcnn_hip_maxpool_bn_backward(P(dpool), P(idx), P(ram), P(x), P(g), n, c, h, w, oh, ow, 3, 2, P(sc), P(z[0]), P(b),
                                           P(z[1]), P(mean), P(var), P(z[2]), P(z[3]), a)
            return [yp, idx, ram, g] + z
        new, old = both(run)
        bad = [k for k, (p, q) in enumerate(zip(new, old)) if not torch.equal(p.view(torch.int32), q.view(torch.int32))]
        out["%%s/%%s" %% ("x".join(map(str, shape)), act)] = bad
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def first_generation():
    lib = os.path.join(ROOT, "bcnn_amd", "lib", "libbcnn_hip_exp.so")
    assert os.path.exists(lib), "experiment build missing: __graft_entry__.build() makes it"
    e = dict(os.environ)
    e["BCNN_HIP_LIB"] = lib
    e.pop("BCNN_HIP_POOL_PAIR_V1", None)
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, ROOT)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])


@pytest.mark.parametrize("act", sorted(ACTS), ids=str)
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "n%d_c%d_%dx%d" % s)
def test_both_kernels_equal_the_first_generation_bit_for_bit(first_generation, shape, act):
    names = ["pooled values", "indexes", "kept raw values", "dx", "dscales", "dbias", "dmean", "dvar"]
    bad = first_generation["%s/%s" % ("x".join(map(str, shape)), act)]
    assert not bad, "differs from the first generation: " + ", ".join(names[k] for k in bad)


# ---- backward against the separate calls (tests/test_pool_bn_backward.py, same tolerance) ----------------------------------------
def _close(a, b, tol, what):
    d = (a.double() - b.double()).abs().max().item()
    ref = b.double().abs().max().item()
    assert d <= tol * max(ref, 1e-3), "%s: %.3g of %.3g" % (what, d, ref)


@pytest.mark.parametrize("act", sorted(ACTS), ids=str)
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "n%d_c%d_%dx%d" % s)
def test_backward_matches_the_separate_calls(shape, act):
    from bcnn_amd import _lib, ops
    L = _lib.load()
    n, c, oh, ow = shape
    a = ACTS[act]
    cin, k = 3, 3
    rs = np.random.RandomState(23)
    T = lambda *sh: torch.from_numpy(rs.uniform(-1, 1, sh).astype(np.float32)).to(DEV)
    P = lambda t: 0 if t is None else t.data_ptr()
    x0, w1 = T(n, cin, oh, ow), T(c, cin, k, k) * 0.3
    scn, bnp = _channels(rs, c, True)
    scales, b1 = torch.from_numpy(scn).to(DEV), torch.from_numpy(bnp).to(DEV)
    Z = lambda: torch.zeros(c, device=DEV)
    bn = dict(run_mean=Z(), run_var=Z() + 1, scales=scales, saved_mean=Z(), saved_var=Z(),
              workspace=torch.empty((n, c, oh, ow), device=DEV))
    y1 = torch.empty((n, c, oh, ow), device=DEV)
    ops.conv_forward(x0, w1, b1, y1, k, 1, 1, 1, a, bn=bn)
    raw = bn["workspace"]
    raw[n - 1, c - 1] = 0.75  # a constant plane; the normalised tensor of the separate calls follows it
    ops.batchnorm_apply(raw, y1, scales, b1, bn["saved_mean"], bn["saved_var"], a)
    ph, pw = (oh + 1) // 2, ow // 2
    yp = torch.empty((n, c, ph, pw), device=DEV)
    idx = torch.empty((n, c, ph, pw), device=DEV, dtype=torch.int32)
    ram = torch.full((n, c, ph, pw), float("nan"), device=DEV)
    L.bcnn_hip_maxpool_forward_bn_keep(P(raw), P(yp), P(idx), n, c, oh, ow, ph, pw, 3, 2, P(scales), P(b1),
                                       P(bn["saved_mean"]), P(bn["saved_var"]), a, P(ram))
    dpool = T(n, c, ph, pw) * 0.1
    ws = torch.zeros(max(1, ops.conv_workspace_size(n, cin, oh, ow, c, k, 1, 1, 1)), device=DEV)

    def run(fused):
        g = torch.full((n, c, oh, ow), float("nan"), device=DEV)
        dw1, db1 = torch.zeros_like(w1), torch.zeros_like(b1)
        dsc, dm, dv = Z(), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        if fused:
            assert L.bcnn_hip_maxpool_bn_backward_fusable(n, c, oh, ow, ph, pw, 3, 2, a, P(raw), P(dpool), P(idx), P(g))
            L.bcnn_hip_maxpool_bn_backward(P(dpool), P(idx), P(ram), P(raw), P(g), n, c, oh, ow, ph, pw, 3, 2, P(scales),
                                           P(dsc), P(b1), P(db1), P(bn["saved_mean"]), P(bn["saved_var"]), P(dm), P(dv), a)
        else:
            L.bcnn_hip_maxpool_backward(P(dpool), P(idx), P(g), n, c, oh, ow, ph, pw, 3, 2, 1)
            L.bcnn_hip_conv_backward(P(x0), P(w1), P(b1), P(y1), P(g), 0, P(dw1), P(db1), n, cin, oh, ow, c, k, 1, 1, 1, a,
                                     0, 0, 1, P(scales), P(dsc), P(bn["saved_mean"]), P(bn["saved_var"]), P(dm), P(dv), 0,
                                     P(raw), P(ws), ws.numel())
        torch.cuda.synchronize()
        return g

    _close(run(True), run(False), 1e-5, "dx")
