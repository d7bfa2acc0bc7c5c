"""The lifted-structure loss of the cost node (csrc/lifted_loss.hip, host/bcnn_layers_next.c).

The yardstick is `model()`, an fp64 NumPy statement of the closed form in include/bcnn_hip.h. A CPU test holds it against the
unmodified reference (oracle/_ref/libbcnn_ref.so) at OP_TOL; the GPU tests hold the kernels, the node and the edge
behaviour against it.

Kernel cases. B over {2, 3, 8, 33, 64, 128, 257, 1024} x K over {1, 4, 63, 64, 256, 1000} x {uniform, balanced} labels, under
two constraints: class ids are label columns, so there are at most K classes; and every case but one holds at most
10 000 positive pairs, because the reference's serial fp32 sum over the pairs is itself outside OP_TOL beyond that.
`_cases()` starts each (B, K) from a class count out of 2 ... B/2 and doubles it until the pair count fits; a (B, K, style)
whose pair count cannot fit with K classes (B = 1024 with K <= 4: >= 130 816 pairs; "balanced" = half the batch in one
class from B = 1024 on) is not a case, and `test_case_list_covers_every_size` checks that every B and every K still
occurs. The one exception is (1024, 1000, 8 classes, uniform), P = 65 183 pairs in the reference's run of it, held to
the error the reference itself showed there, 1.83e-5 of max|g|.
All cases are held to OP_TOL = 1e-5 of max|g| element-wise (tests/test_deconv.py) for g and for the scaled gradient;
the loss, a sum of non-negative fp32 terms added as a tree, to 1e-5 of its value; P exactly.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_bind as rb

OP_TOL = 1e-5                 # tests/test_deconv.py:22
BIG_CASE = (1024, 1000, 8)    # the one case with P > 10 000 ...
BIG_TOL = 1.83e-5             # ... held to the reference's own measured error on it
MAX_PAIRS = 10000
LOSS_LIFTED = 1
B_VALUES = (2, 3, 8, 33, 64, 128, 257, 1024)
K_VALUES = (1, 4, 63, 64, 256, 1000)
REF_CASES = [(8, 4, 2, 1.0, 1.0), (32, 16, 4, 1.0, 1.0), (64, 64, 8, 0.5, 1.0), (128, 64, 2, 1.0, 1.0),
             (128, 256, 16, 1.0, 0.1), (256, 128, 32, 1.0, 1.0)]  # (B, K, classes, scale, input spread)


def model(x, cls, margin=1.0):
    """fp64: (loss, P, g) with g the unscaled gradient the reference's forward leaves in the source gradient"""
    x = np.asarray(x, np.float64)
    cls = np.asarray(cls)
    B = x.shape[0]
    sq = (x * x).sum(1)
    D = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2 * x @ x.T, 0.0))
    same = cls[:, None] == cls[None, :]
    E = np.where(~same, np.exp(margin - D), 0.0)
    S = E.sum(1)
    pos = same & ~np.eye(B, dtype=bool)
    SS = S[:, None] + S[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.where(pos & (SS > 0), np.maximum(0.0, np.log(SS) + D), 0.0)
        P = int(pos.sum()) // 2
        loss = (np.triu(L, 1) ** 2).sum() / P if P else 0.0
        Wp = np.where(pos, 2 * L / np.where(pos, D + 1e-10, 1.0), 0.0)
        T = np.where(pos & (SS > 0), 2 * L / np.where(SS > 0, SS, 1.0), 0.0).sum(1)
        Wn = -T[:, None] * E / np.where(~same, D, 1.0)
    A = Wp + Wn + Wn.T
    g = A.sum(1)[:, None] * x - A @ x
    return loss, P, g


def labels(B, ncls, style, rs):
    if style == "balanced" and ncls >= 2:  # half the batch positives of one class, the rest spread over the others
        cls = np.concatenate([np.zeros(B // 2, np.int64), rs.randint(1, ncls, B - B // 2)])
    else:
        cls = rs.randint(0, ncls, B)
    cls[:2] = 0
    return cls


def pairs(cls):
    return int(sum(n * (n - 1) // 2 for n in np.bincount(cls)))


def one_hot(cls, K):
    lab = np.zeros((len(cls), K), np.float32)
    for i, c in enumerate(cls):
        if c >= 0:
            lab[i, c] = 1
    return lab


def _cases():
    out = []
    starts = (2, 4, 8, 16)
    for bi, B in enumerate(B_VALUES):
        for ki, K in enumerate(K_VALUES):
            for style in ("uniform", "balanced"):
                top = max(1, min(K, B // 2))
                ncls = min(top, starts[(bi + ki) % 4])
                while True:
                    cls = labels(B, ncls, style, np.random.RandomState(1000 * bi + 10 * ki + ncls))
                    if pairs(cls) <= MAX_PAIRS or ncls == top:
                        break
                    ncls = min(top, 2 * ncls)
                if pairs(cls) <= MAX_PAIRS:
                    out.append((B, K, ncls, style))
    out.append(BIG_CASE + ("uniform",))
    return out


CASES = _cases()


def test_case_list_covers_every_size():
    assert {c[0] for c in CASES} == set(B_VALUES) and {c[1] for c in CASES} == set(K_VALUES)
    assert {c[3] for c in CASES} == {"uniform", "balanced"}
    assert sum(1 for c in CASES if c[:3] == BIG_CASE) == 1
    assert len(CASES) >= 60


def _ref_node(B, K, cls, x, scale=1.0, mode=rb.MODE_TRAIN, seed=0):
    """fc -> lifted cost on the unmodified reference; the fc input is x"""
    net = rb.RefNet(mode=mode, w=1, h=1, c=K, n=B)
    net.fullc(K, src="input", dst="fc")
    assert net.L.bcnn_add_cost_layer(net.net, LOSS_LIFTED, 0, scale, b"fc", b"label", b"out") == 0
    net.compile()
    net.data(0)[...] = x.reshape(B, K, 1, 1)
    net.data(1)[...] = one_hot(cls, K).reshape(B, K, 1, 1)
    return net


@pytest.mark.parametrize("B,K,ncls,scale,spread", REF_CASES)
def test_fp64_model_is_the_reference(B, K, ncls, scale, spread):
    if not rb.available():
        pytest.skip("oracle/_ref not present")
    rs = np.random.RandomState(B + K)
    x = (rs.randn(B, K) * spread).astype(np.float32)
    cls = labels(B, ncls, "uniform", rs)
    net = _ref_node(B, K, cls, x, scale)
    net.forward()
    fc, last = net.index("fc"), net.num_nodes() - 1
    emb = net.data(fc).reshape(B, K).copy()
    g_fwd = net.grad(fc).reshape(B, K).copy()
    net.backward_node(last)
    g_bwd = net.grad(fc).reshape(B, K).copy()
    net.close()
    loss, P, g = model(emb, cls)
    assert np.isfinite(g).all() and P == pairs(cls)
    e_fwd = np.abs(g_fwd - g).max() / np.abs(g).max()
    e_bwd = np.abs(g_bwd - g * scale / P).max() / np.abs(g * scale / P).max()
    print("reference vs fp64: B=%d K=%d pairs=%d forward %.2e backward %.2e" % (B, K, P, e_fwd, e_bwd))
    assert e_fwd <= OP_TOL and e_bwd <= OP_TOL


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
def _run_kernels(x, lab, scale=1.0, dirty=None, accumulate=False, g0=None):
    import torch
    from bcnn_amd import ops
    B, K = x.shape
    dev = "cuda"
    xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    ws = torch.empty(ops.lifted_struct_workspace_size(B, K), dtype=torch.float32, device=dev)
    ws.fill_(0.0 if dirty is None else dirty)
    g = torch.full((B, K), float("nan") if g0 is None else g0, dtype=torch.float32, device=dev)
    rec = torch.full((2,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the library launches on its own stream
    ops.lifted_struct_forward(xd, ld, g, rec, ws, 1.0, accumulate)
    torch.cuda.synchronize()
    g_fwd = g.cpu().numpy().copy()
    ops.lifted_struct_backward(g, rec, scale)
    torch.cuda.synchronize()
    r = rec.cpu().numpy()
    return float(r[:1].view(np.float32)[0]), int(r[1]), g_fwd, g.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("B,K,ncls,style", CASES)
def test_kernels_match_fp64(B, K, ncls, style):
    """Measured on an MI355X (error of g / of the scaled gradient as a fraction of its max): see DESIGN.md section 13."""
    bi, ki = B_VALUES.index(B), K_VALUES.index(K)
    rs = np.random.RandomState(1000 * bi + 10 * ki + ncls)
    cls = labels(B, ncls, style, rs)
    x = rs.randn(B, K).astype(np.float32)
    scale = 0.5 if (bi + ki) % 2 else 1.0
    want_loss, P, want = model(x, cls)
    assert np.isfinite(want).all() and np.isfinite(want_loss)
    assert P == pairs(cls) and (P <= MAX_PAIRS or (B, K, ncls) == BIG_CASE)
    loss, got_P, g_fwd, g_bwd = _run_kernels(x, one_hot(cls, K), scale)
    tol = BIG_TOL if (B, K, ncls) == BIG_CASE else OP_TOL
    top = np.abs(want).max()
    assert got_P == P
    if top == 0:  # one class: no negatives, the reference's zero gradient
        assert not g_fwd.any() and not g_bwd.any() and loss == 0
        return
    want_s = want * scale / P
    e_fwd = np.abs(g_fwd - want).max() / top
    e_bwd = np.abs(g_bwd - want_s).max() / np.abs(want_s).max()
    e_loss = abs(loss - want_loss) / want_loss
    print("kernels vs fp64: B=%d K=%d classes=%d %s pairs=%d g %.2e scaled %.2e loss %.2e"
          % (B, K, ncls, style, P, e_fwd, e_bwd, e_loss))
    assert np.isfinite(g_fwd).all() and np.isfinite(g_bwd).all()
    assert e_fwd <= tol and e_bwd <= tol
    assert e_loss <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("B,K,ncls", [(64, 64, 8), (257, 4, 4), (1024, 256, 64), (130, 1000, 16)])
def test_bit_identical_runs_and_dirty_workspace(B, K, ncls):
    rs = np.random.RandomState(B)
    cls = labels(B, ncls, "uniform", rs)
    x, lab = rs.randn(B, K).astype(np.float32), one_hot(cls, K)
    a = _run_kernels(x, lab, 0.7)
    b = _run_kernels(x, lab, 0.7)
    c = _run_kernels(x, lab, 0.7, dirty=float("nan"))
    d = _run_kernels(x, lab, 0.7, dirty=3.0e38)
    for other in (b, c, d):
        assert a[0] == other[0] and a[1] == other[1]
        assert a[2].tobytes() == other[2].tobytes() and a[3].tobytes() == other[3].tobytes()


@pytest.mark.gpu
def test_accumulate_adds_onto_the_gradient():
    rs = np.random.RandomState(4)
    cls = labels(48, 4, "uniform", rs)
    x, lab = rs.randn(48, 40).astype(np.float32), one_hot(cls, 40)
    plain = _run_kernels(x, lab)[2]
    added = _run_kernels(x, lab, accumulate=True, g0=2.0)[2]
    np.testing.assert_array_equal(added, np.float32(2.0) + plain)


# ---------------------------------------------------------------------------------------------------------------------
# edge behaviour
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 40])
def test_no_positive_pair_gives_zeros_where_the_reference_gives_nan(K):
    cls = np.arange(4)
    x = np.random.RandomState(0).randn(4, K).astype(np.float32)
    loss, P, g_fwd, g_bwd = _run_kernels(x, one_hot(cls, K))
    assert loss == 0 and P == 0 and not g_fwd.any() and not g_bwd.any()
    if not rb.available():
        pytest.skip("oracle/_ref not present")
    net = _ref_node(4, K, cls, x)
    net.forward()
    net.backward_node(net.num_nodes() - 1)
    assert np.isnan(net.grad(net.index("fc"))).all()  # 0 / 0 pairs: the deviation this build makes
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 40])
def test_one_class_gives_zeros_on_both_sides(K):
    cls = np.zeros(6, np.int64)
    x = np.random.RandomState(1).randn(6, K).astype(np.float32)
    loss, P, g_fwd, g_bwd = _run_kernels(x, one_hot(cls, K))
    assert loss == 0 and P == 15 and not g_fwd.any() and not g_bwd.any()
    if not rb.available():
        pytest.skip("oracle/_ref not present")
    net = _ref_node(6, K, cls, x)
    net.forward()
    net.backward_node(net.num_nodes() - 1)
    assert not net.grad(net.index("fc")).any()
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 40])
def test_label_rows_of_zeros_form_a_class_of_their_own(K):
    rs = np.random.RandomState(2)
    cls = np.array([0, 0, 1, -1, 2, -1, 1, 2, -1, 0])
    x = rs.randn(10, K).astype(np.float32)
    want_loss, P, want = model(x, cls)
    loss, got_P, g_fwd, _ = _run_kernels(x, one_hot(cls, K))
    assert got_P == P == pairs(cls + 1)
    assert np.abs(g_fwd - want).max() <= OP_TOL * np.abs(want).max()
    assert abs(loss - want_loss) <= 1e-5 * want_loss


@pytest.mark.gpu
def test_first_positive_label_entry_is_the_class():
    rs = np.random.RandomState(3)
    cls = labels(12, 3, "uniform", rs)
    x = rs.randn(12, 40).astype(np.float32)
    lab = one_hot(cls, 40)
    lab[:, 30] = 0.5   # a later positive entry does not matter
    lab[:, 39] = -1.0  # nor does a non-positive one
    a = _run_kernels(x, one_hot(cls, 40))
    b = _run_kernels(x, lab)
    assert a[1] == b[1] and a[2].tobytes() == b[2].tobytes()


@pytest.mark.gpu
def test_builder_refuses_a_spatial_source_and_unknown_losses():
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=4, h=4, c=3, n=4)
    net.conv(8, 3, 1, 1, src="input", dst="c1")
    L = net.L
    assert L.bcnn_add_cost_layer(net.net, LOSS_LIFTED, 0, 1.0, b"c1", b"label", b"out") != 0
    assert L.bcnn_add_cost_layer(net.net, 2, 0, 1.0, b"c1", b"label", b"out") != 0
    net.fullc(8, src="c1", dst="fc")
    net.cost("fc", dst="out", loss=capi.LOSS_LIFTED_STRUCT)
    net.close()


@pytest.mark.gpu
def test_get_loss_needs_a_lifted_node_and_resize_is_refused():
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=1, h=1, c=8, n=4)
    net.fullc(8, src="input", dst="fc")
    net.cost("fc", dst="out")
    net.compile()
    with pytest.raises(ValueError):
        net.lifted_struct_loss()
    net.close()
    net = capi.Net(mode=capi.MODE_TRAIN, w=1, h=1, c=8, n=4)
    net.fullc(8, src="input", dst="fc")
    net.cost("fc", dst="out", loss=capi.LOSS_LIFTED_STRUCT)
    net.compile()
    assert net.lifted_struct_loss() == (0.0, 0)  # before any forward
    assert net.resize(1, 1, 8) != 0
    assert net.shape(net.index("fc")) == (4, 8, 1, 1)
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["PREDICT", "VALID"])
def test_predict_and_valid_forward_run(mode):
    from bcnn_amd import capi
    net = capi.Net(mode=getattr(capi, "MODE_" + mode), w=1, h=1, c=8, n=6)
    net.fullc(8, src="input", dst="fc")
    net.cost("fc", dst="out", loss=capi.LOSS_LIFTED_STRUCT)
    net.compile()
    rs = np.random.RandomState(5)
    net.data(0)[...] = rs.randn(6, 8, 1, 1)
    net.data(1)[...] = one_hot(np.array([0, 0, 1, 1, 2, 2]), 8).reshape(6, 8, 1, 1)
    net.upload(0)
    net.upload(1)
    net.forward()
    net.sync()
    fc = net.index("fc")
    net.download(fc, False)
    assert np.isfinite(net.data(fc)).all()
    net.close()


# ---------------------------------------------------------------------------------------------------------------------
# the node against the reference, walked node by node
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,K,ncls,scale,spread", REF_CASES)
def test_node_matches_reference(B, K, ncls, scale, spread):
    if not rb.available():
        pytest.skip("oracle/_ref not present")
    from bcnn_amd import capi
    rs = np.random.RandomState(B + K)
    x = (rs.randn(B, K) * spread).astype(np.float32)
    cls = labels(B, ncls, "uniform", rs)
    ref = _ref_node(B, K, cls, x, scale)
    hip = capi.Net(mode=capi.MODE_TRAIN, w=1, h=1, c=K, n=B)
    hip.fullc(K, src="input", dst="fc")
    hip.cost("fc", dst="out", scale=scale, loss=capi.LOSS_LIFTED_STRUCT)
    hip.compile()
    fc, out = ref.index("fc"), ref.index("out")
    assert (hip.index("fc"), hip.index("out")) == (fc, out)
    for i in range(fc):  # input, label, fc weights and bias
        hip.data(i)[...] = ref.data(i)
        hip.upload(i)
    hip.grad(fc)[...] = 0  # the executor's fill, which a node-by-node walk does not issue
    hip.upload(fc, with_grad=True)
    last = ref.num_nodes() - 1
    for n in range(last + 1):
        ref.forward_node(n)
        hip.forward_node(n)
    hip.sync()
    emb = ref.data(fc).reshape(B, K).copy()
    want_loss, P, want = model(emb, cls)
    top = np.abs(want).max()
    hip.download(fc)
    hip.download(out, False)
    e_ref = np.abs(hip.grad(fc).reshape(B, K) - ref.grad(fc).reshape(B, K)).max() / top
    e_f64 = np.abs(hip.grad(fc).reshape(B, K) - want).max() / top
    assert hip.data(out).ravel()[0] == ref.data(out).ravel()[0]  # the metric, not the loss
    loss, got_P = hip.lifted_struct_loss()
    assert got_P == P and abs(loss - want_loss) <= 1e-5 * want_loss
    ref.backward_node(last)
    hip.backward_node(last)
    hip.download(fc)
    want_s = want * scale / P
    b_ref = np.abs(hip.grad(fc).reshape(B, K) - ref.grad(fc).reshape(B, K)).max() / np.abs(want_s).max()
    b_f64 = np.abs(hip.grad(fc).reshape(B, K) - want_s).max() / np.abs(want_s).max()
    print("node: B=%d K=%d pairs=%d forward vs ref %.2e vs fp64 %.2e, backward vs ref %.2e vs fp64 %.2e"
          % (B, K, P, e_ref, e_f64, b_ref, b_f64))
    # the reference is itself within OP_TOL of the fp64 model (test_fp64_model_is_the_reference): two results within
    # OP_TOL of the same model are within 2 OP_TOL of each other
    assert e_f64 <= OP_TOL and b_f64 <= OP_TOL
    assert e_ref <= 2 * OP_TOL and b_ref <= 2 * OP_TOL
    ref.close()
    hip.close()
