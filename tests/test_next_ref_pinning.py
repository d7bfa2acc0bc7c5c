"""Pins the numpy restatements of tests/_next_ref.py to the unmodified reference (oracle/_ref/libbcnn_ref.so), on the CPU:
one-node eltwise, full-connected and softmax graphs are built through the reference's public API, their tensors are filled
directly, the node alone is run forward and backward (ref_forward_node / ref_backward_node), and the result is compared
with the restatement under the bars the GPU tests hold the HIP kernels to. This is what makes the numpy forms a statement
of the reference and not of the HIP code."""
import numpy as np
import pytest

from oracle import ref_bind as rb
from tests import _golden as G
from tests import _next_ref as R
from tests.test_hip_parity import ACT_TOL, REL_TOL

F32 = np.float32
ACTS = [a for a in range(10) if a != R.ACT_PRELU]


def need_ref():
    if not rb.available():
        pytest.skip("oracle/_ref not present")


def eltwise_net():
    """input (3, 6, 10) x 2 images; p = maxpool 2/2 of it (3, 3, 5); big (5, 6, 10), same (3, 6, 10) and thin (2, 6, 10)
    are 1x1 convolutions of it. Only the eltwise nodes are ever run: their operands are filled directly. The node orders
    its two operands by tensor index (the later tensor first), not by argument order."""
    net = rb.RefNet(mode=rb.MODE_TRAIN, w=10, h=6, c=3, n=2, input_grad=True)
    net.maxpool(2, 2, rb.PADDING_SAME, "input", "p")
    net.conv(5, 1, 1, 0, 1, 0, rb.ACT_NONE, "input", "big")
    net.conv(3, 1, 1, 0, 1, 0, rb.ACT_NONE, "input", "same")
    net.conv(2, 1, 1, 0, 1, 0, rb.ACT_NONE, "input", "thin")
    return net


PAIRS = {  # name: (first argument, second argument)
    "same_shape_batch2": ("same", "input"),        # quirk 5: the second operand reaches image 0 only
    "channel_mismatch": ("big", "thin"),           # same planes, 5 against 2 channels
    "half_size_second": ("big", "p"),              # destination twice the second operand's planes, x_c < y_c
    "half_size_second_swapped": ("p", "big"),      # the same pair in the other argument order
    "half_size_first": ("p", "input"),             # the first operand is the small one: strides the other way
    "half_size_thin": ("thin", "p"),               # x_c > y_c
}


def eltwise_restated(a, b, act, dy, da0, db0):
    """the eltwise node in terms of tests/_next_ref.py: a, b are the operands as (n, c, h, w) arrays"""
    n, yc, yh, yw = a.shape
    _, bc, bh, bw = b.shape
    mind = (min(yc, bc), min(yh, bh), min(yw, bw))
    s0, s1 = max(1, yw // bw), max(1, bw // yw)
    if s0 == 1 and s1 == 1:
        b_count = mind[0] * yh * yw
        y32, y64 = R.eltwise_forward(a.ravel(), b.ravel(), b_count, act)
        g, da, db_head, g64 = R.eltwise_backward(y32, dy.ravel(), da0.ravel(), db0.ravel()[:b_count], b_count, act, 0)
        db = db0.ravel().copy()
        db[:b_count] = db_head
        return y32, y64, g, g64, da, db
    s32, _ = R.axpy_strided(n, 1.0, b, a, s0, s1, b.shape[1:], a.shape[1:], mind)
    y32, y64 = R.act_forward32(s32.ravel(), act), R.act_forward64(s32.ravel(), act)
    g, da, _, g64 = R.eltwise_backward(y32, dy.ravel(), da0.ravel(), None, 0, act, 0)
    db, _ = R.axpy_strided(n, 1.0, g.reshape(a.shape), db0, s1, s0, a.shape[1:], b.shape[1:], mind)
    return y32, y64, g, g64, da, db.ravel()


@pytest.mark.parametrize("act", ACTS, ids=lambda a: R.ACT_NAMES[a])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_eltwise_restatement_matches_the_reference(pair, act):
    need_ref()
    net = eltwise_net()
    node = net.eltwise(act, PAIRS[pair][0], PAIRS[pair][1], "out")
    net.compile()
    ia, ib, iy = net.node_src(node, 0), net.node_src(node, 1), net.node_dst(node)
    rs = np.random.RandomState(len(pair) + act)
    u = lambda shape: rs.uniform(-1, 1, shape).astype(F32)
    a, b = u(net.shape(ia)), u(net.shape(ib))
    a.ravel()[::7] = F32(0)
    dy, da0, db0 = u(net.shape(iy)), u(net.shape(ia)), u(net.shape(ib))
    assert net.shape(iy) == a.shape
    net.data(ia)[...] = a
    net.data(ib)[...] = b
    net.forward_node(node)
    y_ref = net.data(iy).copy()
    net.grad(iy)[...] = dy
    net.grad(ia)[...] = da0
    net.grad(ib)[...] = db0
    net.backward_node(node)
    g_ref, da_ref, db_ref = net.grad(iy).copy(), net.grad(ia).copy(), net.grad(ib).copy()
    net.close()

    y32, y64, g, g64, da, db = eltwise_restated(a, b, act, dy, da0, db0)
    tag = "ref/eltwise/%s/%s" % (pair, R.ACT_NAMES[act])
    R.assert_bar(R.FWD_BAR[act], tag + "/y", y_ref, y32, y64, ACT_TOL)
    # backward from the reference's own y (it may differ from the restated y within the forward bar)
    y_in = y_ref.ravel()
    g, _, _, g64 = R.eltwise_backward(y_in, dy.ravel(), None, None, 0, act, 0)
    R.assert_bar(R.BWD_BAR[act], tag + "/dy", g_ref, g, g64, ACT_TOL)
    # the two accumulations are single float32 adds of the stored g
    _, _, _, _, da, db = eltwise_restated(a, b, R.ACT_NONE, g_ref, da0, db0)
    R.assert_bits(tag + "/da", da_ref, da)
    R.assert_bits(tag + "/db", db_ref, db)


def test_quirk5_is_visible_in_the_same_shape_case():
    """the restatement adds the second operand to image 0 only: with batch 2 the second image is act(a) alone"""
    a = np.full((2, 3, 6, 10), 1.0, F32)
    b = np.full((2, 3, 6, 10), 2.0, F32)
    y32, _ = R.eltwise_forward(a.ravel(), b.ravel(), 3 * 60, R.ACT_NONE)
    assert np.all(y32[:180] == 3.0) and np.all(y32[180:] == 1.0)


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_RELU, R.ACT_LOGISTIC], ids=lambda a: R.ACT_NAMES[a])
def test_fullc_restatement_matches_the_reference(act):
    """y = act(x W^T + b) is bcnn_hip_gemm(0, 1) + add_rowvec + activation with spatial = 1; backward is the activation
    backward, db += column sums, dW += dy^T x (gemm(1, 0)) and dx += dy W (gemm(0, 0))"""
    need_ref()
    B, S, P = 5, 8 * 8 * 8, 37
    net = rb.RefNet(mode=rb.MODE_TRAIN, w=8, h=8, c=8, n=B, input_grad=True)
    node = net.fullc(P, act, "input", "fc")
    net.compile()
    ix, iw, ib, iy = net.node_src(node, 0), net.node_src(node, 1), net.node_src(node, 2), net.node_dst(node)
    rs = np.random.RandomState(act)
    u = lambda shape: rs.uniform(-1, 1, shape).astype(F32)
    x, w, bias = u((B, S)), u((P, S)), u(P)
    net.data(ix)[...] = x.reshape(net.shape(ix))
    net.data(iw)[...] = w.reshape(net.shape(iw))
    net.data(ib)[...] = bias.reshape(net.shape(ib))
    net.forward_node(node)
    y_ref = net.data(iy).reshape(B, P).copy()
    dy, dx0, dw0, db0 = u((B, P)), u((B, S)), u((P, S)), u(P)
    net.grad(iy)[...] = dy.reshape(net.shape(iy))
    net.grad(ix)[...] = dx0.reshape(net.shape(ix))
    net.grad(iw)[...] = dw0.reshape(net.shape(iw))
    net.grad(ib)[...] = db0.reshape(net.shape(ib))
    net.backward_node(node)
    g_ref = net.grad(iy).reshape(B, P).copy()
    dx_ref, dw_ref, db_ref = net.grad(ix).reshape(B, S).copy(), net.grad(iw).reshape(P, S).copy(), net.grad(ib).ravel().copy()
    net.close()

    def close(tag, got, want, bound):
        G.assert_close(tag, got, want, REL_TOL)
        assert np.all(np.abs(got.astype(np.float64) - want) <= bound), tag

    tag = "ref/fullc/%s" % R.ACT_NAMES[act]
    rows = np.tile(bias, (B, 1))                         # gemm with beta = 1 on top of the bias rows == gemm, then add_rowvec
    pre, bound = R.gemm64(0, 1, B, P, S, 1.0, x, w, 1.0, rows)
    if act == R.ACT_NONE:
        close(tag + "/y", y_ref, pre, bound)
    else:                                                # both activations are 1-Lipschitz: the gemm bound carries over
        close(tag + "/y", y_ref, R.act_forward64(pre.astype(F32), act), bound + ACT_TOL * np.abs(pre) + 2.0 ** -23)
    g, _, _, g64 = R.eltwise_backward(y_ref.ravel(), dy.ravel(), None, None, 0, act, 0)
    R.assert_bar(R.BWD_BAR[act], tag + "/dy", g_ref, g, g64, ACT_TOL)
    g_ref64 = g_ref.astype(np.float64)
    G.assert_close(tag + "/db", db_ref, db0 + g_ref64.sum(axis=0), REL_TOL)
    want, bound = R.gemm64(1, 0, P, S, B, 1.0, g_ref, x, 1.0, dw0)
    close(tag + "/dw", dw_ref, want, bound)
    want, bound = R.gemm64(0, 0, B, S, P, 1.0, g_ref, w, 1.0, dx0)
    close(tag + "/dx", dx_ref, want, bound)


SOFTMAX_SHAPES = [(n, c, hw) for c in (1, 2, 10, 63, 64, 65, 130, 1000) for hw in (1, 5, 49) for n in (1, 3)] + [(3, 5, 3000)]


def test_softmax_reference_order_stays_inside_the_bound():
    """the bound the HIP kernel is held to must not hide it behind the reference's own error: the reference's order of
    operations, restated, is inside it for every input the GPU test uses"""
    worst = 0.0
    for n, c, hw in SOFTMAX_SHAPES:
        x = R.softmax_inputs(n, c, hw, 100 * c + hw + n)
        assert np.all(np.isfinite(x))
        y, _ = R.softmax_ref_order(x)
        worst = max(worst, R.check_softmax(y, x, "restated/n%d_c%d_hw%d" % (n, c, hw)))
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("c,h,w,n", [(10, 1, 1, 3), (65, 1, 1, 7), (130, 7, 7, 1), (5, 5, 1, 3), (1000, 1, 1, 7)])
def test_softmax_restatement_matches_the_reference(c, h, w, n):
    need_ref()
    net = rb.RefNet(mode=rb.MODE_TRAIN, w=w, h=h, c=c, n=n)
    node = net.softmax("input", "sm")
    net.compile()
    x = R.softmax_inputs(n, c, h * w, c + n)
    net.data(0)[...] = x.reshape(net.shape(0))
    net.forward_node(node)
    y_ref = net.data(net.node_dst(node)).reshape(n, c, h * w).copy()
    net.close()
    R.check_softmax(y_ref, x, "ref/softmax")
    y, _ = R.softmax_ref_order(x)
    same = R.bits(y) == R.bits(y_ref)
    # numpy's exp / log and the C library's may differ in the last bit of a double, which a float conversion shows rarely
    assert same.mean() >= 0.99, same.mean()
    assert np.all(np.abs(y.astype(np.float64) - y_ref) <= R.softmax_bound(x) * R.softmax64(x))
