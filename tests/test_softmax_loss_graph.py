"""The softmax-loss node inside nets (bcnn_amd.capi): the segmentation head of tests/test_interp_graph.py ending in the
new node, built by builder calls and from an INI string under both section names,

    input 2x3x17x17 -> conv 3x3 (8) -> dilated conv 3x3 d2 (8, groups 2, ReLU) -> conv 1x1 (5)
                    -> interp zoom 4, align_corners (65x65) -> softmax_loss on a [2][1][65][65] class-index map,

with ignore label 255 on about a fifth of the pixels, in blocks.

Against the same graph in torch float64 on the net's weights (F.cross_entropy, ignore_index=255): the probabilities and
the gradient at the first convolution's output at the project's net-level bar (1e-4 of the tensor's maximum,
tests/test_net_parity.py); the counts exactly; the loss at the operator test's bound, which is a bound against float64
ON THE SAME LOGITS, so its reference is tests/_softmax_loss_ref.py on the logits the net computed (and torch's loss, on
its own float64 logits, at the net-level bar).

Then: the chain it replaces (softmax -> Euclidean cost on the dense one-hot label) gives the same gradient with
BCNN_LOSS_NORM_NONE; a second consumer of the logits selects the add form and a sole consumer gets no zero fill; one
SGD step moves the weights as torch's gradient says; a PREDICT net writes the same probabilities and has no statistics
(the getter returns BCNN_INVALID_PARAMETER); bcnn_resize_net moves output and label; a model-file round trip."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _next_ref as N
from tests import _softmax_loss_ref as R

pytestmark = pytest.mark.gpu
NET_TOL = 1e-4  # tests/test_net_parity.py
SEED = 20261021
SHP = dict(w=17, h=17, c=3, n=2)
CLASSES = 5
IGNORE = 255


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


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def _compare(tag, a, b, tol=NET_TOL):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a64.shape == b64.shape, (tag, a64.shape, b64.shape)
    assert np.isfinite(a64).all(), tag
    diff = float(np.max(np.abs(a64 - b64)))
    print("%s: max abs diff %.3g of max %.3g" % (tag, diff, float(np.max(np.abs(b64)))))
    assert diff <= tol * float(np.max(np.abs(b64))) + 1e-7, "%s: max abs diff %.3g" % (tag, diff)


def _data(net, idx):
    net.download(idx, False)
    return net.data(idx).copy()


def _grad(net, idx):
    net.download(idx, True)
    return net.grad(idx).copy()


def _head(mode, loss="softmax_loss", side=False, seed=SEED, normalize="valid_per_image", ignore=IGNORE, scale=1.0):
    """the head by builder calls. loss: "softmax_loss", or "chain" for softmax -> Euclidean cost; side: a second consumer
    of the logits, outside the loss. Returns (net, the loss node's index)"""
    from bcnn_amd import capi
    C.CDLL(None).srand(seed)   # the fillers draw from rand()
    net = capi.Net(mode=mode, **SHP)
    net.conv(8, 3, 1, 1, act=capi.ACT_NONE, src="input", dst="c1")
    net.dilated_conv(8, 3, 1, 2, 2, g=2, act=capi.ACT_RELU, src="c1", dst="dc")
    net.conv(CLASSES, 1, 1, 0, act=capi.ACT_NONE, src="dc", dst="c3")
    net.interp("c3", "up", zoom=4, align_corners=True)
    if side:
        net.pool2d("avg", 2, 2, 0, src="up", dst="side")
    if loss == "chain":
        net.softmax("up", "prob")
        node = net.cost("prob", "label", "cost")
    else:
        node = net.softmax_loss("up", "prob", ignore_label=ignore, normalize=normalize, scale=scale)
    net.compile()
    return net, node


HEAD_CFG = """
[net]
input_width=17
input_height=17
input_channels=3
batch_size=2

[conv]
filters=8
size=3
stride=1
pad=1
activation=linear
src=input
dst=c1

[conv]
filters=8
size=3
stride=1
pad=2
dilation=2
groups=2
activation=relu
src=c1
dst=dc

[conv]
filters=5
size=1
stride=1
pad=0
activation=linear
src=dc
dst=c3

[interp]
zoom=4
align_corners=1
src=c3
dst=up

[%s]
ignore_label=255
src=up
dst=prob
"""


def _label_map(seed=7):
    """class indices with 255 on six blocks of up to 17 x 17 pixels: 1632 of the 2 x 65 x 65 pixels, about a fifth"""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, CLASSES, (SHP["n"], 65, 65)).astype(np.float32)
    for b, (i, j) in enumerate([(3, 40), (30, 5)]):
        lab[b, i:i + 17, j:j + 17] = IGNORE
        lab[b, 46:63, 20 + 9 * b:37 + 9 * b] = IGNORE
        lab[1 - b, 0:17, 0:17 - 6 * b] = IGNORE
    return lab


def _feed(net, dense=False, ignore=True, seed=7):
    rs = np.random.RandomState(seed)
    for node in range(3):   # non-trivial biases (the builders fill 0)
        i = net.node_src(node, 2)
        net.data(i)[...] = rs.uniform(-0.5, 0.5, net.shape(i))
        net.upload(i)
    net.data(0)[...] = rs.uniform(-1, 1, net.shape(0))
    net.upload(0)
    lab = _label_map(seed)
    if not ignore:
        lab = np.where(lab == IGNORE, 2.0, lab).astype(np.float32)
    if dense:   # the one-hot label of the chain
        assert net.shape(1) == (SHP["n"], CLASSES, 65, 65)
        one = np.zeros(net.shape(1), np.float32)
        np.put_along_axis(one, lab.astype(np.int64)[:, None], 1.0, axis=1)
        net.data(1)[...] = one
    else:
        assert net.shape(1) == (SHP["n"], 1, 65, 65)
        net.data(1)[...] = lab[:, None]
    net.upload(1)
    return lab


def _torch_head(net, lab, D, scale=1.0):
    """the same graph in float64 on the net's weights; returns dict(p, loss, c1 gradient, weight and bias gradients)"""
    t = lambda i: torch.tensor(_data(net, i), dtype=torch.float64)
    w = [t(net.node_src(k, 1)).requires_grad_(True) for k in range(3)]
    b = [t(net.node_src(k, 2)).reshape(-1).requires_grad_(True) for k in range(3)]
    c1 = F.conv2d(t(0), w[0].reshape(8, 3, 3, 3), b[0], padding=1)
    c1.retain_grad()
    dc = F.relu(F.conv2d(c1, w[1].reshape(8, 4, 3, 3), b[1], padding=2, dilation=2, groups=2))
    c3 = F.conv2d(dc, w[2].reshape(CLASSES, 8, 1, 1), b[2])
    up = F.interpolate(c3, size=(65, 65), mode="bilinear", align_corners=True)
    loss = F.cross_entropy(up, torch.tensor(lab.astype(np.int64)), ignore_index=IGNORE, reduction="sum") / D
    (scale * loss).backward()
    return dict(p=F.softmax(up, dim=1).detach().numpy(), loss=float(loss.detach()), c1=c1.grad.numpy(),
                dw=[x.grad.numpy() for x in w], db=[x.grad.numpy() for x in b])


def _loss_bound(logits, ref):
    """the operator test's loss bound (tests/test_softmax_loss.py) for float32 logits (n, C, HW)"""
    B = N.softmax_bound(logits)
    valid = ref["kind"] == R.VALID
    Bt = np.take_along_axis(B, np.where(valid, ref["cls"], 0)[:, None, :], axis=1)[:, 0, :]
    return float(np.where(valid, Bt, 0.0).sum()) / ref["D"] + 2.0 ** -24 * abs(ref["loss"])


def _check_forward(net, node, lab, norm=R.NORM_VALID_PER_IMAGE):
    """probabilities, statistics and confusion matrix of the latest forward against the restatement on the net's logits"""
    n, c, h, w = net.shape(net.index("up"))
    logits = _data(net, net.index("up")).reshape(n, c, h * w)
    ref = R.reference(logits, lab.reshape(n, h * w), IGNORE, norm)
    N.check_softmax(_data(net, net.index("prob")).reshape(n, c, h * w), logits, "probabilities")
    stats = net.softmax_loss_stats(node)
    for name in ("valid", "ignored", "out_of_range", "correct"):
        assert stats[name] == ref[name], (name, stats[name], ref[name])
    err, bound = abs(stats["loss"] - ref["loss"]), _loss_bound(logits, ref)
    print("loss %.7g, float64 on the same logits %.7g: err %.3e, bound %.3e" % (stats["loss"], ref["loss"], err, bound))
    assert err <= bound
    conf = net.confusion_matrix(node)
    assert np.array_equal(conf, ref["confusion"]) and conf.trace() == stats["correct"] and conf.sum() == stats["valid"]
    return ref, stats


@pytest.mark.parametrize("how", ["builders", "ini-softmax_loss", "ini-softmaxwithloss"])
def test_segmentation_head_against_torch(tmp_path, how):
    from bcnn_amd import capi
    if how == "builders":
        net, node = _head(capi.MODE_TRAIN)
    else:
        cfg = tmp_path / "head.cfg"
        cfg.write_text(HEAD_CFG % how[4:])
        C.CDLL(None).srand(SEED)
        net, node = capi.Net.load_net(str(cfg), None, mode=capi.MODE_TRAIN), 4
        net.compile()
    assert net.num_nodes == 5 and net.node_type(node) == capi.LAYER_SOFTMAX_LOSS == 22
    up, prob, c1 = net.index("up"), net.index("prob"), net.index("c1")
    assert net.node_src(node, 0) == up and net.node_src(node, 1) == 1 and net.node_dst(node) == prob
    assert net.shape(prob) == (2, CLASSES, 65, 65) and net.shape(1) == (2, 1, 65, 65)
    lab = _feed(net)
    _trace(True)
    net.forward()
    net.backward()
    net.sync()
    ran = _trace(False)
    assert "softmax_loss_fwd_pixels_reg" in ran and "softmax_loss_finalize" in ran, ran   # 4225 pixels: the scalar form
    assert "softmax_loss_bwd:overwrite" in ran and "softmax_loss_bwd" not in ran, ran      # the only writer of up's gradient
    assert "softmax_kernel" not in ran
    ref, stats = _check_forward(net, node, lab)
    assert stats["ignored"] == 1632 and 0.15 < stats["ignored"] / lab.size < 0.25 and stats["out_of_range"] == 0
    want = _torch_head(net, lab, ref["D"])
    assert ref["D"] == ref["valid"] / 2.0
    _compare("probabilities", _data(net, prob), want["p"])
    _compare("gradient at the first convolution's output", _grad(net, c1), want["c1"])
    _compare("loss against torch", [stats["loss"]], [want["loss"]])
    if how != "builders":   # the file builds the graph the builder calls build: the same bits on the same weights
        twin, tnode = _head(capi.MODE_TRAIN)
        _feed(twin)
        twin.forward()
        twin.backward()
        twin.sync()
        assert np.array_equal(_bits(_data(net, prob)), _bits(_data(twin, twin.index("prob"))))
        assert np.array_equal(_bits(_grad(net, c1)), _bits(_grad(twin, twin.index("c1"))))
        assert twin.softmax_loss_stats(tnode) == stats
        twin.close()
    net.close()


def test_norm_none_is_the_softmax_cost_chain():
    """no ignored pixel, D = 1: p - y arrives at the logits either way, so the gradient at the first convolution's output
    agrees with the net that ends in softmax -> cost on the dense one-hot label"""
    from bcnn_amd import capi
    new, node = _head(capi.MODE_TRAIN, normalize="none")
    old, _ = _head(capi.MODE_TRAIN, loss="chain")
    _feed(new, ignore=False)
    _feed(old, dense=True, ignore=False)
    grads = []
    for net in (new, old):
        net.forward()
        net.backward()
        net.sync()
        grads.append((_data(net, net.index("prob")), _grad(net, net.index("up")), _grad(net, net.index("c1"))))
    assert new.softmax_loss_stats(node)["ignored"] == 0
    _compare("probabilities, node against chain", grads[0][0], grads[1][0])
    _compare("gradient at the logits, node against chain", grads[0][1], grads[1][1])
    _compare("gradient at the first convolution's output, node against chain", grads[0][2], grads[1][2])
    assert np.abs(grads[1][2]).max() > 0
    new.close()
    old.close()


def test_second_consumer_selects_the_add_form_and_a_sole_consumer_needs_no_fill():
    """The fills of a pass are issued at the start of the forward. A poisoned gradient of the logits therefore survives the
    forward when the loss node is its only consumer (no fill: the overwrite form will write every element) and is zero
    after it when a second node reads the logits. The side branch is outside the loss, its gradient is zero, so both
    forms give the same gradient at the logits and below, bit for bit (0 + g and g + 0 are exact)."""
    from bcnn_amd import capi
    got = {}
    for side in (False, True):
        net, node = _head(capi.MODE_TRAIN, side=side)
        _feed(net)
        up = net.index("up")
        net.grad(up)[...] = 123.0
        net.upload(up, with_grad=True)
        net.forward()
        net.sync()
        after_forward = _grad(net, up)
        assert bool((after_forward == (0.0 if side else 123.0)).all()), side
        _trace(True)
        net.backward()
        net.sync()
        ran = _trace(False)
        assert ("softmax_loss_bwd" in ran) == side and ("softmax_loss_bwd:overwrite" in ran) == (not side), ran
        got[side] = (_grad(net, up), _grad(net, net.index("c1")))
        net.close()
    assert np.abs(got[False][0]).max() > 0
    lab = _label_map()
    ignored = np.broadcast_to((lab == IGNORE)[:, None], got[False][0].shape)
    assert bool((_bits(got[False][0])[ignored] == 0).all())   # +0.0 on every ignored pixel
    for a, b in zip(got[False], got[True]):
        assert np.array_equal(_bits(a), _bits(b))


def test_one_sgd_step_moves_the_weights_as_torch_says():
    """forward / backward / update (bcnn_train_on_batch without its loader): the step's loss, read through the stats, is
    the reference value, and w -= lr / batch * dw with torch's dw. valid_per_image: D = V / n, so lr / batch * dw is lr
    times the gradient of the mean over the valid pixels."""
    from bcnn_amd import capi
    lr = 0.5
    net, node = _head(capi.MODE_TRAIN, scale=0.5)
    net.set_sgd(lr, 0.0, 0.0)
    lab = _feed(net)
    ids = [(net.node_src(k, 1), net.node_src(k, 2)) for k in range(3)]
    before = [(_data(net, w), _data(net, b)) for w, b in ids]
    net.forward()
    net.backward()
    ref, stats = _check_forward(net, node, lab)
    want = _torch_head(net, lab, ref["D"], scale=0.5)
    _compare("the step's loss", [stats["loss"]], [want["loss"]])
    mean = F.cross_entropy(torch.tensor(_data(net, net.index("up")), dtype=torch.float64),
                           torch.tensor(lab.astype(np.int64)), ignore_index=IGNORE, reduction="mean")
    _compare("valid_per_image: the loss is batch x the mean over valid pixels", [stats["loss"]], [SHP["n"] * float(mean)])
    net.update()
    net.sync()
    for k, (w, b) in enumerate(ids):
        _compare("weights of node %d after the step" % k, _data(net, w) - before[k][0],
                 -lr / SHP["n"] * want["dw"][k].reshape(before[k][0].shape))
        _compare("biases of node %d after the step" % k, _data(net, b) - before[k][1],
                 -lr / SHP["n"] * want["db"][k].reshape(before[k][1].shape))
    net.close()


def test_predict_net_writes_the_same_probabilities_and_has_no_statistics():
    from bcnn_amd import capi
    outs = {}
    for mode in (capi.MODE_TRAIN, capi.MODE_VALID, capi.MODE_PREDICT):
        net, node = _head(mode)
        if mode == capi.MODE_PREDICT:   # no label is written: the input and the biases alone
            rs = np.random.RandomState(7)
            for k in range(3):
                i = net.node_src(k, 2)
                net.data(i)[...] = rs.uniform(-0.5, 0.5, net.shape(i))
                net.upload(i)
            net.data(0)[...] = rs.uniform(-1, 1, net.shape(0))
            net.upload(0)
        else:
            _feed(net)
        _trace(True)
        net.forward()
        net.sync()
        ran = _trace(False)
        assert ("softmax_loss_finalize" in ran) == (mode != capi.MODE_PREDICT), ran
        outs[mode] = _data(net, net.index("prob"))
        if mode == capi.MODE_PREDICT:
            out = capi.SoftmaxLossStats(loss=5.0, valid=3)
            assert net.L.bcnn_get_softmax_loss_stats(net.net, node, C.byref(out)) == 1   # BCNN_INVALID_PARAMETER
            assert out.loss == 0.0 and out.valid == 0
            with pytest.raises(ValueError):
                net.softmax_loss_stats(node)
        else:
            assert net.softmax_loss_stats(node)["valid"] > 0
        net.close()
    assert np.abs(outs[capi.MODE_TRAIN]).max() > 0
    for mode in (capi.MODE_VALID, capi.MODE_PREDICT):
        assert np.array_equal(_bits(outs[capi.MODE_TRAIN]), _bits(outs[mode]))


def _tail(w, h, n, mode=None):
    """conv -> softmax_loss on 6 classes (a graph bcnn_resize_net takes: no dilated node)"""
    from bcnn_amd import capi
    C.CDLL(None).srand(SEED)
    net = capi.Net(mode=capi.MODE_TRAIN if mode is None else mode, w=w, h=h, c=3, n=n)
    net.conv(6, 3, 1, 1, act=capi.ACT_NONE, src="input", dst="c1")
    node = net.softmax_loss("c1", "prob", ignore_label=IGNORE, normalize="valid")
    net.compile()
    return net, node


def test_resize_moves_the_output_and_the_label_map():
    net, node = _tail(12, 10, 2)
    assert net.shape(net.index("prob")) == (2, 6, 10, 12) and net.shape(1) == (2, 1, 10, 12)
    # larger than the label's allocation (240 floats) and no need_realloc: refused in the plan, nothing moved
    assert net.resize(19, 15, 3, need_realloc=False) == 1   # BCNN_INVALID_PARAMETER
    assert net.shape(0) == (2, 3, 10, 12) and net.shape(1) == (2, 1, 10, 12) and net.shape(net.index("prob")) == (2, 6, 10, 12)
    # within it: shapes follow, nothing is re-allocated
    assert net.resize(9, 7, 3, need_realloc=False) == 0
    assert net.shape(1) == (1, 1, 7, 9) and net.shape(net.index("prob")) == (1, 6, 7, 9)
    # past it with need_realloc
    assert net.resize(19, 15, 3, need_realloc=True) == 0
    fresh, fnode = _tail(19, 15, 1)
    rs = np.random.RandomState(3)
    x = rs.uniform(-1, 1, (1, 3, 15, 19))
    lab = rs.randint(0, 6, (1, 1, 15, 19)).astype(np.float32)
    lab[0, 0, 4:9, 3:11] = IGNORE
    lab[0, 0, 0, 0] = 6.0   # out of range
    for t, nd in ((net, node), (fresh, fnode)):
        assert t.shape(t.index("prob")) == (1, 6, 15, 19) and t.shape(1) == (1, 1, 15, 19)
        t.data(0)[...] = x
        t.upload(0)
        t.data(1)[...] = lab
        t.upload(1)
        t.forward()
        t.backward()   # in bounds on the re-allocated tensors
        t.sync()
    logits = _data(net, net.index("c1")).reshape(1, 6, 15 * 19)
    ref = R.reference(logits, lab.reshape(1, -1), IGNORE, R.NORM_VALID)
    N.check_softmax(_data(net, net.index("prob")).reshape(1, 6, -1), logits, "resized")
    stats = net.softmax_loss_stats(node)
    assert (stats["valid"], stats["ignored"], stats["out_of_range"]) == (15 * 19 - 41, 40, 1)
    assert stats["correct"] == ref["correct"] and abs(stats["loss"] - ref["loss"]) <= _loss_bound(logits, ref)
    assert stats == fresh.softmax_loss_stats(fnode)
    for name in ("prob", "c1"):
        a, b = _data(net, net.index(name)), _data(fresh, fresh.index(name))
        assert np.abs(b).max() > 0 and np.array_equal(_bits(a), _bits(b)), name
    assert np.array_equal(_bits(_grad(net, net.index("c1"))), _bits(_grad(fresh, fresh.index("c1"))))
    net.close()
    fresh.close()


def test_model_file_round_trip_with_the_node_in_the_graph(tmp_path):
    from bcnn_amd import capi
    a, node = _head(capi.MODE_TRAIN)
    _feed(a)
    a.forward()
    a.sync()
    path = str(tmp_path / "head.bcnnmodel")
    assert a.save_weights(path) == 0
    b, bnode = _head(capi.MODE_TRAIN, seed=SEED + 1)   # other weights, until the file is loaded
    assert b.node_type(bnode) == capi.LAYER_SOFTMAX_LOSS
    assert b.load_weights(path) == 0
    b.data(0)[...] = a.data(0)   # input and label alone: weights and biases came from the file
    b.upload(0)
    b.data(1)[...] = a.data(1)
    b.upload(1)
    b.forward()
    b.sync()
    for name in ("c3", "up", "prob"):
        assert np.array_equal(_bits(_data(a, a.index(name))), _bits(_data(b, b.index(name)))), name
    assert a.softmax_loss_stats(node) == b.softmax_loss_stats(bnode)
    a.close()
    b.close()
