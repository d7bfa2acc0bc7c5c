"""The dice-loss node inside nets (bcnn_amd.capi): a 1x1 convolution into [dice_loss] against torch float64 autograd,
bcnn_resize_net, PREDICT mode, the config keys, and Swin-UNet's 0.4 CE + 0.6 Dice on a small Swin-UNet-shaped graph."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_dice_loss import BITS, IGNORE, U, reference
from tests.test_group_norm_net import _data, _feed, _grad

pytestmark = pytest.mark.gpu
SEED = 20261128
HEAD = "[net]\ninput_width=%d\ninput_height=%d\ninput_channels=%d\nbatch_size=2\n\n"
CONV = "filters=%d\nsize=%d\nstride=%d\npad=0\nactivation=linear\n"


def _sections(*sections):
    return "".join("[%s]\n%ssrc=%s\ndst=%s\n\n" % s for s in sections)


TINY = HEAD % (8, 8, 3) + _sections(("conv", CONV % (5, 1, 1), "input", "out"), ("dice_loss", "ignore_label=%d\n" % IGNORE, "out", "prob"))
# tests/test_swin_unet_net.py's graph with Swin-UNet's objective at its end: embedding, norm, merge, two expands, a skip
UNET = HEAD % (16, 16, 3) + _sections(
    ("conv", CONV % (4, 4, 4), "input", "emb"), ("channelnorm", "", "emb", "ln"), ("patch_merging", "", "ln", "pm"),
    ("conv", CONV % (8, 1, 1), "pm", "d"), ("conv", CONV % (16, 1, 1), "d", "e"), ("patch_expanding", "", "e", "u"),
    ("route", "", "u,ln", "cat"), ("conv", CONV % (4, 1, 1), "cat", "f"), ("conv", CONV % (64, 1, 1), "f", "g"),
    ("patch_expanding", "block=4\n", "g", "v"), ("conv", CONV % (3, 1, 1), "v", "out"),
    ("dice_loss", "ce_weight=0.4\ndice_weight=0.6\n", "out", "prob"))


def _load(tmp_path, text, mode):
    from bcnn_amd import capi
    cfg = tmp_path / "net.cfg"
    cfg.write_text(text)
    C.CDLL(None).srand(SEED)
    net = capi.Net.load_net(str(cfg), None, mode=mode)
    net.compile()
    return net


def _feed_classes(net, seed, classes, stripe=None):
    _feed(net, seed, label=False)
    lab = np.random.RandomState(seed).randint(0, classes, net.shape(1)).astype(np.float32)
    if stripe is not None:
        lab[:, :, stripe, :] = IGNORE
    net.data(1)[...] = lab
    net.upload(1)
    return lab


def test_one_train_step_against_torch_float64_autograd(tmp_path):
    """the loss within the operator test's bound; dW within that test's dx bound summed over the n h w products of the
    1x1 convolution: N max|x| (tol_dx + (8 max|logit| + 4) u max|dx|), the second term for float32 logits and sums"""
    from bcnn_amd import capi
    net = _load(tmp_path, TINY, capi.MODE_TRAIN)
    assert net.num_nodes == 2 and net.node_type(1) == capi.LAYER_DICE_LOSS and net.shape(1) == (2, 1, 8, 8)
    lab = _feed_classes(net, 5, 5, stripe=3)
    net.set_sgd(0.1, 0.0)
    net.forward()
    net.backward()
    net.sync()
    stats, sums = net.dice_loss_stats(1), net.dice_loss_sums(1)
    x, logits = net.data(0).copy(), _data(net, net.index("out"))
    w, b = (torch.tensor(_data(net, net.node_src(0, s)).astype(np.float64), requires_grad=True) for s in (1, 2))
    out = F.conv2d(torch.tensor(x.astype(np.float64)), w.reshape(5, 3, 1, 1), b.ravel())
    t = torch.tensor(lab[:, 0].astype(np.int64))
    valid = (t != IGNORE)[:, None].double()
    onehot = F.one_hot(torch.where(t == IGNORE, 0, t), 5).permute(0, 3, 1, 2).double() * valid
    p = out.softmax(1)
    I, Z, Y = ((a * valid).sum((0, 2, 3)) for a in (p * onehot, p * p, onehot))
    s = float(np.float32(1e-5))
    loss = float(np.float32(0.4)) * F.cross_entropy(out, t, ignore_index=IGNORE) + float(np.float32(0.6)) * (1 - (2 * I + s) / (Z + Y + s)).mean()
    loss.backward()
    loss = loss.detach()
    ref = reference(logits.reshape(2, 5, 64), lab.reshape(2, 64), IGNORE, float(np.float32(0.4)), float(np.float32(0.6)), s, True, "batch")
    assert stats["valid"] == 2 * 56 and stats["ignored"] == 16 and np.array_equal(sums[..., 2], ref["izy"][..., 2])
    e_p, L = 8 * U, 1
    r_I, r_Z = e_p + (L + 10) * U, 2 * e_p + (L + 11) * U
    assert abs(stats["loss"] - float(loss)) <= 0.4 * (23 * U + U * ref["ce"]) + 0.6 * (r_I + r_Z + U) + U * float(loss) + 16 * U
    gamma, top = float((np.abs(ref["A"]) + 2 * np.abs(ref["B"])).max()), float(np.abs(ref["dx"]).max())
    tol_dx = 0.6 * 2 * gamma * (r_I + 2 * r_Z + 3 * e_p + 15 * U) + 0.4 / 112 * (e_p + 3 * U) + 2 * U * top
    tol_w = 128 * float(np.abs(x).max()) * (tol_dx + (8 * float(np.abs(logits).max()) + 4) * U * top)
    err = float(np.abs(_grad(net, net.node_src(0, 1)).ravel() - w.grad.numpy().ravel()).max())
    print("dW err %.3e, bound %.3e, max|dW| %.3e" % (err, tol_w, float(w.grad.abs().max())))
    assert float(w.grad.abs().max()) > 0 and err <= tol_w
    net.update()   # the step completes; a second forward sees other weights
    net.forward()
    net.sync()
    assert net.dice_loss_stats(1)["loss"] != stats["loss"]
    net.close()


def test_resize_and_back_the_label_follows(tmp_path):
    from bcnn_amd import capi
    net = _load(tmp_path, TINY, capi.MODE_TRAIN)
    assert net.resize(12, 12, 3, need_realloc=False) == 1 and net.shape(1) == (2, 1, 8, 8), "the label would outgrow its allocation"
    assert net.resize(12, 12, 3, need_realloc=True) == 0 and net.shape(1) == (1, 1, 12, 12) and net.shape(net.index("prob")) == (1, 5, 12, 12)
    _feed_classes(net, 6, 5, stripe=0)
    net.forward()
    net.sync()
    assert net.dice_loss_stats(1)["valid"] == 132 and net.dice_loss_stats(1)["ignored"] == 12
    assert net.resize(8, 8, 3, need_realloc=False) == 0 and net.shape(1) == (1, 1, 8, 8)
    _feed_classes(net, 7, 5)
    net.forward()
    net.sync()
    assert net.dice_loss_stats(1)["valid"] == 64 and np.array_equal(net.confusion_matrix(1).sum(1), net.dice_loss_sums(1)[0, :, 2])
    net.close()


@pytest.mark.parametrize("reduce,groups", [("batch", 1), ("image", 2)])
def test_sums_through_the_net_have_one_group_per_image_under_reduce_image(reduce, groups):
    """Net.dice_loss_sums sizes its buffer from the node: [G][C][3], equal to the float64 sums of the net's own logits
    within the operator test's bounds (one tile, L = 1)"""
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=8, h=8, c=3, n=2)
    net.conv(5, 1, 1, 0, src="input", dst="out")
    node = net.dice_loss("out", "prob", ignore_label=IGNORE, reduce=reduce)
    net.compile()
    lab = _feed_classes(net, 11, 5, stripe=2)
    net.forward()
    net.sync()
    sums, stats = net.dice_loss_sums(node), net.dice_loss_stats(node)
    ref = reference(_data(net, net.index("out")).reshape(2, 5, 64), lab.reshape(2, 64), IGNORE, 0.4, 0.6, 1e-5, True, reduce)
    assert sums.shape == (groups, 5, 3) == ref["izy"].shape and np.array_equal(sums[..., 2], ref["izy"][..., 2])
    assert np.abs(sums[..., :2] - ref["izy"][..., :2]).max() <= (2 * 8 + 12) * U * ref["izy"][..., :2].max()
    assert abs(stats["dice"] - ref["dice"]) <= (3 * 8 + 24) * U and stats["valid"] == 112
    net.close()


def test_predict_mode_writes_p_and_no_statistics(tmp_path):
    from bcnn_amd import capi, ops
    net = _load(tmp_path, TINY, capi.MODE_PREDICT)
    _feed(net, 8, label=False)
    net.forward()
    net.sync()
    with pytest.raises(ValueError):
        net.dice_loss_stats(1)
    with pytest.raises(ValueError):
        net.dice_loss_sums(1)
    p = torch.zeros(2, 5, 8, 8, device="cuda:0")
    ops.softmax_loss_forward(torch.tensor(_data(net, net.index("out")), device="cuda:0"), None, p, None)
    assert np.array_equal(BITS(_data(net, net.index("prob"))), BITS(p.cpu().numpy()))
    net.close()


@pytest.mark.parametrize("name,keys,want", [
    ("dice_loss", "", "ignore -1 ce 0.4 dice 0.6 smooth 1e-05 squared reduce batch"),
    ("softmax_dice_loss", "ignore_label=7\nce_weight=0.5\ndice_weight=0.5\nsmooth=1\nsquared=0\nreduce=image\n",
     "ignore 7 ce 0.5 dice 0.5 smooth 1 plain reduce image")])
def test_config_defaults_and_keys_reach_the_builder(tmp_path, capfd, name, keys, want):
    from bcnn_amd import capi
    L, net = capi.lib(), C.c_void_p()
    assert L.bcnn_init_net(C.byref(net), capi.MODE_TRAIN) == 0
    L.bcnn_set_log_context(net, None, 0)   # BCNN_LOG_INFO: the builder's line
    cfg = tmp_path / "loss.cfg"
    cfg.write_text(HEAD % (8, 6, 3) + _sections(("conv", CONV % (4, 1, 1), "input", "c1"), (name, keys, "c1", "loss")))
    capfd.readouterr()
    assert L.bcnn_load_net(net, str(cfg).encode(), None) == 0
    io = capfd.readouterr()
    assert want in io.err + io.out, io.err + io.out
    assert L.bcnn_get_num_nodes(net) == 2 and L.bcnn_get_node_type(net, 1) == capi.LAYER_DICE_LOSS
    for bad in ((1 << 24, 0.4, 0.6, 1e-5, 0), (255, 0.4, 0.6, -1e-9, 0), (255, 0.4, 0.6, float("inf"), 0), (255, 0.4, 0.6, 1e-5, 2),
                (255, float("nan"), 0.6, 1e-5, 0)):
        assert L.bcnn_add_dice_loss_layer(net, bad[0], bad[1], bad[2], bad[3], 1, bad[4], b"c1", b"label", b"x") == 1, bad
    assert L.bcnn_add_dice_loss_layer(net, (1 << 24) - 1, 0.4, 0.6, 0.0, 1, 1, b"c1", b"label", b"x") == 0 and L.bcnn_get_num_nodes(net) == 3
    L.bcnn_end_net(C.byref(net))


def test_swin_unet_objective_decreases_over_sgd_steps(tmp_path):
    from bcnn_amd import capi
    net = _load(tmp_path, UNET, capi.MODE_TRAIN)
    loss_node = net.num_nodes - 1
    assert net.node_type(loss_node) == capi.LAYER_DICE_LOSS and net.shape(net.index("prob")) == (2, 3, 16, 16)
    net.set_sgd(0.02, 0.9)
    _feed_classes(net, 9, 3)
    losses = []
    for _ in range(8):
        net.forward()
        net.backward()
        net.update()
        losses.append(net.dice_loss_stats(loss_node)["loss"])
    print("losses", losses)
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    net.close()
