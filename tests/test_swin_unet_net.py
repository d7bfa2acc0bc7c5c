"""The patch-expanding node inside nets (bcnn_amd.capi): a small Swin-UNet-shaped graph against torch float64 autograd, the
model file, the config sections, the builder refusals and bcnn_resize_net."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_group_norm_net import _bits, _data, _feed, _grad, _set_params, _state
from tests.test_patch_expand import expand

pytestmark = pytest.mark.gpu
SEED = 20261127
F32 = np.float32
HEAD = "[net]\ninput_width=%d\ninput_height=%d\ninput_channels=%d\nbatch_size=2\n\n"
CONV = "filters=%d\nsize=%d\nstride=%d\npad=0\nactivation=linear\n"


def _sections(*sections):
    return "".join("[%s]\n%ssrc=%s\ndst=%s\n\n" % s for s in sections)


# C = 4: 4x4/s4 embedding -> norm -> merge (4C = 16) -> 1x1 -> 1x1 to 2 x 8 -> expand -> cat with the skip -> 1x1 -> 1x1 to 16C ->
# expand x4 -> 1x1 to 3 classes -> loss
BODY = _sections(("conv", CONV % (4, 4, 4), "input", "emb"), ("channelnorm", "", "emb", "ln"), ("patch_merging", "", "ln", "pm"),
                 ("conv", CONV % (8, 1, 1), "pm", "d"), ("conv", CONV % (16, 1, 1), "d", "e"), ("patch_expanding", "", "e", "u"),
                 ("route", "", "u,ln", "cat"), ("conv", CONV % (4, 1, 1), "cat", "f"), ("conv", CONV % (64, 1, 1), "f", "g"),
                 ("patch_expanding", "block=4\n", "g", "v"), ("conv", CONV % (3, 1, 1), "v", "out"))
UNET = HEAD % (16, 16, 3) + BODY + _sections(("softmax_loss", "", "out", "prob"))
EMB, LN, PM, CONV1, CONV2, PE2, CAT, CONV3, CONV4, PE4, CONV5, LOSS = range(12)
NORMS, CONVS = (LN, PM, PE2, PE4), (EMB, CONV1, CONV2, CONV3, CONV4, CONV5)


def _load(tmp_path, text, mode, name="net.cfg"):
    from bcnn_amd import capi
    cfg = tmp_path / name
    cfg.write_text(text)
    C.CDLL(None).srand(SEED)
    net = capi.Net.load_net(str(cfg), None, mode=mode)
    net.compile()
    return net


def _params(net, node):
    return [_data(net, net.node_src(node, slot)) for slot in (1, 2)]


def _feed_classes(net, seed):
    _feed(net, seed, label=False)
    net.data(1)[...] = np.random.RandomState(seed).randint(0, 3, net.shape(1))
    net.upload(1)


def test_unet_against_torch_float64_autograd(tmp_path):
    """the logits and every parameter gradient within 1e-5 of the tensor's largest value (the bar of tests/test_swin_stage_net.py)"""
    from bcnn_amd import capi
    net = _load(tmp_path, UNET, capi.MODE_TRAIN)
    assert [net.node_type(k) for k in (PE2, PE4, LOSS)] == [capi.LAYER_PATCH_EXPANDING] * 2 + [capi.LAYER_SOFTMAX_LOSS]
    assert net.shape(net.index("u")) == (2, 4, 4, 4) and net.shape(net.index("v")) == (2, 4, 16, 16)
    assert net.shape(net.node_src(PE2, 1)) == net.shape(net.node_src(PE4, 2)) == (1, 1, 1, 4) and net.shape(1) == (2, 1, 16, 16)
    for node in NORMS:
        _set_params(net, node, 3 + node)
    _feed_classes(net, 8)
    net.forward()
    net.backward()
    net.sync()
    p = {k: [torch.tensor(v.astype(np.float64), requires_grad=True) for v in _params(net, k)] for k in NORMS + CONVS}

    def norm(t, k):
        return F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), p[k][0].ravel(), p[k][1].ravel(), 1e-5).permute(0, 3, 1, 2)

    def conv(t, k, size=1):
        return F.conv2d(t, p[k][0].reshape(-1, t.shape[1], size, size), p[k][1].ravel(), stride=size)

    def expand_t(t, b):   # einops 'b h w (p1 p2 c) -> b (h p1) (w p2) c' on NCHW
        n, c_in, h, w = t.shape
        return t.reshape(n, b, b, c_in // (b * b), h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c_in // (b * b), b * h, b * w)

    ln = norm(conv(torch.tensor(net.data(0).astype(np.float64)), EMB, 4), LN)
    pm = norm(torch.cat([ln[:, :, 0::2, 0::2], ln[:, :, 1::2, 0::2], ln[:, :, 0::2, 1::2], ln[:, :, 1::2, 1::2]], 1), PM)
    u = norm(expand_t(conv(conv(pm, CONV1), CONV2), 2), PE2)
    v = norm(expand_t(conv(conv(torch.cat([u, ln], 1), CONV3), CONV4), 4), PE4)
    out = conv(v, CONV5)
    out.backward(torch.tensor(_grad(net, net.index("out")).astype(np.float64)))
    assert np.abs(_grad(net, net.index("out"))).max() > 0
    checks = [("out", _data(net, net.index("out")), out.detach())]
    checks += [("node %d slot %d" % (k, s + 1), _grad(net, net.node_src(k, s + 1)), p[k][s].grad) for k in NORMS + CONVS for s in (0, 1)]
    for what, got, want in checks:
        want = want.numpy().reshape(got.shape)
        assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), what
    net.close()


def test_model_file_round_trip_and_predict_equals_train(tmp_path):
    from bcnn_amd import capi
    a = _load(tmp_path, UNET, capi.MODE_TRAIN)
    for node in (PE2, PE4):
        _set_params(a, node, 20 + node)
    path, again = str(tmp_path / "unet.bcnnmodel"), str(tmp_path / "again.bcnnmodel")
    assert a.save_weights(path) == 0
    blob = open(path, "rb").read()
    before_pe2 = (4 * 48 + 4) + 8 + 32 + (8 * 16 + 8) + (16 * 8 + 16)
    after_pe2 = (4 * 8 + 4) + (64 * 4 + 64) + 8 + (3 * 4 + 3)
    assert len(blob) == 16 + 4 * (before_pe2 + 8 + after_pe2)
    in_file = np.frombuffer(blob[16 + 4 * before_pe2:16 + 4 * (before_pe2 + 8)], F32)   # b, then scales
    scales, b = (v.ravel() for v in _params(a, PE2))
    assert np.array_equal(_bits(in_file[:4]), _bits(b)) and np.array_equal(_bits(in_file[4:]), _bits(scales))
    p = _load(tmp_path, HEAD % (16, 16, 3) + BODY, capi.MODE_PREDICT, "predict.cfg")
    assert p.load_weights(path) == 0 and not p.node_state(PE2, 0) and a.node_state(PE2, 0) and a.node_state(PE4, 0)
    assert p.save_weights(again) == 0 and open(again, "rb").read() == blob
    outs = []
    for net in (a, p):
        _feed(net, 31, label=False)
        net.forward()
        net.sync()
        outs.append(_data(net, net.index("out")))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "PREDICT computes what TRAIN computes"
    a.close()
    p.close()


@pytest.mark.parametrize("section,block,order,norm", [
    ("[patch_expanding]\n", 2, "blocks", 1), ("[patchexpand]\nblock=4\neps=0.001\n", 4, "blocks", 1),
    ("[patch_expanding]\nnorm=0\norder=channels\n", 2, "channels", 0), ("[depth_to_space]\n", 2, "blocks", 0),
    ("[pixel_shuffle]\nblock=4\n", 4, "channels", 0), ("[pixel_shuffle]\norder=blocks\nnorm=1\n", 2, "blocks", 0)])
def test_patch_expanding_sections(tmp_path, section, block, order, norm):
    from bcnn_amd import capi, ops
    net = _load(tmp_path, HEAD % (3, 2, 32) + section + "src=input\ndst=y\n", capi.MODE_PREDICT)
    c = 32 // (block * block)
    assert net.num_nodes == 1 and net.node_type(0) == capi.LAYER_PATCH_EXPANDING and net.shape(net.index("y")) == (2, c, 2 * block, 3 * block)
    _feed(net, 9, label=False)
    if norm:
        _set_params(net, 0, 5)
    net.forward()
    net.sync()
    x = net.data(0).copy()
    if not norm:
        assert np.array_equal(_bits(_data(net, net.index("y"))), _bits(expand(x, block, order)))
    else:
        ty = torch.zeros(2, c, 2 * block, 3 * block, device="cuda:0")
        scales, b = (torch.tensor(v.ravel(), device="cuda:0") for v in _params(net, 0))
        ops.patch_expand_forward(torch.tensor(x, device="cuda:0"), scales, b, ty, None, None, block, order, 1e-3 if "eps" in section else 1e-5)
        assert np.array_equal(_bits(_data(net, net.index("y"))), _bits(ty.cpu().numpy()))
    net.close()


def test_builder_refusals_leave_the_node_count():
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=6, h=4, c=2, n=2)
    net.conv(16, 1, 1, 0, src="input", dst="a")
    net.conv(6, 1, 1, 0, src="input", dst="six")
    L, h = net.L, net.net
    nodes = L.bcnn_get_num_nodes(h)
    for block, order, src in ((2, 0, b"nowhere"), (3, 0, b"a"), (8, 0, b"a"), (2, 2, b"a"), (2, -1, b"a"), (2, 0, b"six"), (4, 1, b"six")):
        for norm in (0, 1):
            assert L.bcnn_add_patch_expanding_layer(h, block, order, norm, 0.0, src, b"x") == 1 and L.bcnn_get_num_nodes(h) == nodes
    assert L.bcnn_add_patch_expanding_layer(h, 4, 1, 1, 0.0, b"a", b"x") == 0 and L.bcnn_get_num_nodes(h) == nodes + 1
    net.close()


def test_resize_to_a_new_extent(tmp_path):
    from bcnn_amd import capi, ops
    text = HEAD % (4, 4, 3) + _sections(("conv", CONV % (8, 1, 1), "input", "a"), ("patch_expanding", "", "a", "u"),
                                        ("conv", CONV % (2, 1, 1), "u", "out"), ("cost", "", "out", "cost"))
    net = _load(tmp_path, text, capi.MODE_TRAIN)
    assert net.resize(3, 5, 3, need_realloc=False) == 0 and net.shape(net.index("u")) == (1, 2, 10, 6), "within the capacity"
    assert net.resize(10, 6, 3, need_realloc=False) == 1, "the statistics would outgrow their buffer"
    assert net.shape(net.index("u")) == (1, 2, 10, 6), "a refused resize changes nothing"
    assert net.resize(10, 6, 3, need_realloc=True) == 0
    assert net.shape(net.index("u")) == (1, 2, 12, 20) and net.shape(net.index("out")) == (1, 2, 12, 20)
    _feed(net, 12, label=False)
    net.forward()
    net.sync()
    ty, tm, tr = torch.zeros(1, 2, 12, 20, device="cuda:0"), torch.zeros(240, device="cuda:0"), torch.zeros(240, device="cuda:0")
    scales, b = (torch.tensor(v.ravel(), device="cuda:0") for v in _params(net, 1))
    ops.patch_expand_forward(torch.tensor(_data(net, net.index("a")), device="cuda:0"), scales, b, ty, tm, tr)
    assert np.array_equal(_bits(_data(net, net.index("u"))), _bits(ty.cpu().numpy()))
    assert np.array_equal(_bits(_state(net, 1, 480)), _bits(torch.cat([tm, tr]).cpu().numpy())), "the statistics followed"
    net.close()
