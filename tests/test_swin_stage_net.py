"""The residual, patch-merging and GELU nodes inside nets (bcnn_amd.capi): the residual add over the whole batch in bits, a
Swin stage transition against torch float64 autograd, the model file, the config sections and bcnn_resize_net."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_group_norm_net import _bits, _data, _feed, _grad, _set_params, _state
from tests.test_patch_merge import merge

pytestmark = pytest.mark.gpu
SEED = 20261126
F32 = np.float32
HEAD = "[net]\ninput_width=4\ninput_height=4\ninput_channels=6\nbatch_size=%d\n\n"
CONV = "filters=%d\nsize=1\nstride=1\npad=0\nactivation=%s\n"


def _sections(*sections):
    return "".join("[%s]\n%ssrc=%s\ndst=%s\n\n" % s for s in sections)


# tokennorm -> conv 1x1 (gelu: split into the node and the in-place activation) -> conv 1x1 -> + input -> merge -> conv 1x1
STAGE = HEAD % 2 + _sections(("tokennorm", "", "input", "ln"), ("conv", CONV % (12, "gelu"), "ln", "h"),
                             ("conv", CONV % (6, "linear"), "h", "m"), ("residual", "", "input,m", "r"),
                             ("patch_merging", "", "r", "pm"), ("conv", CONV % (12, "linear"), "pm", "out"),
                             ("cost", "", "out", "cost"))
NORM0, CONV1, ACT, CONV2, RES, PM, CONV3 = range(7)


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


@pytest.mark.parametrize("with_eltwise", [False, True])
def test_residual_adds_every_image_and_eltwise_keeps_its_quirk(tmp_path, with_eltwise):
    """batch 3: forward and both gradients in bits; with a second reader of `a` the node adds to its gradient, else assigns"""
    from bcnn_amd import capi
    quirk = [("eltwise", "activation=linear\n", "a,b", "quirk")] if with_eltwise else []
    text = HEAD % 3 + _sections(("conv", CONV % (6, "linear"), "input", "a"), ("conv", CONV % (6, "linear"), "input", "b"),
                                ("residual", "", "a,b", "sum"), *quirk, ("cost", "", "sum", "cost"))
    net = _load(tmp_path, text, capi.MODE_TRAIN)
    assert net.node_type(2) == capi.LAYER_RESIDUAL and [net.node_src(2, k) for k in (0, 1)] == [net.index("a"), net.index("b")]
    assert net.L.bcnn_grad_sole_writer(net.net, net.index("a")) == (0 if with_eltwise else 1)
    _feed(net, 5)
    net.forward()
    net.backward()
    net.sync()
    a, b = _data(net, net.index("a")), _data(net, net.index("b"))
    assert np.array_equal(_bits(_data(net, net.index("sum"))), _bits(a + b)), "every image"
    if with_eltwise:   # [eltwise] on the same inputs: its second operand reaches image 0 only
        first, second = (_data(net, net.node_src(3, k)) for k in (0, 1))
        first[0] += second[0]
        assert np.array_equal(_bits(_data(net, net.index("quirk"))), _bits(first))
    g = _grad(net, net.index("sum"))   # (the eltwise node's output has no reader: it hands on zeros)
    assert np.abs(g[1:]).max() > 0
    assert np.array_equal(_bits(_grad(net, net.index("a"))), _bits(g)) and np.array_equal(_bits(_grad(net, net.index("b"))), _bits(g))
    net.close()


def test_stage_against_torch_float64_autograd(tmp_path):
    """the output and every parameter gradient within 1e-5 of the tensor's largest value (the attention net tests' bar)"""
    from bcnn_amd import capi
    net = _load(tmp_path, STAGE, capi.MODE_TRAIN)
    assert [net.node_type(k) for k in (ACT, RES, PM)] == [capi.LAYER_ACTIVATION, capi.LAYER_RESIDUAL, capi.LAYER_PATCH_MERGING]
    assert net.node_activation(ACT) == capi.ACT_GELU and net.node_activation(CONV1) == capi.ACT_NONE
    assert net.shape(net.index("pm")) == (2, 24, 2, 2) and net.shape(net.node_src(PM, 1)) == (1, 1, 1, 24)
    for node, seed in ((NORM0, 3), (PM, 4)):
        _set_params(net, node, seed)
    _feed(net, 8)
    net.forward()
    net.backward()
    net.sync()
    nodes = (NORM0, CONV1, CONV2, PM, CONV3)
    p = {k: [torch.tensor(v.astype(np.float64), requires_grad=True) for v in _params(net, k)] for k in nodes}
    x = torch.tensor(net.data(0).astype(np.float64))

    def norm(t, k):
        return F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), p[k][0].ravel(), p[k][1].ravel(), 1e-5).permute(0, 3, 1, 2)

    def conv(t, k):
        return F.conv2d(t, p[k][0].reshape(-1, t.shape[1], 1, 1), p[k][1].ravel())

    r = x + conv(F.gelu(conv(norm(x, NORM0), CONV1)), CONV2)
    merged = torch.cat([r[:, :, 0::2, 0::2], r[:, :, 1::2, 0::2], r[:, :, 0::2, 1::2], r[:, :, 1::2, 1::2]], 1)
    out = conv(norm(merged, PM), CONV3)
    out.backward(torch.tensor(_grad(net, net.index("out")).astype(np.float64)))
    checks = [("out", _data(net, net.index("out")), out.detach())]
    checks += [("node %d slot %d" % (k, s + 1), _grad(net, net.node_src(k, s + 1)), p[k][s].grad) for k in nodes for s in (0, 1)]
    for what, got, want in checks:
        want = want.numpy().reshape(got.shape)
        assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), what
    net.close()


def test_model_file_round_trip_and_predict_equals_train(tmp_path):
    from bcnn_amd import capi
    a = _load(tmp_path, STAGE, capi.MODE_TRAIN)
    _set_params(a, PM, 23)
    path, again = str(tmp_path / "stage.bcnnmodel"), str(tmp_path / "again.bcnnmodel")
    assert a.save_weights(path) == 0
    blob = open(path, "rb").read()
    before_pm = 12 + (12 * 6 + 12) + (6 * 12 + 6)
    assert len(blob) == 16 + 4 * (before_pm + 48 + 12 * 24 + 12)
    in_file = np.frombuffer(blob[16 + 4 * before_pm:16 + 4 * (before_pm + 48)], F32)   # b, then scales
    scales, b = (v.ravel() for v in _params(a, PM))
    assert np.array_equal(_bits(in_file[:24]), _bits(b)) and np.array_equal(_bits(in_file[24:]), _bits(scales))
    p = _load(tmp_path, STAGE.replace("[cost]\nsrc=out\ndst=cost\n\n", ""), capi.MODE_PREDICT, "predict.cfg")
    assert p.load_weights(path) == 0 and not p.node_state(PM, 0) and a.node_state(PM, 0)
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


@pytest.mark.parametrize("section,norm", [("[patch_merging]\n", 1), ("[patchmerge]\neps=0.001\n", 1), ("[patch_merging]\nnorm=0\n", 0),
                                          ("[space_to_depth]\n", 0), ("[focus]\n", 0)])
def test_patch_merging_sections(tmp_path, section, norm):
    from bcnn_amd import capi, ops
    net = _load(tmp_path, HEAD % 2 + section + "src=input\ndst=y\n", capi.MODE_PREDICT)
    assert net.num_nodes == 1 and net.node_type(0) == capi.LAYER_PATCH_MERGING and net.shape(net.index("y")) == (2, 24, 2, 2)
    _feed(net, 9, label=False)
    if norm:
        _set_params(net, 0, 5)
    net.forward()
    net.sync()
    x = net.data(0).copy()
    if not norm:
        assert np.array_equal(_bits(_data(net, net.index("y"))), _bits(merge(x)))
    else:
        ty = torch.zeros(2, 24, 2, 2, device="cuda:0")
        scales, b = (torch.tensor(v.ravel(), device="cuda:0") for v in _params(net, 0))
        ops.patch_merge_forward(torch.tensor(x, device="cuda:0"), scales, b, ty, None, None, 1e-3 if "eps" in section else 1e-5)
        assert np.array_equal(_bits(_data(net, net.index("y"))), _bits(ty.cpu().numpy()))
    net.close()


PRE = HEAD % 2 + _sections(("conv", CONV % (6, "linear"), "input", "c"))


@pytest.mark.parametrize("text", [
    PRE + "[patch_merging]\nactivation=relu\nsrc=c\ndst=y\n", PRE + "[residual]\nactivation=relu\nsrc=input,c\ndst=y\n",
    PRE.replace("input_width=4", "input_width=5") + "[patch_merging]\nsrc=c\ndst=y\n", PRE + "[focus]\nsrc=nowhere\ndst=f\n"])
def test_refused_sections(tmp_path, text):
    from bcnn_amd import capi
    with pytest.raises(RuntimeError):
        _load(tmp_path, text, capi.MODE_PREDICT)
    _load(tmp_path, PRE + "[add]\nsrc=input,c\ndst=y\n", capi.MODE_PREDICT).close()   # (the section before the bad one is fine)


def test_builder_refusals_leave_the_node_count():
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=6, h=4, c=2, n=2)
    net.conv(2, 1, 1, 0, src="input", dst="a")
    net.conv(2, 3, 1, 0, src="input", dst="odd")   # 4 x 2 -> [2,2,2,4]; then one more: 3 wide
    net.conv(2, 2, 1, 0, src="odd", dst="odd3")    # [2,2,1,3]
    L, h = net.L, net.net
    nodes = L.bcnn_get_num_nodes(h)
    for refused in (lambda: L.bcnn_add_patch_merging_layer(h, 1, 0.0, b"nowhere", b"x"),
                    lambda: L.bcnn_add_patch_merging_layer(h, 1, 0.0, b"odd3", b"x"),
                    lambda: L.bcnn_add_patch_merging_layer(h, 0, 0.0, b"odd3", b"x"),
                    lambda: L.bcnn_add_residual_layer(h, b"a", b"nowhere", b"x"), lambda: L.bcnn_add_residual_layer(h, b"a", b"a", b"x"),
                    lambda: L.bcnn_add_residual_layer(h, b"a", b"odd", b"x")):
        assert refused() == 1 and L.bcnn_get_num_nodes(h) == nodes
    net.close()


def test_resize_to_an_even_extent_and_refusal_of_an_odd_one(tmp_path):
    from bcnn_amd import capi, ops
    net = _load(tmp_path, STAGE, capi.MODE_TRAIN)
    assert net.resize(12, 8, 6, need_realloc=True) == 0
    assert net.shape(net.index("r")) == (1, 6, 8, 12) and net.shape(net.index("pm")) == (1, 24, 4, 6)
    shapes = [net.shape(k) for k in (net.index("r"), net.index("pm"), net.index("out"))]
    assert net.resize(11, 8, 6, need_realloc=True) == 1 and net.resize(12, 7, 6, need_realloc=True) == 1
    assert [net.shape(k) for k in (net.index("r"), net.index("pm"), net.index("out"))] == shapes, "a refused resize changes nothing"
    _feed(net, 12, label=False)
    net.forward()
    net.sync()
    r = _data(net, net.index("r"))
    assert np.array_equal(_bits(r), _bits(net.data(0) + _data(net, net.index("m")))), "the residual node followed"
    ty, tm, tr = torch.zeros(1, 24, 4, 6, device="cuda:0"), torch.zeros(24, device="cuda:0"), torch.zeros(24, device="cuda:0")
    scales, b = (torch.tensor(v.ravel(), device="cuda:0") for v in _params(net, PM))
    ops.patch_merge_forward(torch.tensor(r, device="cuda:0"), scales, b, ty, tm, tr)
    assert np.array_equal(_bits(_data(net, net.index("pm"))), _bits(ty.cpu().numpy()))
    assert np.array_equal(_bits(_state(net, PM, 48)), _bits(torch.cat([tm, tr]).cpu().numpy())), "the statistics followed"
    net.close()
