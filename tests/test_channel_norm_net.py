"""The channel-norm node inside nets (bcnn_amd.capi): forward = the ops call, bit for bit; a TRAIN step against float64."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_channel_norm import reference
from tests.test_group_norm_net import _bits, _data, _feed, _grad, _set_params, _state, _t

pytestmark = pytest.mark.gpu
SEED = 20261126
INVALID_PARAMETER = 1
HEAD = "[net]\ninput_width=4\ninput_height=4\ninput_channels=8\nbatch_size=2\n\n"
CONV = "filters=8\nsize=1\nstride=1\npad=0\nactivation=linear\n"


def _params(net, node):
    return [_data(net, net.node_src(node, slot)).ravel() for slot in (1, 2)]


def _forward_is_the_ops_call(net, node, eps=1e-5):
    """runs the net's forward: the node's output carries the bits of the ops call on its source; x, scales, mean, rstd"""
    from bcnn_amd import ops
    net.forward()
    net.sync()
    x, (scales, b) = _data(net, net.node_src(node, 0)), _params(net, node)
    positions = x.size // x.shape[1]
    ty, tm, tr = _t(np.zeros_like(x)), _t(np.zeros(positions)), _t(np.zeros(positions))
    ops.channel_norm_forward(_t(x), _t(scales), _t(b), ty, tm, tr, eps)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_data(net, net.node_dst(node))), _bits(ty.cpu().numpy())), "node output"
    return x, scales, tm.cpu().numpy(), tr.cpu().numpy()


def _net(mode, second_consumer=False, head=True, shape=(2, 3, 5, 5), norm=True):
    """input -> conv 1x1 -> 6 [-> channelnorm [-> eltwise with the conv output]] -> conv 1x1 -> 4 -> cost"""
    from bcnn_amd import capi
    n, c, h, w = shape
    C.CDLL(None).srand(SEED)
    net = capi.Net(mode=mode, w=w, h=h, c=c, n=n)
    net.conv(6, 1, 1, 0, act=capi.ACT_NONE, src="input", dst="c1")
    node = net.channelnorm("c1", "cn") if norm else None
    if second_consumer:
        net.eltwise(capi.ACT_NONE, "c1", "cn", "sum")
    if head:
        net.conv(4, 1, 1, 0, act=capi.ACT_NONE, src="sum" if second_consumer else "cn" if norm else "c1", dst="c2")
        net.cost("c2", "label", "cost")
    net.compile()
    if norm:
        _set_params(net, node, 11)
    return net, node


def test_builder_and_refusals():
    from bcnn_amd import capi
    net, node = _net(capi.MODE_TRAIN)
    assert net.node_type(node) == capi.LAYER_CHANNEL_NORM
    assert net.shape(net.node_src(node, 1)) == (1, 1, 1, 6) and net.shape(net.node_src(node, 2)) == (1, 1, 1, 6)
    nodes = net.L.bcnn_get_num_nodes(net.net)
    assert net.L.bcnn_add_channel_norm_layer(net.net, 0.0, b"no_such_tensor", b"z") == INVALID_PARAMETER
    assert net.L.bcnn_get_num_nodes(net.net) == nodes
    net.close()
    big, L = C.c_void_p(), capi.lib()   # 2^31 elements: refused before anything is allocated (the shape alone is set)
    assert L.bcnn_init_net(C.byref(big), capi.MODE_PREDICT) == 0
    L.bcnn_set_log_context(big, None, capi.LOG_SILENT)
    L.bcnn_set_input_shape(big, 65536, 32768, 1, 1)
    assert L.bcnn_add_channel_norm_layer(big, 0.0, b"input", b"z") == INVALID_PARAMETER and L.bcnn_get_num_nodes(big) == 0
    L.bcnn_set_input_shape(big, 4, 4, 1, 1)
    L.bcnn_end_net(C.byref(big))


@pytest.mark.parametrize("second_consumer", [False, True])
def test_train_step_against_float64(second_consumer):
    """dx, dscales, db within the float64 bounds of tests/test_channel_norm.py on the node's own statistics; dx is assigned by a
    sole writer, else added to the eltwise node's share (one more rounding, 2^-24 of the sum); the update is ops.sgd_update"""
    from bcnn_amd import capi, ops
    net, node = _net(capi.MODE_TRAIN, second_consumer)
    lr, momentum, decay = 0.05, 0.9, 5e-4
    net.set_sgd(lr, momentum, decay)
    assert net.L.bcnn_grad_sole_writer(net.net, net.index("c1")) == (0 if second_consumer else 1)
    _feed(net, 3)
    x, scales, mean, rstd = _forward_is_the_ops_call(net, node)
    net.backward()
    net.sync()
    r = reference(x.reshape(2, 6, 25).astype(np.float64), scales.astype(np.float64),
                  _grad(net, net.index("cn")).reshape(2, 6, 25).astype(np.float64), stats=(mean.reshape(2, 25), rstd.reshape(2, 25)))
    want = r["dx64"].reshape(x.shape).copy()
    if second_consumer:   # the eltwise node hands its gradient to image 0 of its second operand (bcnn_layers_next.c)
        want[0] += _grad(net, net.index("sum"))[0]
    g_x, g_s, g_b = (_grad(net, i) for i in (net.index("c1"), net.node_src(node, 1), net.node_src(node, 2)))
    assert (np.abs(g_x - want) <= r["dx_bound"].reshape(x.shape) + 2.0 ** -24 * np.abs(want) * second_consumer).all()
    assert (np.abs(g_s.ravel() - r["dscales64"]) <= r["dscales_bound"]).all() and (np.abs(g_b.ravel() - r["db64"]) <= r["db_bound"]).all()
    tw, tb = _t(scales), _t(_params(net, node)[1])
    ops.sgd_update(tw, tb, _t(g_s.ravel()), _t(g_b.ravel()), 2, lr, momentum, decay)
    net.update()
    net.sync()
    after = _params(net, node)
    assert np.array_equal(_bits(after[0]), _bits(tw.cpu().numpy())) and np.array_equal(_bits(after[1]), _bits(tb.cpu().numpy()))
    assert not np.array_equal(_bits(after[0]), _bits(scales))
    net.close()


def test_model_file_round_trip_and_a_net_without_the_node(tmp_path):
    from bcnn_amd import capi
    a, node = _net(capi.MODE_TRAIN)
    _set_params(a, node, 23)
    path, other = str(tmp_path / "cn.bcnnmodel"), str(tmp_path / "plain.bcnnmodel")
    assert a.save_weights(path) == 0
    blob = open(path, "rb").read()
    conv1, conv2 = 6 * 3 + 6, 4 * 6 + 4
    assert len(blob) == 16 + 4 * (conv1 + 12 + conv2)
    in_file = np.frombuffer(blob[16 + 4 * conv1:16 + 4 * conv1 + 48], np.float32)   # b, then scales
    scales, b = _params(a, node)
    assert np.array_equal(_bits(in_file[:6]), _bits(b)) and np.array_equal(_bits(in_file[6:]), _bits(scales))
    p, node_p = _net(capi.MODE_PREDICT)
    assert p.load_weights(path) == 0 and not p.node_state(node_p, 0)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(_params(p, node_p), (scales, b)))
    plain, _ = _net(capi.MODE_PREDICT, norm=False)   # without the node: the two convolutions and nothing else
    assert plain.save_weights(other) == 0
    assert open(other, "rb").read() == blob[:16 + 4 * conv1] + blob[16 + 4 * (conv1 + 12):]
    for net in (a, p, plain):
        net.close()


@pytest.mark.parametrize("section,eps", [("[channelnorm]\n", 1e-5), ("[layernorm2d]\neps=0.001\n", 1e-3), ("[tokennorm]\n", 1e-5)])
def test_config_sections(tmp_path, section, eps):
    from bcnn_amd import capi
    cfg = tmp_path / "cn.cfg"
    cfg.write_text(HEAD + section + "src=input\ndst=a\n")
    net = capi.Net.load_net(str(cfg), None, mode=capi.MODE_PREDICT)
    net.compile()
    assert net.num_nodes == 1 and net.node_type(0) == capi.LAYER_CHANNEL_NORM
    _set_params(net, 0, 5)
    _feed(net, 9, label=False)
    _forward_is_the_ops_call(net, 0, eps)
    net.close()


def test_resize_grows_the_statistics():
    from bcnn_amd import capi
    net, node = _net(capi.MODE_TRAIN, head=False, shape=(1, 3, 4, 4))
    assert net.resize(12, 12, 3, need_realloc=True) == 0 and net.shape(net.index("cn")) == (1, 6, 12, 12)
    _feed(net, 12, label=False)
    _, _, mean, rstd = _forward_is_the_ops_call(net, node)
    stats = _state(net, node, 288)
    assert np.array_equal(_bits(stats[:144]), _bits(mean)) and np.array_equal(_bits(stats[144:]), _bits(rstd))
    net.close()


BLOCK = HEAD + "".join("[%s]\n%ssrc=%s\ndst=%s\n\n" % s for s in (
    ("tokennorm", "", "input", "ln"), ("conv", CONV, "ln", "q"), ("conv", CONV, "ln", "k"), ("conv", CONV, "ln", "v"),
    ("attention", "heads=2\n", "q,k,v", "att"), ("conv", CONV, "att", "proj"),
    ("eltwise", "activation=linear\n", "proj,input", "out")))


def test_encoder_block_against_float64(tmp_path):
    """channelnorm -> 1x1 conv (q, k, v) -> attention -> 1x1 conv -> add, from a config string, against a float64 numpy
    composition within the convolution's 1e-4 parity bar plus the attention's 1e-5 bar (relative to the largest output)"""
    from bcnn_amd import capi
    cfg = tmp_path / "block.cfg"
    cfg.write_text(BLOCK)
    C.CDLL(None).srand(SEED)
    net = capi.Net.load_net(str(cfg), None, mode=capi.MODE_PREDICT)
    net.compile()
    _set_params(net, 0, 7)
    _feed(net, 21, label=False)
    net.forward()
    net.sync()
    x = net.data(0).astype(np.float64).reshape(2, 8, 16)
    scales, b = (p.astype(np.float64) for p in _params(net, 0))
    ln = (x - x.mean(axis=1, keepdims=True)) / np.sqrt(x.var(axis=1, keepdims=True) + 1e-5) * scales[:, None] + b[:, None]

    def conv(node, t):
        w, bias = (p.astype(np.float64) for p in _params(net, node))
        return np.einsum("fc,ncp->nfp", w.reshape(8, 8), t) + bias[:, None]

    q, k, v = (conv(node, ln).reshape(2, 2, 4, 16) for node in (1, 2, 3))
    s = np.einsum("nhti,nhtj->nhij", q, k) / 2.0   # 1 / sqrt(d), d = 4
    p = np.exp(s - s.max(axis=3, keepdims=True))
    p /= p.sum(axis=3, keepdims=True)
    want = conv(5, np.einsum("nhrj,nhij->nhri", v, p).reshape(2, 8, 16))
    want[0] += x[0]   # the eltwise node's same-shape path adds its second operand to image 0 (the reference's quirk 5)
    got = _data(net, net.index("out")).reshape(2, 8, 16)
    assert np.abs(got - want).max() / np.abs(want).max() <= 1e-4 + 1e-5
    net.close()
