"""The attention node inside nets (bcnn_amd.capi): bcnn_add_attention_layer, its workers, the [attention] config section and
bcnn_resize_net. The node's output and its three source gradients carry the bits of the bcnn_amd.ops calls on the same values
(tests/test_attention.py holds those to float64). Without a GPU: every refusal leaves the node count, both libraries export the
new symbols."""
import ctypes as C

import numpy as np
import pytest
import torch

DEV = "cuda:0"
F32 = np.float32
SEED = 20261126
INVALID_PARAMETER = 1
HEADS = 2


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


def _t(a):
    return torch.tensor(np.array(a, F32), device=DEV)


def _data(net, idx):
    net.download(idx, False)
    return net.data(idx).copy()


def _grad(net, idx):
    net.download(idx, True)
    return net.grad(idx).copy()


def _feed(net, seed, idx=0):
    net.data(idx)[...] = np.random.RandomState(seed).uniform(-1, 1, net.shape(idx))
    net.upload(idx)


def _net(mode, relu=False):
    """input [2][4][8][9] -> three 1x1 convolutions a (8), b (8), c (12) -> attention, 2 heads [-> relu in place] -> Euclidean
    cost"""
    from bcnn_amd import capi
    C.CDLL(None).srand(SEED)   # the fillers draw from rand(): the same weights for every net built after the same seed
    net = capi.Net(mode=mode, w=9, h=8, c=4, n=2)
    for name, f in (("a", 8), ("b", 8), ("c", 12)):
        net.conv(f, 1, 1, 0, src="input", dst=name)
    node = net.add_attention(HEADS, "a", "b", "c", "att")
    if relu:
        net.activation(capi.ACT_RELU, "att")
    net.cost("att", "label", "cost")
    net.compile()
    return net, node


def _check_against_the_ops(net, node, dy):
    """the node's output and source gradients (already computed from dy) are the bits of the op on the same values"""
    from bcnn_amd import ops
    ids = [net.node_src(node, i) for i in range(3)]
    q, k, v = [_t(_data(net, i)) for i in ids]
    o = torch.zeros(net.shape(net.node_dst(node)), dtype=torch.float32, device=DEV)
    lse = torch.zeros(q.shape[0] * HEADS * q.shape[2] * q.shape[3], dtype=torch.float32, device=DEV)
    ops.attention_forward(q, k, v, o, lse, HEADS)
    dq, dk, dv = [torch.full_like(x, 3.0) for x in (q, k, v)]
    ops.attention_backward(q, k, v, o, lse, _t(dy), dq, dk, dv, HEADS, overwrite=(True, True, True))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_data(net, net.node_dst(node))), _bits(o.cpu().numpy())), "node output"
    assert np.abs(o.cpu().numpy()).max() > 0
    for i, g in zip(ids, (dq, dk, dv)):
        assert net.L.bcnn_grad_sole_writer(net.net, i) == 1
        got = _grad(net, i)
        assert np.array_equal(_bits(got), _bits(g.cpu().numpy())) and np.abs(got).max() > 0, "gradient of tensor %d" % i


CFG = """
[net]
input_width=9
input_height=8
input_channels=4
batch_size=2
""" + "".join("\n[conv]\nfilters=%d\nsize=1\nstride=1\npad=0\nsrc=input\ndst=%s\n" % (f, n) for n, f in (("a", 8), ("b", 8), ("c", 12))) + """
[attention]
heads=2
src=a,b,c
dst=att
"""


@pytest.mark.gpu
def test_train_net_resize_and_config_section(tmp_path):
    from bcnn_amd import capi
    net, node = _net(capi.MODE_TRAIN)
    att = net.index("att")
    assert net.node_type(node) == capi.LAYER_ATTENTION == capi.LAYER_POOL2D + 7 == 24 and net.shape(att) == (2, 12, 8, 9)
    _feed(net, 3)
    _feed(net, 4, 1)
    net.forward()
    net.backward()
    net.sync()
    _check_against_the_ops(net, node, _grad(net, att))
    out = _data(net, att)
    # the INI form builds the same node: same weights, same input, same output bits
    cfg = tmp_path / "attention.cfg"
    cfg.write_text(CFG)
    C.CDLL(None).srand(SEED)
    ini = capi.Net.load_net(str(cfg), None, mode=capi.MODE_PREDICT)
    ini.compile()
    assert ini.num_nodes == 4 and ini.node_type(3) == capi.LAYER_ATTENTION and not ini.node_state(3, 0)
    _feed(ini, 3)
    ini.forward()
    ini.sync()
    assert np.array_equal(_bits(_data(ini, ini.index("att"))), _bits(out))
    ini.close()
    # bcnn_resize_net to 5 x 13 (batch 1): the node runs at the new shape, forward and backward
    assert net.resize(13, 5, 4, need_realloc=True) == 0 and net.shape(att) == (1, 12, 5, 13)
    _feed(net, 5)
    for i in range(node + 1):
        net.forward_node(i)
    dy = np.random.RandomState(6).uniform(-1, 1, net.shape(att)).astype(F32)
    net.download(att, False)   # (the upload below sends the host's data along with the gradient)
    net.grad(att)[...] = dy
    net.upload(att, with_grad=True)
    net.backward_node(node)
    net.sync()
    _check_against_the_ops(net, node, dy)
    net.close()


@pytest.mark.gpu
def test_in_place_activation_behind_the_node():
    """the relu rewrites att between forward and backward; the source gradients still are those of the float64 formulas for the
    gradient that reaches the node (1e-5 of the largest value, the bar of tests/test_attention.py)"""
    from bcnn_amd import capi
    from tests.test_attention import reference
    net, node = _net(capi.MODE_TRAIN, relu=True)
    _feed(net, 3)
    _feed(net, 4, 1)
    net.forward()
    net.backward()
    net.sync()
    ids = [net.node_src(node, i) for i in range(3)]
    q, k, v = [_data(net, i).astype(np.float64).reshape(2, HEADS, -1, 72) for i in ids]
    out, dy = _data(net, net.index("att")), _grad(net, net.index("att"))
    ref, _ = reference(q, k, v, dy.astype(np.float64).reshape(2, HEADS, -1, 72), 0.5)
    assert (out == 0).any() and (ref["o"] < 0).any() and np.abs(dy).max() > 0, "the relu did rewrite the output"
    for i, name in zip(ids, ("dq", "dk", "dv")):
        err, bar = np.abs(_grad(net, i).reshape(ref[name].shape) - ref[name]).max(), 1e-5 * np.abs(ref[name]).max()
        print("%s: max error %.3g, bar %.3g" % (name, err, bar))
        assert err <= bar, (name, err, bar)
    net.close()


@pytest.mark.gpu
def test_resize_refuses_k_and_v_of_different_extents():
    """k through a 2x2 / 2 convolution (floor(h / 2)), v through a max-pool (ceil(h / 2)): equal at 8 x 8, not at 7 x 7"""
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=8, h=8, c=4, n=2)
    net.conv(4, 2, 2, 0, src="input", dst="k")
    net.maxpool(2, 2, src="input", dst="v")
    node = net.add_attention(HEADS, "input", "k", "v", "att")
    net.compile()
    att = net.index("att")
    assert net.shape(net.index("k")) == net.shape(net.index("v")) == (2, 4, 4, 4)
    assert net.resize(7, 7, 4, need_realloc=True) == INVALID_PARAMETER
    assert net.shape(att) == (2, 4, 8, 8) and net.shape(net.index("k")) == (2, 4, 4, 4), "a refused resize changes nothing"
    assert net.resize(6, 6, 4, need_realloc=True) == 0 and net.shape(att) == (1, 4, 6, 6)
    net.forward_node(node)
    net.sync()
    net.close()


def test_builder_refusals_leave_the_node_count():
    """no node is built, so no device is needed: q, k, v are the input [2][8][4][4] and the label tensor in a shape set here"""
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_PREDICT, w=4, h=4, c=8, n=2)
    L, label = net.L, net.tensor(1)
    cases = [((2, 8, 4, 4), 2, (b"nope", b"input", b"input")),      # an unknown source, in each slot
             ((2, 8, 4, 4), 2, (b"input", b"nope", b"input")),
             ((2, 8, 4, 4), 2, (b"input", b"input", b"nope")),
             ((3, 8, 4, 4), 2, (b"input", b"input", b"label")),     # different N
             ((2, 4, 4, 4), 2, (b"input", b"label", b"input")),     # q / k channel mismatch
             ((2, 8, 2, 4), 2, (b"input", b"input", b"label")),     # k / v spatial mismatch
             ((2, 8, 4, 4), 0, (b"input", b"input", b"input")),     # heads <= 0
             ((2, 8, 4, 4), -2, (b"input", b"input", b"input")),
             ((2, 8, 4, 4), 3, (b"input", b"input", b"input")),     # heads dividing neither depth
             ((2, 6, 4, 4), 4, (b"input", b"input", b"label")),     # ... and only q's and k's
             ((2, 258, 4, 4), 2, (b"label", b"label", b"input")),   # d = 129
             ((2, 129, 4, 4), 1, (b"input", b"input", b"label")),   # c = 129
             ((2, 8, 32768, 8192), 2, (b"label", b"input", b"input"))]   # q (and the output) of 2^32 elements
    for shape, heads, (q, k, v) in cases:
        label.n, label.c, label.h, label.w = shape
        assert L.bcnn_add_attention_layer(net.net, heads, 0.0, q, k, v, b"att") == INVALID_PARAMETER, (shape, heads, q, k, v)
        assert L.bcnn_get_num_nodes(net.net) == 0 and not L.bcnn_peek_tensor(net.net, 2), "nothing was added"
    label.n = label.c = label.h = label.w = 0   # (the net owns no device memory; bcnn_end_net would ask for the device)


def test_both_libraries_export_the_new_symbols():
    from bcnn_amd import _lib, capi
    host, hip = C.CDLL(capi.LIB_PATH), C.CDLL(_lib.LIB_PATH)
    assert hasattr(host, "bcnn_add_attention_layer")
    for name in ("bcnn_hip_attention_forward", "bcnn_hip_attention_backward", "bcnn_hip_attention_lse_size"):
        assert hasattr(hip, name), name
