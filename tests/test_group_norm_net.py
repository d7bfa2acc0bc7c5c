"""The group-normalisation node inside nets (bcnn_amd.capi): bcnn_add_groupnorm_layer, its workers, update, model files, the
config sections and bcnn_resize_net.

The node's output, the source gradient and the two parameter gradients of a TRAIN step carry the bits of the bcnn_amd.ops
calls on the same inputs (tests/test_group_norm.py holds those to float64); bcnn_update equals ops.sgd_update on copies (the
scales by the weights' rule, the biases by the biases'). PREDICT gives the same output bits and owns no statistics. With a
second consumer of the source the node adds to what that consumer left. Parameters survive a model file. [groupnorm] / [gn] /
[layernorm] / [instancenorm] build the node with 3, 3, 1 and C groups. Every refusal leaves the node count as it was.
bcnn_resize_net: the statistics follow N * groups, which a resize (batch 1) never grows, so its buffer holds every shape the
call can produce; with need_realloc the forward at the larger extent is the ops call at that shape."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SEED = 20261020
INVALID_PARAMETER, INVALID_MODEL = 1, 3


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


def _t(a):
    return torch.tensor(np.array(a, F32), device=DEV)


def _feed(net, seed, label=True):
    rs = np.random.RandomState(seed)
    net.data(0)[...] = rs.uniform(-1, 1, net.shape(0))
    net.upload(0)
    if label:
        net.data(1)[...] = rs.uniform(-1, 1, net.shape(1))
        net.upload(1)


def _data(net, idx):
    net.download(idx, False)
    return net.data(idx).copy()


def _grad(net, idx):
    net.download(idx, True)
    return net.grad(idx).copy()


def _state(net, node, count):
    from bcnn_amd import _lib
    got = torch.empty(count, dtype=torch.float32, device=DEV)
    _lib.load().bcnn_hip_memcpy_d2d(got.data_ptr(), net.node_state(node, 0), count * 4)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _set_params(net, node, seed):
    """non-trivial scales and biases (the builder fills 1 and 0)"""
    rs = np.random.RandomState(seed)
    for slot, lo, hi in ((1, 0.5, 1.5), (2, -1.0, 1.0)):
        i = net.node_src(node, slot)
        net.data(i)[...] = rs.uniform(lo, hi, net.shape(i))
        net.upload(i)


def _net(mode, groups=3, head=True, shape=(2, 3, 5, 5), second_consumer=False):
    """input -> conv 3x3 -> 6 -> groupnorm -> [relu in place | eltwise with the conv output] -> fc 4 -> cost"""
    from bcnn_amd import capi
    n, c, h, w = shape
    C.CDLL(None).srand(SEED)   # the fillers draw from rand(): the same weights for every net built after the same seed
    net = capi.Net(mode=mode, w=w, h=h, c=c, n=n)
    net.conv(6, 3, 1, 1, act=capi.ACT_NONE, src="input", dst="c1")
    node = net.groupnorm(groups, "c1", "gn")
    last = "gn"
    if second_consumer:
        net.eltwise(capi.ACT_NONE, "c1", "gn", "sum")
        last = "sum"
    elif head:
        net.activation(capi.ACT_RELU, "gn")
    if head:
        net.fullc(4, src=last, dst="fc")
        net.cost("fc", "label", "cost")
    net.compile()
    _set_params(net, node, 11)
    return net, node


def _ops_forward(x, gamma, beta, groups, eps=1e-5):
    from bcnn_amd import ops
    n, c = x.shape[:2]
    tx, ty = _t(x), _t(np.zeros_like(x))
    tm, tr = _t(np.zeros(n * groups)), _t(np.zeros(n * groups))
    ops.group_norm_forward(tx, _t(gamma), _t(beta), ty, tm, tr, groups, eps)
    torch.cuda.synchronize()
    return ty.cpu().numpy(), tm.cpu().numpy(), tr.cpu().numpy()


def _ops_backward(x, gamma, mean, rstd, dy, groups, dx0=None):
    from bcnn_amd import ops
    c = x.shape[1]
    tdx = _t(np.full_like(x, 5.0) if dx0 is None else dx0)
    tdg, tdb = _t(np.zeros(c)), _t(np.zeros(c))
    ops.group_norm_backward(_t(x), _t(gamma), _t(mean), _t(rstd), _t(dy), tdx, tdg, tdb, groups, overwrite=dx0 is None)
    torch.cuda.synchronize()
    return tdx.cpu().numpy(), tdg.cpu().numpy(), tdb.cpu().numpy()


def test_train_step_carries_the_bits_of_the_ops_calls():
    from bcnn_amd import capi, ops
    net, node = _net(capi.MODE_TRAIN)
    lr, momentum, decay = 0.05, 0.9, 5e-4
    net.set_sgd(lr, momentum, decay)
    assert net.node_type(node) == capi.LAYER_GROUPNORM and net.node_activation(node) == -1
    c1, gn = net.index("c1"), net.index("gn")
    i_scales, i_b = net.node_src(node, 1), net.node_src(node, 2)
    assert net.node_src(node, 0) == c1 and net.node_dst(node) == gn
    assert net.shape(i_scales) == (1, 1, 1, 6) and net.shape(i_b) == (1, 1, 1, 6)
    assert net.L.bcnn_grad_sole_writer(net.net, c1) == 1   # the only consumer of c1: it assigns
    _feed(net, 3)
    net.forward()
    net.backward()
    net.sync()
    x, gamma, beta = _data(net, c1), _data(net, i_scales).ravel(), _data(net, i_b).ravel()
    y, mean, rstd = _ops_forward(x, gamma, beta, 3)
    ty = _t(y)
    ops.activation_forward(ty, ops.ACT["relu"])   # the in-place node behind it
    assert np.array_equal(_bits(_data(net, gn)), _bits(ty.cpu().numpy())), "node output"
    stats = _state(net, node, 2 * 2 * 3)
    assert np.array_equal(_bits(stats[:6]), _bits(mean)) and np.array_equal(_bits(stats[6:]), _bits(rstd)), "mean, rstd"
    dy = _grad(net, gn)
    assert np.abs(dy).max() > 0
    dx, dg, db = _ops_backward(x, gamma, mean, rstd, dy, 3)
    assert np.array_equal(_bits(_grad(net, c1)), _bits(dx)), "source gradient"
    g_scales, g_b = _grad(net, i_scales).ravel(), _grad(net, i_b).ravel()
    assert np.array_equal(_bits(g_scales), _bits(dg)) and np.array_equal(_bits(g_b), _bits(db)), "parameter gradients"
    assert np.abs(g_scales).max() > 0 and np.abs(g_b).max() > 0
    # the step: scales as weights (with decay), biases as biases
    tw, tb, tdw, tdb = _t(gamma), _t(beta), _t(g_scales), _t(g_b)
    ops.sgd_update(tw, tb, tdw, tdb, 2, lr, momentum, decay)
    net.update()
    net.sync()
    assert np.array_equal(_bits(_data(net, i_scales).ravel()), _bits(tw.cpu().numpy())), "scales after the step"
    assert np.array_equal(_bits(_data(net, i_b).ravel()), _bits(tb.cpu().numpy())), "biases after the step"
    assert not np.array_equal(_bits(tw.cpu().numpy()), _bits(gamma))
    net.close()


def test_predict_gives_the_same_bits_and_owns_no_statistics():
    from bcnn_amd import capi
    train, node = _net(capi.MODE_TRAIN)
    pred, node_p = _net(capi.MODE_PREDICT)
    valid, node_v = _net(capi.MODE_VALID)
    assert train.node_state(node, 0) and valid.node_state(node_v, 0)
    assert not pred.node_state(node_p, 0) and not pred.node_state(node_p, 1)
    outs = []
    for net in (train, pred, valid):
        _feed(net, 4)
        net.forward()
        net.sync()
        outs.append(_data(net, net.index("gn")))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[0]), _bits(outs[2]))
    assert np.abs(outs[0]).max() > 0
    for net in (train, pred, valid):
        net.close()


def test_first_node_of_a_net_and_a_source_without_gradient():
    """the node reads the net input; the input has no gradient, so only the parameter gradients are written"""
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=5, h=5, c=6, n=2)
    node = net.groupnorm(2, "input", "gn", eps=1e-3)
    net.fullc(4, src="gn", dst="fc")
    net.cost("fc", "label", "cost")
    net.compile()
    _set_params(net, node, 2)
    _feed(net, 6)
    net.forward()
    net.backward()
    net.sync()
    x = net.data(0).copy()
    gamma, beta = _data(net, net.node_src(node, 1)).ravel(), _data(net, net.node_src(node, 2)).ravel()
    y, mean, rstd = _ops_forward(x, gamma, beta, 2, eps=1e-3)
    assert np.array_equal(_bits(_data(net, net.index("gn"))), _bits(y))
    _, dg, db = _ops_backward(x, gamma, mean, rstd, _grad(net, net.index("gn")), 2)
    assert np.array_equal(_bits(_grad(net, net.node_src(node, 1)).ravel()), _bits(dg))
    assert np.array_equal(_bits(_grad(net, net.node_src(node, 2)).ravel()), _bits(db))
    net.close()


def test_two_consumers_of_the_source_accumulate():
    from bcnn_amd import capi
    net, node = _net(capi.MODE_TRAIN, second_consumer=True)
    c1, gn, total = net.index("c1"), net.index("gn"), net.index("sum")
    assert net.L.bcnn_grad_sole_writer(net.net, c1) == 0   # the eltwise node writes it too: no mark, the fill stays
    _feed(net, 5)
    net.forward()
    net.backward()
    net.sync()
    x, gamma, beta = _data(net, c1), _data(net, net.node_src(node, 1)).ravel(), _data(net, net.node_src(node, 2)).ravel()
    _, mean, rstd = _ops_forward(x, gamma, beta, 3)
    d_sum, dy = _grad(net, total), _grad(net, gn)
    assert np.array_equal(_bits(dy), _bits(d_sum))           # the eltwise node hands its gradient to its first operand ...
    share = d_sum.copy()
    share[1:] = 0   # ... and, same-size operands, to image 0 of the second (the reference's quirk, bcnn_layers_next.c)
    assert np.abs(share).max() > 0
    dxv, _, _ = _ops_backward(x, gamma, mean, rstd, dy, 3)
    assert np.array_equal(_bits(_grad(net, c1)), _bits(share + dxv)), "the eltwise share plus the node's"
    acc, _, _ = _ops_backward(x, gamma, mean, rstd, dy, 3, dx0=share)
    assert np.array_equal(_bits(_grad(net, c1)), _bits(acc))
    net.close()


def test_model_file_round_trip_and_a_short_file(tmp_path):
    from bcnn_amd import capi
    a, node = _net(capi.MODE_TRAIN)
    _set_params(a, node, 23)
    path = str(tmp_path / "gn.bcnnmodel")
    assert a.save_weights(path) == 0
    blob = open(path, "rb").read()
    conv_floats = 6 * 3 * 3 * 3 + 6
    fc_floats = 4 * 6 * 5 * 5 + 4
    assert len(blob) == 16 + 4 * (conv_floats + 2 * 6 + fc_floats)
    # behind the convolution: the node's biases, then its scales
    at = 16 + 4 * conv_floats
    in_file = np.frombuffer(blob[at:at + 48], F32)
    assert np.array_equal(_bits(in_file[:6]), _bits(_data(a, a.node_src(node, 2)).ravel()))
    assert np.array_equal(_bits(in_file[6:]), _bits(_data(a, a.node_src(node, 1)).ravel()))
    b, node_b = _net(capi.MODE_PREDICT)
    assert b.load_weights(path) == 0
    for slot in (1, 2):
        assert np.array_equal(_bits(_data(a, a.node_src(node, slot))), _bits(_data(b, b.node_src(node_b, slot)))), slot
    for net in (a, b):
        _feed(net, 8, label=net is a)
        net.forward()
        net.sync()
    assert np.array_equal(_bits(_data(a, a.index("gn"))), _bits(_data(b, b.index("gn"))))
    # a file that ends inside the node's scales
    short = str(tmp_path / "short.bcnnmodel")
    open(short, "wb").write(blob[:at + 4 * 9])
    assert b.load_weights(short) == INVALID_MODEL
    a.close()
    b.close()


CFG = """
[net]
input_width=5
input_height=5
input_channels=3
batch_size=2

[conv]
filters=6
size=3
stride=1
pad=1
src=input
dst=c1

[groupnorm]
groups=3
src=c1
dst=a

[gn]
num_groups=3
eps=0.001
src=a
dst=b

[layernorm]
src=b
dst=c

[instancenorm]
src=c
dst=d
"""


def test_config_sections(tmp_path):
    from bcnn_amd import capi
    cfg = tmp_path / "gn.cfg"
    cfg.write_text(CFG)
    C.CDLL(None).srand(SEED)
    net = capi.Net.load_net(str(cfg), None, mode=capi.MODE_PREDICT)
    net.compile()
    assert net.num_nodes == 5
    assert [net.node_type(k) for k in range(1, 5)] == [capi.LAYER_GROUPNORM] * 4
    for k in range(1, 5):
        _set_params(net, k, 30 + k)
    _feed(net, 9, label=False)
    net.forward()
    net.sync()
    # the groups each section built, read off what it computes: 3, 3, 1 and C
    src = "c1"
    for k, (dst, groups, eps) in enumerate((("a", 3, 1e-5), ("b", 3, 1e-3), ("c", 1, 1e-5), ("d", 6, 1e-5)), start=1):
        x = _data(net, net.index(src))
        gamma, beta = _data(net, net.node_src(k, 1)).ravel(), _data(net, net.node_src(k, 2)).ravel()
        y, _, _ = _ops_forward(x, gamma, beta, groups, eps)
        assert np.array_equal(_bits(_data(net, net.index(dst))), _bits(y)), dst
        for other in {1, 2, 3, 6} - {groups}:
            assert not np.array_equal(_bits(_ops_forward(x, gamma, beta, other, eps)[0]), _bits(y)), (dst, other)
        src = dst
    net.close()


@pytest.mark.parametrize("section", ["[groupnorm]\n", "[groupnorm]\ngroups=4\n", "[gn]\ngroups=0\n", "[gn]\ngroups=-3\n",
                                     "[groupnorm]\ngroups=3\nactivation=relu\n", "[layernorm]\nfunction=relu\n",
                                     "[instancenorm]\nactivation=mish\n"])
def test_config_refusals_leave_the_node_count(tmp_path, section):
    from bcnn_amd import capi
    cfg = tmp_path / "bad.cfg"
    cfg.write_text(CFG.split("[groupnorm]")[0] + section + "src=c1\ndst=a\n")
    L = capi.lib()
    net = C.c_void_p()
    assert L.bcnn_init_net(C.byref(net), capi.MODE_PREDICT) == 0
    L.bcnn_set_log_context(net, None, capi.LOG_SILENT)
    assert L.bcnn_load_net(net, str(cfg).encode(), None) == INVALID_PARAMETER
    assert L.bcnn_get_num_nodes(net) == 1   # the convolution in front of the refused section
    L.bcnn_end_net(C.byref(net))


def test_builder_refusals_leave_the_node_count():
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=5, h=5, c=3, n=2)
    net.conv(6, 3, 1, 1, src="input", dst="c1")
    tensors = 0
    while net.L.bcnn_peek_tensor(net.net, tensors):
        tensors += 1
    for groups, src in ((4, b"c1"), (5, b"c1"), (0, b"c1"), (-2, b"c1"), (12, b"c1"), (3, b"no_such_tensor")):
        assert net.L.bcnn_add_groupnorm_layer(net.net, groups, 0.0, src, b"gn") == INVALID_PARAMETER, (groups, src)
        assert net.L.bcnn_get_num_nodes(net.net) == 1
        assert not net.L.bcnn_peek_tensor(net.net, tensors), "no tensor was added either"
    assert net.L.bcnn_add_groupnorm_layer(net.net, 6, 0.0, b"c1", b"gn") == 0
    assert net.L.bcnn_get_num_nodes(net.net) == 2
    net.close()


def test_resize_follows_the_statistics_by_rows():
    """bcnn_resize_net sets the batch to 1: N * groups never grows, so the statistics buffer (2 N groups floats) holds every
    shape a resize can produce, with and without need_realloc; the tensors follow the call's own contract"""
    from bcnn_amd import capi
    net, node = _net(capi.MODE_TRAIN, head=False, shape=(2, 3, 8, 8))
    gn = net.index("gn")
    state = net.node_state(node, 0)
    assert net.resize(6, 6, 3, need_realloc=False) == 0 and net.shape(gn) == (1, 6, 6, 6)
    assert net.node_state(node, 0) == state
    assert net.resize(12, 12, 3, need_realloc=True) == 0 and net.shape(gn) == (1, 6, 12, 12)
    assert net.node_state(node, 0) == state, "one row count fewer: nothing to grow"
    _feed(net, 12, label=False)
    net.forward()
    net.sync()
    x = _data(net, net.index("c1"))
    assert x.shape == (1, 6, 12, 12)
    gamma, beta = _data(net, net.node_src(node, 1)).ravel(), _data(net, net.node_src(node, 2)).ravel()
    y, mean, rstd = _ops_forward(x, gamma, beta, 3)
    assert np.array_equal(_bits(_data(net, gn)), _bits(y)), "forward at the new shape"
    stats = _state(net, node, 6)
    assert np.array_equal(_bits(stats[:3]), _bits(mean)) and np.array_equal(_bits(stats[3:]), _bits(rstd))
    net.backward_node(node)   # the backward runs at the new shape
    net.sync()
    net.close()
