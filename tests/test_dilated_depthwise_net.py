"""The dilated depthwise node inside nets (bcnn_amd.capi): bcnn_add_dilated_depthwise_conv_layer, its workers, update, model
files, the `dilation` key of the [depthwise-conv] / [dw-conv] sections, the refusals, bcnn_resize_net, the bf16 mode and the
dispatch trace.

The node's output, source gradient and parameter gradients of a TRAIN step carry the bits of the bcnn_amd.ops calls on the same
inputs (tests/test_dilated_depthwise.py holds those to torch's float64 convolution). The node accumulates onto its source
gradient, and assigns it when it is the gradient's only writer, as the depthwise node does in the same position.
bcnn_update equals ops.sgd_update / ops.adam_update on copies."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SEED = 20261021
INVALID_PARAMETER = 1
OP_TOL = 1e-5      # tests/test_dilated_depthwise.py
CH, K, S, P, D = 4, 3, 1, 2, 2


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


def _set_params(net, node, seed):
    """non-trivial weights and biases (the builder fills the biases with 0)"""
    rs = np.random.RandomState(seed)
    for slot in (1, 2):
        i = net.node_src(node, slot)
        net.data(i)[...] = rs.uniform(-0.5, 0.5, net.shape(i))
        net.upload(i)


def _ops_forward(x, wt, b, k, s, p, d, act):
    from bcnn_amd import ops
    n, c, h, w = x.shape
    oh, ow = ops.dilated_conv_out_hw(h, w, k, s, p, d)
    ty = torch.full((n, c, oh, ow), float("nan"), device=DEV)
    ops.dilated_depthwise_forward(_t(x), _t(wt), _t(b), ty, k, s, p, d, act)
    torch.cuda.synchronize()
    return ty.cpu().numpy()


def _ops_backward(x, wt, y, dy, k, s, p, d, act, dx0=None):
    """(dy * act'(y), dx, dw, db) of the ops call; dx0 None: assigned into NaNs, else accumulated onto dx0"""
    from bcnn_amd import ops
    n, c, h, w = x.shape
    tdy = _t(dy)
    tdx = torch.full(x.shape, float("nan"), device=DEV) if dx0 is None else _t(dx0)
    tdw, tdb = _t(np.zeros(wt.size)), _t(np.zeros(c))
    ws = torch.zeros(ops.dilated_depthwise_workspace_size(n, c, h, w, k, s, p, d), device=DEV)
    ops.dilated_depthwise_backward(_t(x), _t(wt), _t(y), tdy, tdx, tdw, tdb, k, s, p, d, act, dx0 is None, ws)
    torch.cuda.synchronize()
    return tdy.cpu().numpy(), tdx.cpu().numpy(), tdw.cpu().numpy(), tdb.cpu().numpy()


def _torch_dx(x, wt, g, s, p, d):
    tx = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    z = torch.nn.functional.conv2d(tx, torch.tensor(np.asarray(wt, np.float64).reshape(-1, 1, K, K)), None, stride=s,
                                   padding=p, dilation=d, groups=x.shape[1])
    z.backward(torch.tensor(np.asarray(g, np.float64)))
    return tx.grad.numpy()


def _close(tag, got, want, tol=OP_TOL):
    bound = tol * float(np.abs(want).max())
    diff = float(np.abs(np.asarray(got, np.float64) - want).max())
    assert diff <= bound, "%s: max abs diff %.3g > %.3g" % (tag, diff, bound)


def _net(mode, head=True, act=None):
    """input [2][4][9][9] -> dilated depthwise 3x3 d=2 p=2, ReLU -> 1x1 convolution, 5 filters -> cost"""
    from bcnn_amd import capi
    C.CDLL(None).srand(SEED)   # the fillers draw from rand(): the same weights for every net built after the same seed
    net = capi.Net(mode=mode, w=9, h=9, c=CH, n=2, input_grad=mode == capi.MODE_TRAIN)
    node = net.dilated_depthwise(K, S, P, D, act=capi.ACT_RELU if act is None else act, src="input", dst="dd")
    if head:
        net.conv(5, 1, 1, 0, act=capi.ACT_NONE, src="dd", dst="pw")
        net.cost("pw", "label", "cost")
    net.compile()
    _set_params(net, node, 11)
    return net, node


def test_train_step_carries_the_bits_of_the_ops_calls_and_sgd_updates():
    from bcnn_amd import capi, ops
    net, node = _net(capi.MODE_TRAIN)
    lr, momentum, decay = 0.05, 0.9, 5e-4
    net.set_sgd(lr, momentum, decay)
    assert net.node_type(node) == capi.LAYER_DILATED_DEPTHWISE_CONV2D == 23
    assert net.node_activation(node) == capi.ACT_RELU
    dd, i_w, i_b = net.index("dd"), net.node_src(node, 1), net.node_src(node, 2)
    assert net.node_src(node, 0) == 0 and net.node_dst(node) == dd
    assert net.shape(dd) == (2, CH, 9, 9) and int(np.prod(net.shape(i_w))) == CH * 9 and int(np.prod(net.shape(i_b))) == CH
    assert net.tensor(i_w).name == b"input_w" and net.tensor(i_b).name == b"input_b"
    _feed(net, 3)
    net.forward()
    net.sync()
    x, wt, b = net.data(0).copy(), _data(net, i_w), _data(net, i_b).ravel()
    y = _ops_forward(x, wt, b, K, S, P, D, ops.ACT["relu"])
    assert np.array_equal(_bits(_data(net, dd)), _bits(y)), "node output"
    net.backward_node(2)   # cost, 1x1 convolution: what reaches the node, before it multiplies by act'(y) in place
    net.backward_node(1)
    net.sync()
    dy = _grad(net, dd)
    assert np.abs(dy).max() > 0
    net.backward_node(node)
    net.sync()
    g, dx, dw, db = _ops_backward(x, wt, y, dy, K, S, P, D, ops.ACT["relu"])
    assert np.array_equal(_bits(_grad(net, dd)), _bits(g)), "dy * act'(y)"
    # the node is the input gradient's only writer: assigned, and what torch gives
    assert np.array_equal(_bits(_grad(net, 0)), _bits(dx)), "source gradient"
    _close("source gradient", _grad(net, 0), _torch_dx(x, wt, g, S, P, D))
    g_w, g_b = _grad(net, i_w), _grad(net, i_b).ravel()
    assert np.array_equal(_bits(g_w.ravel()), _bits(dw)) and np.array_equal(_bits(g_b), _bits(db)), "parameter gradients"
    assert np.abs(g_w).max() > 0 and np.abs(g_b).max() > 0
    # the step: the one-launch SGD table
    tw, tb, tdw, tdb = _t(wt.ravel()), _t(b), _t(g_w.ravel()), _t(g_b)
    ops.sgd_update(tw, tb, tdw, tdb, 2, lr, momentum, decay)
    net.update()
    net.sync()
    assert np.array_equal(_bits(_data(net, i_w).ravel()), _bits(tw.cpu().numpy())), "weights after the step"
    assert np.array_equal(_bits(_data(net, i_b).ravel()), _bits(tb.cpu().numpy())), "biases after the step"
    assert not np.array_equal(_bits(tw.cpu().numpy()), _bits(wt.ravel()))
    net.close()


def test_source_gradient_accumulates_next_to_a_second_consumer():
    """input -> conv c1 -> {dilated depthwise on c1, eltwise(c1, that)} -> 1x1 conv -> cost"""
    from bcnn_amd import capi, ops
    C.CDLL(None).srand(SEED)
    net = capi.Net(mode=capi.MODE_TRAIN, w=9, h=9, c=3, n=2)
    net.conv(CH, 3, 1, 1, act=capi.ACT_NONE, src="input", dst="c1")
    node = net.dilated_depthwise(K, S, P, D, act=capi.ACT_NONE, src="c1", dst="dd")
    net.eltwise(capi.ACT_NONE, "c1", "dd", "sum")
    net.conv(5, 1, 1, 0, act=capi.ACT_NONE, src="sum", dst="pw")
    net.cost("pw", "label", "cost")
    net.compile()
    _set_params(net, node, 12)
    _feed(net, 5)
    net.forward()
    for k in (4, 3, 2):   # cost, 1x1 convolution, eltwise
        net.backward_node(k)
    net.sync()
    c1, dd = net.index("c1"), net.index("dd")
    share, dy = _grad(net, c1), _grad(net, dd)   # what the eltwise node left on c1, and what reaches the node
    assert np.abs(share).max() > 0 and np.abs(dy).max() > 0
    net.backward_node(node)
    net.sync()
    got = _grad(net, c1)
    x, wt, y = _data(net, c1), _data(net, net.node_src(node, 1)), _data(net, dd)
    _, dx, _, _ = _ops_backward(x, wt, y, dy, K, S, P, D, ops.ACT["none"], dx0=share)
    assert np.array_equal(_bits(got), _bits(dx)), "the eltwise share plus the node's data gradient"
    _close("share + dx", got, share.astype(np.float64) + _torch_dx(x, wt, dy, S, P, D))
    assert float(np.abs(got - share).max()) > 0
    net.close()


CFG = """
[network]
input_width=9
input_height=9
input_channels=4
batch_size=2
%s
[%s]
size=3
stride=1
pad=%d
%ssrc=input
dst=dd
%s"""
ADAM = "optimizer=adam\nlearning_rate=0.01\nmomentum=0.9\ndecay=0.0005\nbeta1=0.9\nbeta2=0.999\n"
HEAD = """
[convolutional]
filters=5
size=1
stride=1
pad=0
src=dd
dst=pw

[cost]
src=pw
dst=out
loss=euclidean
metric=error
"""


def _load(tmp_path, text, mode, name="net.cfg", model=None):
    from bcnn_amd import capi
    cfg = tmp_path / name
    cfg.write_text(text)
    C.CDLL(None).srand(SEED)
    net = capi.Net.load_net(str(cfg), model, mode=mode)
    net.compile()
    return net


def test_adam_from_a_config_equals_the_ops_step(tmp_path):
    from bcnn_amd import capi, ops
    net = _load(tmp_path, CFG % (ADAM, "depthwise-conv", 2, "dilation=2\nfunction=relu\n", HEAD), capi.MODE_TRAIN)
    assert net.node_type(0) == capi.LAYER_DILATED_DEPTHWISE_CONV2D
    _set_params(net, 0, 13)
    i_w, i_b = net.node_src(0, 1), net.node_src(0, 2)
    m, v = _t(np.zeros(CH * 9)), _t(np.zeros(CH * 9))
    for step in range(2):
        _feed(net, 20 + step)
        net.forward()
        net.backward()
        net.sync()
        wt, b = _data(net, i_w), _data(net, i_b).ravel()
        tw, tb, tdw, tdb = _t(wt.ravel()), _t(b), _t(_grad(net, i_w).ravel()), _t(_grad(net, i_b).ravel())
        assert float(tdw.abs().max()) > 0
        ops.adam_update(tw, tb, tdw, tdb, m, v, 2, (step + 1) * 2, 0.9, 0.999, 0.01, 0.9, 0.0005)
        net.update()
        net.sync()
        assert np.array_equal(_bits(_data(net, i_w).ravel()), _bits(tw.cpu().numpy())), "weights, step %d" % step
        assert np.array_equal(_bits(_data(net, i_b).ravel()), _bits(tb.cpu().numpy())), "biases, step %d" % step
        assert not np.array_equal(_bits(tw.cpu().numpy()), _bits(wt.ravel()))
    net.close()


def test_model_file_round_trip(tmp_path):
    from bcnn_amd import capi
    a, node = _net(capi.MODE_TRAIN)
    path = str(tmp_path / "dd.bcnnmodel")
    assert a.save_weights(path) == 0
    blob = open(path, "rb").read()
    assert len(blob) == 16 + 4 * (CH + CH * 9 + 5 + 5 * CH)
    in_file = np.frombuffer(blob[16:16 + 4 * (CH + CH * 9)], F32)   # biases, then weights
    assert np.array_equal(_bits(in_file[:CH]), _bits(_data(a, a.node_src(node, 2)).ravel()))
    assert np.array_equal(_bits(in_file[CH:]), _bits(_data(a, a.node_src(node, 1)).ravel()))
    C.CDLL(None).srand(SEED + 1)   # other weights until the file is read
    b = capi.Net(mode=capi.MODE_PREDICT, w=9, h=9, c=CH, n=2)
    node_b = b.dilated_depthwise(K, S, P, D, act=capi.ACT_RELU, src="input", dst="dd")
    b.conv(5, 1, 1, 0, act=capi.ACT_NONE, src="dd", dst="pw")
    b.compile()
    assert not np.array_equal(_bits(_data(a, a.node_src(node, 1))), _bits(_data(b, b.node_src(node_b, 1))))
    assert b.load_weights(path) == 0
    for slot in (1, 2):
        assert np.array_equal(_bits(_data(a, a.node_src(node, slot))), _bits(_data(b, b.node_src(node_b, slot)))), slot
    a.set_mode(capi.MODE_PREDICT)
    for net in (a, b):
        _feed(net, 8, label=False)
        net.forward()
        net.sync()
    for name in ("dd", "pw"):
        out = _data(a, a.index(name))
        assert np.abs(out).max() > 0
        assert np.array_equal(_bits(out), _bits(_data(b, b.index(name)))), name
    a.close()
    b.close()


@pytest.mark.parametrize("section", ["depthwise-conv", "dw-conv"])
def test_config_dilation_key_builds_the_node(tmp_path, section):
    from bcnn_amd import capi, ops
    net = _load(tmp_path, CFG % ("", section, 2, "dilation=2\nactivation=relu\n", ""), capi.MODE_PREDICT)
    assert net.num_nodes == 1 and net.node_type(0) == capi.LAYER_DILATED_DEPTHWISE_CONV2D
    assert net.node_activation(0) == capi.ACT_RELU
    assert net.shape(net.index("dd")) == (2, CH, 9, 9)   # an undilated 3x3 with pad 2 would give 11 x 11
    _set_params(net, 0, 14)
    _feed(net, 4, label=False)
    net.forward()
    net.sync()
    y = _ops_forward(net.data(0).copy(), _data(net, net.node_src(0, 1)), _data(net, net.node_src(0, 2)).ravel(), K, S, P, D,
                     ops.ACT["relu"])
    assert np.array_equal(_bits(_data(net, net.index("dd"))), _bits(y))
    net.close()
    # an activation that needs the layer's input: the node with no activation and the in-place node, as for the other sections
    net = _load(tmp_path, CFG % ("", section, 2, "dilation=2\nactivation=swish\n", ""), capi.MODE_PREDICT)
    assert [net.node_type(k) for k in range(net.num_nodes)] == [capi.LAYER_DILATED_DEPTHWISE_CONV2D, capi.LAYER_ACTIVATION]
    assert net.node_activation(0) == capi.ACT_NONE and net.node_activation(1) == capi.ACT_SWISH
    net.close()


def test_config_section_predicts_what_torch_gives_from_the_loaded_weights(tmp_path):
    """Without the change the section built a dense 3x3 at pad 2: an 11 x 11 output of other values."""
    from bcnn_amd import capi
    text = CFG % ("", "depthwise-conv", 2, "dilation=2\nactivation=relu\n", "")
    first = _load(tmp_path, text, capi.MODE_PREDICT)
    _set_params(first, 0, 15)
    wt, b = _data(first, first.node_src(0, 1)).ravel().copy(), _data(first, first.node_src(0, 2)).ravel().copy()
    path = str(tmp_path / "dd.bcnnmodel")
    assert first.save_weights(path) == 0
    first.close()
    C.CDLL(None).srand(SEED + 2)
    net = _load(tmp_path, text, capi.MODE_PREDICT, model=path)
    assert np.array_equal(_bits(_data(net, net.node_src(0, 1)).ravel()), _bits(wt))
    assert np.array_equal(_bits(_data(net, net.node_src(0, 2)).ravel()), _bits(b))
    _feed(net, 6, label=False)
    net.forward()
    net.sync()
    x = net.data(0).copy()
    want = torch.nn.functional.conv2d(torch.tensor(x, dtype=torch.float64),
                                      torch.tensor(wt.astype(np.float64).reshape(CH, 1, 3, 3)),
                                      torch.tensor(b.astype(np.float64)), stride=1, padding=2, dilation=2, groups=CH)
    want = torch.relu(want).numpy()
    got = _data(net, net.index("dd"))
    assert got.shape == want.shape == (2, CH, 9, 9)
    _close("prediction", got, want)
    net.close()


def test_config_without_dilation_builds_the_depthwise_node_as_before(tmp_path):
    from bcnn_amd import capi
    C.CDLL(None).srand(SEED)
    twin = capi.Net(mode=capi.MODE_PREDICT, w=9, h=9, c=CH, n=2)
    twin.depthwise(3, 1, 1, act=capi.ACT_RELU, src="input", dst="dd")
    twin.compile()
    _set_params(twin, 0, 16)
    path = str(tmp_path / "dw.bcnnmodel")
    assert twin.save_weights(path) == 0
    outs = []
    for name, keys in (("none.cfg", "activation=relu\n"), ("one.cfg", "dilation=1\nactivation=relu\n")):
        net = _load(tmp_path, CFG % ("", "depthwise-conv", 1, keys, ""), capi.MODE_PREDICT, name, model=path)
        assert net.num_nodes == 1 and net.node_type(0) == capi.LAYER_DEPTHWISE_CONV2D == 2
        assert net.shape(net.index("dd")) == (2, CH, 9, 9)
        outs.append(net)
    for net in outs + [twin]:
        _feed(net, 7, label=False)
        net.forward()
        net.sync()
    want = _data(twin, twin.index("dd"))
    assert np.abs(want).max() > 0
    for net in outs:
        assert np.array_equal(_bits(_data(net, net.index("dd"))), _bits(want))
        net.close()
    twin.close()


def test_refusals_leave_the_node_count_and_resize_is_refused():
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=8, h=6, c=3, n=2)
    net.conv(6, 3, 1, 1, src="input", dst="c1")
    L = net.L
    bad = [(3, 1, 2, 2, capi.ACT_NONE, b"no_such_tensor"),
           (0, 1, 2, 2, capi.ACT_NONE, b"c1"), (-3, 1, 2, 2, capi.ACT_NONE, b"c1"),
           (3, 0, 2, 2, capi.ACT_NONE, b"c1"), (3, 1, -1, 2, capi.ACT_NONE, b"c1"),
           (3, 1, 2, 0, capi.ACT_NONE, b"c1"), (3, 1, 2, -2, capi.ACT_NONE, b"c1"),
           (3, 1, 0, 3, capi.ACT_NONE, b"c1"),      # height 6 - 3 * 2 - 1 < 0
           (3, 1, 2, 2, capi.ACT_PRELU, b"c1"),
           (3, 1, 2, 2, capi.ACT_HARD_SWISH, b"c1"), (3, 1, 2, 2, capi.ACT_SWISH, b"c1"),
           (3, 1, 2, 2, capi.ACT_MISH, b"c1")]
    for k, s, p, d, act, src in bad:
        st = L.bcnn_add_dilated_depthwise_conv_layer(net.net, k, s, p, d, capi.FILLER_XAVIER, act, src, b"dd")
        assert st == INVALID_PARAMETER, (k, s, p, d, act, src)
        assert L.bcnn_get_num_nodes(net.net) == 1
        assert net.index("dd") < 0
    node = net.dilated_depthwise(3, 1, 2, 2, act=capi.ACT_RELU, src="c1", dst="dd")
    assert net.node_type(node) == capi.LAYER_DILATED_DEPTHWISE_CONV2D and net.shape(net.index("dd")) == (2, 6, 6, 8)
    one = net.dilated_depthwise(3, 1, 1, 1, act=capi.ACT_RELU, src="dd", dst="plain")   # dilation 1: a depthwise node
    assert net.node_type(one) == capi.LAYER_DEPTHWISE_CONV2D
    net.compile()
    last = net.index("plain")
    before = [net.shape(i) for i in range(last + 1)]
    assert net.resize(12, 10, 3) == INVALID_PARAMETER
    assert net.resize(12, 10, 3, need_realloc=False) == INVALID_PARAMETER
    assert [net.shape(i) for i in range(last + 1)] == before
    net.close()


def test_bf16_mode_leaves_the_node_fp32():
    from bcnn_amd import capi
    net, node = _net(capi.MODE_PREDICT, head=False)
    _feed(net, 9, label=False)
    net.forward()
    net.sync()
    fp32 = _data(net, net.index("dd"))
    assert net.set_inference_precision(capi.PRECISION_BF16) == 0
    net.data(net.index("dd"))[...] = 0
    net.upload(net.index("dd"))
    net.forward()
    net.sync()
    assert np.abs(fp32).max() > 0 and np.array_equal(_bits(_data(net, net.index("dd"))), _bits(fp32))
    net.close()


def test_trace_names_the_kernels():
    from bcnn_amd import _lib, capi
    net, node = _net(capi.MODE_TRAIN)
    _feed(net, 10)
    L = _lib.load()
    L.bcnn_hip_trace_enable(1)
    net.forward()
    net.backward()
    net.sync()
    n = L.bcnn_hip_trace_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    names = buf.value.decode().split()
    for want in ("ddw_fwd_lds_kernel:plane", "ddw_bwd_lds_kernel:plane"):
        assert names.count(want) == 1, (want, names)
    net.close()
