"""The dilated-convolution node inside nets (bcnn_amd.capi): bcnn_add_dilated_conv_layer, its workers, update, model files,
the `dilation` key of the config sections, the refusals, bcnn_resize_net, the bf16 mode and the dispatch trace.

The node's output, source gradient and parameter gradients of a TRAIN step carry the bits of the bcnn_amd.ops calls on the same
inputs (tests/test_dilated_conv.py holds those to torch's float64 convolution). The node overwrites its source gradient, as a
convolution node does in the same position. bcnn_update equals ops.sgd_update / ops.adam_update on copies."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SEED = 20261021
INVALID_PARAMETER, INVALID_MODEL = 1, 3
NET_TOL = 1e-4     # tests/test_net_parity.py


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


def _set_biases(net, node, seed):
    """non-trivial biases (the builder fills 0)"""
    i = net.node_src(node, 2)
    net.data(i)[...] = np.random.RandomState(seed).uniform(-0.5, 0.5, net.shape(i))
    net.upload(i)


def _ops_forward(x, wt, b, f, k, s, p, d, g, act):
    from bcnn_amd import ops
    n, c, h, w = x.shape
    oh, ow = ops.dilated_conv_out_hw(h, w, k, s, p, d)
    ty = torch.full((n, f, oh, ow), float("nan"), device=DEV)
    ops.dilated_conv_forward(_t(x), _t(wt), _t(b), ty, k, s, p, d, g, act)
    torch.cuda.synchronize()
    return ty.cpu().numpy()


def _ops_backward(x, wt, y, dy, k, s, p, d, g, act, dw0=None, db0=None):
    """(dy * act'(y), dx, dw, db) of the ops call with the workspace the node sizes for itself"""
    from bcnn_amd import ops
    n, c, h, w = x.shape
    f = y.shape[1]
    tdy, tdx = _t(dy), torch.full(x.shape, float("nan"), device=DEV)
    tdw = _t(np.zeros(wt.shape) if dw0 is None else dw0)
    tdb = _t(np.zeros(f) if db0 is None else db0)
    ws = torch.zeros(ops.dilated_conv_workspace_size(n, c, h, w, f, k, s, p, d, g), device=DEV)
    ops.dilated_conv_backward(_t(x), _t(wt), _t(y), tdy, tdx, tdw, tdb, k, s, p, d, g, act, ws)
    torch.cuda.synchronize()
    return tdy.cpu().numpy(), tdx.cpu().numpy(), tdw.cpu().numpy(), tdb.cpu().numpy()


def _net(mode, head=True, act=None):
    """input [2][3][7][7] -> dilated 3x3 d=2 p=2, 6 filters, ReLU -> fc 4 -> cost"""
    from bcnn_amd import capi
    C.CDLL(None).srand(SEED)   # the fillers draw from rand(): the same weights for every net built after the same seed
    net = capi.Net(mode=mode, w=7, h=7, c=3, n=2, input_grad=mode == capi.MODE_TRAIN)
    node = net.dilated_conv(6, 3, 1, 2, 2, act=capi.ACT_RELU if act is None else act, src="input", dst="dc")
    if head:
        net.fullc(4, src="dc", dst="fc")
        net.cost("fc", "label", "cost")
    net.compile()
    _set_biases(net, node, 11)
    return net, node


def test_train_step_carries_the_bits_of_the_ops_calls_and_sgd_updates():
    from bcnn_amd import capi, ops
    net, node = _net(capi.MODE_TRAIN)
    lr, momentum, decay = 0.05, 0.9, 5e-4
    net.set_sgd(lr, momentum, decay)
    assert net.node_type(node) == capi.LAYER_DILATED_CONV2D and net.node_activation(node) == capi.ACT_RELU
    dc, i_w, i_b = net.index("dc"), net.node_src(node, 1), net.node_src(node, 2)
    assert net.node_src(node, 0) == 0 and net.node_dst(node) == dc
    assert net.shape(dc) == (2, 6, 7, 7) and net.shape(i_w) == (6, 3, 3, 3) and net.shape(i_b) == (1, 1, 1, 6)
    assert net.tensor(i_w).name == b"input_w" and net.tensor(i_b).name == b"input_b"
    _feed(net, 3)
    net.forward()
    net.sync()
    x, wt, b = net.data(0).copy(), _data(net, i_w), _data(net, i_b).ravel()
    assert np.abs(wt).max() > 0
    y = _ops_forward(x, wt, b, 6, 3, 1, 2, 2, 1, ops.ACT["relu"])
    assert np.array_equal(_bits(_data(net, dc)), _bits(y)), "node output"
    net.backward_node(2)   # cost, fc: what reaches the node, before it multiplies by act'(y) in place
    net.backward_node(1)
    net.sync()
    dy = _grad(net, dc)
    assert np.abs(dy).max() > 0
    net.backward_node(node)
    net.sync()
    g, dx, dw, db = _ops_backward(x, wt, y, dy, 3, 1, 2, 2, 1, ops.ACT["relu"])
    assert np.array_equal(_bits(_grad(net, dc)), _bits(g)), "dy * act'(y)"
    assert np.array_equal(_bits(_grad(net, 0)), _bits(dx)), "source gradient"
    g_w, g_b = _grad(net, i_w), _grad(net, i_b).ravel()
    assert np.array_equal(_bits(g_w), _bits(dw)) and np.array_equal(_bits(g_b), _bits(db)), "parameter gradients"
    assert np.abs(g_w).max() > 0 and np.abs(g_b).max() > 0
    # the step: the one-launch SGD table
    tw, tb, tdw, tdb = _t(wt), _t(b), _t(g_w), _t(g_b)
    ops.sgd_update(tw, tb, tdw, tdb, 2, lr, momentum, decay)
    net.update()
    net.sync()
    assert np.array_equal(_bits(_data(net, i_w)), _bits(tw.cpu().numpy().reshape(wt.shape))), "weights after the step"
    assert np.array_equal(_bits(_data(net, i_b).ravel()), _bits(tb.cpu().numpy())), "biases after the step"
    assert not np.array_equal(_bits(tw.cpu().numpy().reshape(wt.shape)), _bits(wt))
    net.close()


def _two_consumers(dilated):
    """input -> conv c1 -> (dilated | plain) 3x3 conv on c1 -> eltwise(c1, that) -> fc -> cost"""
    from bcnn_amd import capi
    C.CDLL(None).srand(SEED)
    net = capi.Net(mode=capi.MODE_TRAIN, w=7, h=7, c=3, n=2)
    net.conv(6, 3, 1, 1, act=capi.ACT_NONE, src="input", dst="c1")
    if dilated:
        node = net.dilated_conv(6, 3, 1, 2, 2, act=capi.ACT_NONE, src="c1", dst="dc")
    else:
        node = net.conv(6, 3, 1, 1, act=capi.ACT_NONE, src="c1", dst="dc")
    net.eltwise(capi.ACT_NONE, "c1", "dc", "sum")
    net.fullc(4, src="sum", dst="fc")
    net.cost("fc", "label", "cost")
    net.compile()
    _feed(net, 5)
    net.forward()
    for k in (4, 3, 2):   # cost, fc, eltwise
        net.backward_node(k)
    net.sync()
    c1, dc = net.index("c1"), net.index("dc")
    share, dy = _grad(net, c1), _grad(net, dc)   # what the eltwise node left on c1, and what reaches the node
    assert np.abs(share).max() > 0 and np.abs(dy).max() > 0
    net.backward_node(node)
    net.sync()
    x, wt = _data(net, c1), _data(net, net.node_src(node, 1))
    return net, node, x, wt, _data(net, dc), dy, share, _grad(net, c1)


def test_source_gradient_is_overwritten_like_a_convolution_nodes():
    from bcnn_amd import ops
    net, node, x, wt, y, dy, share, got = _two_consumers(True)
    _, dx, _, _ = _ops_backward(x, wt, y, dy, 3, 1, 2, 2, 1, ops.ACT["none"])
    assert np.array_equal(_bits(got), _bits(dx)), "the node's own data gradient, without the eltwise share"
    net.close()
    # the same graph with an undilated convolution node in that position follows the same rule
    net, node, x, wt, y, dy, share, got = _two_consumers(False)
    tdx = torch.full(x.shape, float("nan"), device=DEV)
    ws = torch.zeros(max(ops.conv_workspace_size(2, 6, 7, 7, 6, 3, 1, 1, 1), 1), device=DEV)
    ops.conv_backward(_t(x), _t(wt), _t(y), _t(dy), tdx, _t(np.zeros(wt.shape)), _t(np.zeros(6)), 3, 1, 1, 1,
                      ops.ACT["none"], ws)
    torch.cuda.synchronize()
    dx = tdx.cpu().numpy()
    bound = NET_TOL * float(np.abs(dx).max())
    assert float(np.abs(got - dx).max()) <= bound
    assert float(np.abs(share).max()) > 100 * bound   # the share is no rounding difference: it is gone
    net.close()


ADAM_CFG = """
[network]
input_width=7
input_height=7
input_channels=3
batch_size=2
optimizer=adam
learning_rate=0.01
momentum=0.9
decay=0.0005
beta1=0.9
beta2=0.999

[convolutional]
filters=6
size=3
stride=1
pad=2
dilation=2
function=relu
src=input
dst=dc

[connected]
output=4
src=dc
dst=fc

[cost]
src=fc
dst=out
loss=euclidean
metric=error
"""


def test_adam_from_a_config_equals_the_ops_step(tmp_path):
    from bcnn_amd import capi, ops
    cfg = tmp_path / "adam.cfg"
    cfg.write_text(ADAM_CFG)
    C.CDLL(None).srand(SEED)
    net = capi.Net.load_net(str(cfg), None, mode=capi.MODE_TRAIN)
    net.compile()
    assert net.node_type(0) == capi.LAYER_DILATED_CONV2D
    _set_biases(net, 0, 13)
    i_w, i_b = net.node_src(0, 1), net.node_src(0, 2)
    m, v = _t(np.zeros(6 * 3 * 9)), _t(np.zeros(6 * 3 * 9))
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
    path = str(tmp_path / "dc.bcnnmodel")
    assert a.save_weights(path) == 0
    blob = open(path, "rb").read()
    assert len(blob) == 16 + 4 * (6 + 6 * 3 * 9 + 4 + 4 * 6 * 7 * 7)
    in_file = np.frombuffer(blob[16:16 + 4 * (6 + 162)], F32)   # biases, then weights
    assert np.array_equal(_bits(in_file[:6]), _bits(_data(a, a.node_src(node, 2)).ravel()))
    assert np.array_equal(_bits(in_file[6:]), _bits(_data(a, a.node_src(node, 1)).ravel()))
    C.CDLL(None).srand(SEED + 1)   # other weights until the file is read
    b = capi.Net(mode=capi.MODE_PREDICT, w=7, h=7, c=3, n=2)
    node_b = b.dilated_conv(6, 3, 1, 2, 2, act=capi.ACT_RELU, src="input", dst="dc")
    b.fullc(4, src="dc", dst="fc")
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
    for name in ("dc", "fc"):
        out = _data(a, a.index(name))
        assert np.abs(out).max() > 0
        assert np.array_equal(_bits(out), _bits(_data(b, b.index(name)))), name
    a.close()
    b.close()


HEAD = """
[net]
input_width=7
input_height=7
input_channels=3
batch_size=2

"""
SECTION = """[convolutional]
filters=6
size=3
stride=1
pad=%d
%ssrc=input
dst=out
"""


def _load(tmp_path, text, mode, name="net.cfg"):
    from bcnn_amd import capi
    cfg = tmp_path / name
    cfg.write_text(text)
    C.CDLL(None).srand(SEED)
    net = capi.Net.load_net(str(cfg), None, mode=mode)
    net.compile()
    return net


def test_config_dilation_key_builds_the_node(tmp_path):
    from bcnn_amd import capi, ops
    net = _load(tmp_path, HEAD + SECTION % (2, "dilation=2\nactivation=relu\n"), capi.MODE_PREDICT)
    assert net.num_nodes == 1 and net.node_type(0) == capi.LAYER_DILATED_CONV2D
    assert net.node_activation(0) == capi.ACT_RELU
    assert net.shape(net.index("out")) == (2, 6, 7, 7)   # an undilated 3x3 with pad 2 would give 9 x 9
    _feed(net, 4, label=False)
    net.forward()
    net.sync()
    y = _ops_forward(net.data(0).copy(), _data(net, net.node_src(0, 1)), _data(net, net.node_src(0, 2)).ravel(), 6, 3, 1, 2,
                     2, 1, ops.ACT["relu"])
    assert np.array_equal(_bits(_data(net, net.index("out"))), _bits(y))
    net.close()
    # an activation that needs the layer's input: the node with no activation and the in-place node, as for the other sections
    net = _load(tmp_path, HEAD + SECTION % (2, "dilation=2\nactivation=swish\n"), capi.MODE_PREDICT)
    assert [net.node_type(k) for k in range(net.num_nodes)] == [capi.LAYER_DILATED_CONV2D, capi.LAYER_ACTIVATION]
    assert net.node_activation(0) == capi.ACT_NONE and net.node_activation(1) == capi.ACT_SWISH
    net.close()


@pytest.mark.parametrize("key", ["batchnorm", "bn", "batch_normalize"])
def test_config_batchnorm_splits_into_three_nodes(tmp_path, key):
    from bcnn_amd import capi
    net = _load(tmp_path, HEAD + SECTION % (2, "dilation=2\n%s=1\nactivation=mish\n" % key), capi.MODE_TRAIN)
    assert [net.node_type(k) for k in range(net.num_nodes)] == [capi.LAYER_DILATED_CONV2D, capi.LAYER_BATCHNORM,
                                                                 capi.LAYER_ACTIVATION]
    assert net.node_activation(0) == capi.ACT_NONE and net.node_activation(2) == capi.ACT_MISH
    inner = net.index("out_dc")
    assert inner >= 0 and net.node_dst(0) == inner and net.node_src(1, 0) == inner
    assert net.node_dst(1) == net.index("out") == net.node_src(2, 0)
    C.CDLL(None).srand(SEED)
    twin = capi.Net(mode=capi.MODE_TRAIN, w=7, h=7, c=3, n=2)
    twin.dilated_conv(6, 3, 1, 2, 2, act=capi.ACT_NONE, src="input", dst="out_dc")
    twin.batchnorm("out_dc", "out")
    twin.activation(capi.ACT_MISH, "out")
    twin.compile()
    for n in (net, twin):
        _feed(n, 6, label=False)
        n.forward()
        n.sync()
    for name in ("out_dc", "out"):
        out = _data(net, net.index(name))
        assert np.isfinite(out).all() and np.abs(out).max() > 0
        assert np.array_equal(_bits(out), _bits(_data(twin, twin.index(name)))), name
    # a Darknet .weights file interleaves the section's values: refused before anything is read (the file need not exist)
    assert net.load_weights(str(tmp_path / "no_such_file.weights")) == INVALID_MODEL
    path = str(tmp_path / "split.bcnnmodel")   # the native format round-trips
    assert net.save_weights(path) == 0 and twin.load_weights(path) == 0
    net.close()
    twin.close()


def test_config_without_dilation_builds_the_plain_convolution(tmp_path):
    from bcnn_amd import capi
    outs = []
    for name, keys in (("none.cfg", "activation=relu\n"), ("one.cfg", "dilation=1\nactivation=relu\n")):
        net = _load(tmp_path, HEAD + SECTION % (1, keys), capi.MODE_PREDICT, name)
        assert net.num_nodes == 1 and net.node_type(0) == capi.LAYER_CONV2D
        assert net.shape(net.index("out")) == (2, 6, 7, 7)
        _feed(net, 7, label=False)
        net.forward()
        net.sync()
        outs.append(_data(net, net.index("out")))
        net.close()
    assert np.abs(outs[0]).max() > 0 and np.array_equal(_bits(outs[0]), _bits(outs[1]))


DARKNET = """
[net]
batch=2
width=7
height=7
channels=3

[convolutional]
filters=6
size=3
stride=1
pad=1
dilation=2
%sactivation=linear
"""


def test_darknet_dialect_keeps_its_boolean_pad(tmp_path):
    from bcnn_amd import capi
    cfg = tmp_path / "dark.cfg"
    cfg.write_text(DARKNET % "")
    rs = np.random.RandomState(2)
    b, wt = rs.uniform(-0.5, 0.5, 6).astype(F32), rs.uniform(-0.5, 0.5, (6, 3, 3, 3)).astype(F32)
    model = tmp_path / "dark.weights"   # the extension selects the dialect; biases, then weights
    model.write_bytes(struct.pack("<iii", 0, 2, 0) + struct.pack("<Q", 0) + b.tobytes() + wt.tobytes())
    net = capi.Net.load_net(str(cfg), str(model), mode=capi.MODE_PREDICT)
    net.compile()
    assert net.num_nodes == 1 and net.node_type(0) == capi.LAYER_DILATED_CONV2D
    assert net.shape(net.node_dst(0)) == (2, 6, 5, 5)   # pad = size / 2 = 1: (7 + 2 - 2 * 2 - 1) + 1
    assert np.array_equal(_bits(_data(net, net.node_src(0, 1))), _bits(wt))
    assert np.array_equal(_bits(_data(net, net.node_src(0, 2)).ravel()), _bits(b))
    net.close()
    # with batch-norm the section is three nodes, which the .weights order does not map onto
    cfg.write_text(DARKNET % "batch_normalize=1\n")
    L = capi.lib()
    raw = C.c_void_p()
    assert L.bcnn_init_net(C.byref(raw), capi.MODE_PREDICT) == 0
    L.bcnn_set_log_context(raw, None, capi.LOG_SILENT)
    assert L.bcnn_load_net(raw, str(cfg).encode(), str(model).encode()) == INVALID_MODEL
    assert L.bcnn_get_num_nodes(raw) == 2   # dilated node + batch-norm (linear: no activation node)
    L.bcnn_end_net(C.byref(raw))


def test_refusals_leave_the_node_count_and_resize_is_refused():
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=8, h=6, c=3, n=2)
    net.conv(6, 3, 1, 1, src="input", dst="c1")
    L = net.L
    bad = [(4, 3, 1, 2, 2, 1, capi.ACT_NONE, b"no_such_tensor"),
           (0, 3, 1, 2, 2, 1, capi.ACT_NONE, b"c1"), (4, 0, 1, 2, 2, 1, capi.ACT_NONE, b"c1"),
           (4, 3, 0, 2, 2, 1, capi.ACT_NONE, b"c1"), (4, 3, 1, -1, 2, 1, capi.ACT_NONE, b"c1"),
           (4, 3, 1, 2, 0, 1, capi.ACT_NONE, b"c1"), (4, 3, 1, 2, -2, 1, capi.ACT_NONE, b"c1"),
           (4, 3, 1, 2, 2, 0, capi.ACT_NONE, b"c1"), (4, 3, 1, 2, 2, -1, capi.ACT_NONE, b"c1"),
           (4, 3, 1, 2, 2, 4, capi.ACT_NONE, b"c1"),      # 4 groups do not divide 6 input channels
           (4, 3, 1, 2, 2, 3, capi.ACT_NONE, b"c1"),      # 3 groups do not divide 4 filters
           (4, 3, 1, 0, 3, 1, capi.ACT_NONE, b"c1"),      # height 6 - 3 * 2 - 1 < 0
           (4, 3, 1, 2, 2, 1, capi.ACT_PRELU, b"c1"),
           (4, 3, 1, 2, 2, 1, capi.ACT_HARD_SWISH, b"c1"), (4, 3, 1, 2, 2, 1, capi.ACT_SWISH, b"c1"),
           (4, 3, 1, 2, 2, 1, capi.ACT_MISH, b"c1")]
    for f, k, s, p, d, g, act, src in bad:
        st = L.bcnn_add_dilated_conv_layer(net.net, f, k, s, p, d, g, capi.FILLER_XAVIER, act, src, b"dc")
        assert st == INVALID_PARAMETER, (f, k, s, p, d, g, act, src)
        assert L.bcnn_get_num_nodes(net.net) == 1
        assert net.index("dc") < 0
    node = net.dilated_conv(6, 3, 1, 2, 2, g=3, act=capi.ACT_RELU, src="c1", dst="dc")
    assert net.node_type(node) == capi.LAYER_DILATED_CONV2D and net.shape(net.node_src(node, 1)) == (6, 2, 3, 3)
    one = net.dilated_conv(6, 3, 1, 1, 1, act=capi.ACT_RELU, src="dc", dst="plain")   # dilation 1: an ordinary convolution
    assert net.node_type(one) == capi.LAYER_CONV2D
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
    fp32 = _data(net, net.index("dc"))
    assert net.set_inference_precision(capi.PRECISION_BF16) == 0
    net.data(net.index("dc"))[...] = 0
    net.upload(net.index("dc"))
    net.forward()
    net.sync()
    assert np.abs(fp32).max() > 0 and np.array_equal(_bits(_data(net, net.index("dc"))), _bits(fp32))
    net.close()


def test_trace_names_the_three_kernels():
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
    for want in ("dilated_fwd_kernel", "dilated_dx_kernel", "dilated_dw_kernel"):
        assert names.count(want) == 1, (want, names)
    net.close()
