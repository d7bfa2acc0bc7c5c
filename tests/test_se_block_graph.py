"""Squeeze-and-excitation blocks and the self-gated activations inside nets (bcnn_amd.capi).

The reference has none of this; the yardstick is a torch float64 model of the same graph with the same weights, the
batch-norm written as tests/_bn_ref.py writes it (biased one-pass variance, eps 1e-6 forward / 1e-5 backward), under the rule
of tests/test_net_parity.py: 1e-4 of the tensor maximum. The graph:
    conv 3x3 -> 16 + batch-norm (no activation); in-place swish node; global avgpool; 1x1 conv 16 -> 4 relu;
    1x1 conv 4 -> 16 hard_sigmoid; scale_channels; fc 10; softmax; cost
forward, backward, one SGD step; again with mish + logistic, and with a gate of the features' shape (Darknet's [sam]). In the
same-shape graph the gate convolutions read an identity copy of the features (pool2d avg 1 x 1 / 1): a convolution that is
the lowest-index consumer of a tensor OVERWRITES that tensor's gradient (the reference's rule), which would
drop the scale node's share.
Then: both config dialects against the builder calls bit for bit, activation=logistic, every builder refusal, PREDICT ==
TRAIN bits and the saved-input buffer of the three modes, bcnn_resize_net with and without need_realloc, the model file."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _bn_ref as BN

pytestmark = pytest.mark.gpu
NET_TOL = 1e-4  # tests/test_net_parity.py
DEV = "cuda:0"
SEED = 20260420


def _compare(tag, a, b, tol=NET_TOL):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(np.shape(a))
    assert np.isfinite(a64).all(), tag
    diff = float(np.max(np.abs(a64 - b64))) if a64.size else 0.0
    assert diff <= tol * float(np.max(np.abs(b64))) + 1e-7, "%s: max abs diff %.3g of max %.3g" % (
        tag, diff, float(np.max(np.abs(b64))))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def _num_tensors(net):
    k = 0
    while net.L.bcnn_peek_tensor(net.net, k):
        k += 1
    return k


def _graph(net, act1, gate_act, sam=False, bn=1, head=True):
    """returns the node indexes (activation node, scale node)"""
    from bcnn_amd import capi
    net.conv(16, 3, 1, 1, bn=bn, act=capi.ACT_NONE, src="input", dst="c1")
    n_act = net.activation(act1, "c1")
    if sam:
        net.pool2d("avg", 1, 1, 0, src="c1", dst="sq")   # identity copy: see the module docstring
    else:
        net.avgpool("c1", "sq")
    net.conv(4, 1, 1, 0, act=capi.ACT_RELU, src="sq", dst="s1")
    net.conv(16, 1, 1, 0, act=gate_act, src="s1", dst="g")
    n_scale = net.scale_channels("c1", "g", "se")
    if head:
        net.fullc(10, src="se", dst="fc")
        net.softmax("fc", "sm")
        net.cost("sm", "label", "cost")
    return n_act, n_scale


def _new_net(mode, shape=(4, 3, 12, 12), **kw):
    from bcnn_amd import capi
    n, c, h, w = shape
    C.CDLL(None).srand(SEED)   # the fillers draw from rand(): same weights for every net built after the same seed
    net = capi.Net(mode=mode, w=w, h=h, c=c, n=n)
    nodes = _graph(net, **kw)
    net.compile()
    return net, nodes


def _feed(net, seed, classes=10):
    rs = np.random.RandomState(seed)
    net.data(0)[...] = rs.uniform(-1, 1, net.shape(0))
    net.upload(0)
    lab = np.zeros(net.shape(1), np.float32)
    if lab.size:
        rows = lab.reshape(lab.shape[0], -1)
        rows[np.arange(rows.shape[0]), rs.randint(0, min(classes, rows.shape[1]), rows.shape[0])] = 1
        net.data(1)[...] = lab
        net.upload(1)


def _out(net, name):
    i = net.index(name)
    net.download(i, False)
    return net.data(i).copy()


class _BN64(torch.autograd.Function):
    """the fused batch-norm of the convolution node in TRAIN mode, forward and backward as tests/_bn_ref.py state them"""

    @staticmethod
    def forward(ctx, x, scales, bias):
        n, c, h, w = x.shape
        x3 = x.detach().numpy().reshape(n, c, h * w)
        out = BN.forward64(x3, np.zeros(c), np.ones(c), scales.detach().numpy(), bias.detach().numpy(), BN.MODE_TRAIN)
        ctx.saved = (x3, scales.detach().numpy(), out["saved_mean"], out["saved_var"], x.shape)
        return torch.tensor(out["pre"].reshape(x.shape), dtype=torch.float64)

    @staticmethod
    def backward(ctx, g):
        x3, scales, mean, var, shape = ctx.saved
        n, c, h, w = shape
        out = BN.backward64(g.numpy().reshape(n, c, h * w), x3, scales, mean, var, np.zeros(c), np.zeros(c))
        return (torch.tensor(out["dx"].reshape(shape), dtype=torch.float64), torch.tensor(out["dscales"], dtype=torch.float64),
                torch.tensor(out["db"], dtype=torch.float64))


ACT64 = {"swish": F.silu, "mish": F.mish, "hard_swish": F.hardswish, "hard_sigmoid": F.hardsigmoid,
         "logistic": torch.sigmoid, "relu": F.relu}


@pytest.mark.parametrize("act1,gate,sam", [("swish", "hard_sigmoid", False), ("mish", "logistic", False),
                                           ("swish", "hard_sigmoid", True), ("hard_swish", "logistic", True)])
def test_trained_block_against_torch_float64(act1, gate, sam):
    from bcnn_amd import capi, ops
    net, (n_act, n_scale) = _new_net(capi.MODE_TRAIN, act1=ops.ACT_ALL[act1], gate_act=ops.ACT_ALL[gate], sam=sam)
    lr, decay, batch = 0.01, 5e-4, 4
    net.set_sgd(lr, 0.9, decay)
    rs = np.random.RandomState(7)
    # parameters by node: conv nodes 0, 3, 4 (w, b[, run_mean, run_var, scales]), fc node 6 (w, b)
    ids = {"w1": net.node_src(0, 1), "b1": net.node_src(0, 2), "sc1": net.node_src(0, 5),
           "w2": net.node_src(3, 1), "b2": net.node_src(3, 2), "w3": net.node_src(4, 1), "b3": net.node_src(4, 2),
           "wf": net.node_src(6, 1), "bf": net.node_src(6, 2)}
    for key in ("b1", "b2", "b3", "bf"):   # biases away from 0 (and from the values bcnn_add_scalar skips)
        net.data(ids[key])[...] = rs.uniform(0.05, 0.3, net.shape(ids[key]))
        net.upload(ids[key])
    net.data(ids["sc1"])[...] = rs.uniform(0.7, 1.4, net.shape(ids["sc1"]))
    net.upload(ids["sc1"])
    _feed(net, 11)
    par = {k: torch.tensor(net.data(i).astype(np.float64), requires_grad=True) for k, i in ids.items()}
    x = torch.tensor(net.data(0).astype(np.float64))
    label = torch.tensor(net.data(1).astype(np.float64)).reshape(batch, 10)

    # ---- the float64 model ----
    kept = {}

    def keep(name, t):
        t.retain_grad()
        kept[name] = t
        return t

    raw = keep("raw", F.conv2d(x, par["w1"].reshape(16, 3, 3, 3), None, padding=1))
    c1 = keep("c1", ACT64[act1](_BN64.apply(raw, par["sc1"].reshape(-1), par["b1"].reshape(-1))))
    sq = keep("sq", c1 * 1.0 if sam else c1.mean(dim=(2, 3), keepdim=True))
    s1 = keep("s1", F.relu(keep("s1_pre", F.conv2d(sq, par["w2"].reshape(4, 16, 1, 1), par["b2"].reshape(-1)))))
    g = keep("g", ACT64[gate](keep("g_pre", F.conv2d(s1, par["w3"].reshape(16, 4, 1, 1), par["b3"].reshape(-1)))))
    se = keep("se", c1 * g)
    fc = keep("fc", se.flatten(1) @ par["wf"].reshape(10, -1).T + par["bf"].reshape(-1))
    sm = torch.softmax(fc, dim=1)
    fc.backward(gradient=(sm.detach() - label))   # cost: grad = prediction - label; softmax passes it through

    # ---- the net ----
    net.forward()
    net.backward()
    net.sync()
    for name in ("c1", "sq", "s1", "g", "se", "fc"):
        i = net.index(name)
        net.download(i)
        _compare("%s" % name, net.data(i), kept[name].detach().numpy())
        # a node's backward turns its output gradient, in place, into the gradient of what it computed before its
        # activation (and batch-norm); the in-place activation node does the same to c1's
        want = kept[{"c1": "raw", "s1": "s1_pre", "g": "g_pre"}.get(name, name)].grad
        _compare("d%s" % name, net.grad(i), want.numpy())
    _compare("sm", _out(net, "sm"), sm.detach().numpy())
    before = {}
    for key, i in ids.items():
        net.download(i)
        before[key] = net.data(i).astype(np.float64).copy()
        _compare("d%s" % key, net.grad(i), par[key].grad.numpy())
    # the saved input of the activation node is the batch-norm output, and it went through no other route
    assert net.node_state(n_act, 0)
    pre = _BN64.apply(raw.detach(), par["sc1"].detach().reshape(-1), par["b1"].detach().reshape(-1))
    _compare("saved input", _saved(net, n_act, net.shape(net.index("c1"))), pre.numpy())
    assert net.node_state(n_scale, 0) is None

    net.update()
    net.sync()
    for key, i in ids.items():
        net.download(i)
        grad = par[key].grad.numpy().reshape(before[key].shape)
        if key == "sc1":      # the scales of a fused batch-norm collect a gradient that no update applies
            want = before[key]
        elif key.startswith("w"):
            want = before[key] - (lr / batch) * (grad + decay * batch * before[key])
        else:
            want = before[key] - (lr / batch) * grad
        _compare("updated %s" % key, net.data(i), want)
    net.close()


# ---- config files ------------------------------------------------------------------------------------------------------
BCNN_CFG = """
[net]
input_width=12
input_height=12
input_channels=3
batch_size=4

[conv]
filters=16
size=3
stride=1
pad=1
bn=1
function={act1}
src=input
dst=c1

[avgpool]
src=c1
dst=sq

[conv]
filters=4
size=1
stride=1
pad=0
function=relu
src=sq
dst=s1

[conv]
filters=16
size=1
stride=1
pad=0
function={gate}
src=s1
dst=g

[scale_channels]
src=c1,g
dst=se

[connected]
output=10
src=se
dst=fc

[softmax]
src=fc
dst=sm

[cost]
src=sm
dst=cost
"""

DARKNET_CFG = """
[net]
batch=4
width=12
height=12
channels=3

[convolutional]
batch_normalize=1
filters=16
size=3
stride=1
pad=1
activation={act1}

[avgpool]

[convolutional]
filters=4
size=1
stride=1
pad=0
activation=relu

[convolutional]
filters=16
size=1
stride=1
pad=0
activation={gate}

[scale_channels]
from=-4
activation=linear

[connected]
output=10
activation=linear

[softmax]

[cost]
"""


def _darknet_weights(path, twin):
    """a Darknet model file of the twin's parameters: per convolution biases, [scales, mean, variance,] weights; fc: biases,
    weights"""
    with open(path, "wb") as fp:
        fp.write(struct.pack("<iii", 0, 2, 0) + struct.pack("<Q", 0))
        for node in range(twin.num_nodes):
            w = twin.node_src(node, 1)
            if w < 0 or not twin.tensor(w).name.decode().endswith("_w"):
                continue
            order = [2] + ([5, 3, 4] if twin.node_src(node, 5) >= 0 else []) + [1]
            for k in order:
                fp.write(np.ascontiguousarray(twin.data(twin.node_src(node, k)), np.float32).tobytes())


@pytest.mark.parametrize("dialect", ["bcnn", "darknet"])
@pytest.mark.parametrize("act1,gate", [("swish", "hard_sigmoid"), ("mish", "logistic")])
def test_config_file_builds_the_builder_calls_graph(tmp_path, dialect, act1, gate):
    from bcnn_amd import capi, ops
    twin, _ = _new_net(capi.MODE_TRAIN, act1=ops.ACT_ALL[act1], gate_act=ops.ACT_ALL[gate])
    cfg = tmp_path / "se.cfg"
    model = None
    if dialect == "bcnn":
        cfg.write_text(BCNN_CFG.format(act1=act1, gate=gate))
    else:
        cfg.write_text(DARKNET_CFG.format(act1=act1, gate=gate))
        model = str(tmp_path / "se.weights")   # the extension selects the dialect
        _darknet_weights(model, twin)
    C.CDLL(None).srand(SEED)
    net = capi.Net.load_net(str(cfg), model, mode=capi.MODE_TRAIN)
    net.compile()
    # the node list of the builder calls: the convolution section was split into the NONE layer + the in-place node
    assert net.num_nodes == twin.num_nodes == 9
    for node in range(twin.num_nodes):
        assert net.node_type(node) == twin.node_type(node), node
        assert net.node_activation(node) == twin.node_activation(node), node
        assert net.shape(net.node_dst(node)) == twin.shape(twin.node_dst(node)), node
    assert net.node_type(1) == capi.LAYER_ACTIVATION and net.node_activation(1) == ops.ACT_ALL[act1]
    assert net.node_activation(0) == capi.ACT_NONE and net.node_dst(1) == net.node_dst(0)
    assert net.node_type(5) == capi.LAYER_SCALE_CHANNELS
    assert net.node_src(5, 0) == net.node_dst(0) and net.node_src(5, 1) == net.node_dst(4)   # features, then the gate
    for n in (net, twin):
        _feed(n, 5)
        n.forward()
        n.sync()
    for node in range(twin.num_nodes - 1):
        a, b = net.node_dst(node), twin.node_dst(node)
        net.download(a, False)
        twin.download(b, False)
        assert np.array_equal(_bits(net.data(a)), _bits(twin.data(b))), "output of node %d" % node
    net.close()
    twin.close()


SAM_DARKNET = """
[net]
batch=2
width=8
height=8
channels=3

[convolutional]
filters=6
size=3
stride=1
pad=1
activation=hswish

[convolutional]
filters=6
size=1
stride=1
pad=0
activation=logistic

[sam]
from=-2
"""


def test_sam_section_and_the_logistic_name(tmp_path):
    """`activation=logistic` used to take the unknown-name branch and build a ReLU layer"""
    from bcnn_amd import capi
    cfg = tmp_path / "sam.cfg"
    cfg.write_text(SAM_DARKNET)
    C.CDLL(None).srand(SEED)
    twin = capi.Net(mode=capi.MODE_PREDICT, w=8, h=8, c=3, n=2)
    twin.conv(6, 3, 1, 1, act=capi.ACT_NONE, src="input", dst="a")
    twin.activation(capi.ACT_HARD_SWISH, "a")
    twin.conv(6, 1, 1, 0, act=capi.ACT_LOGISTIC, src="a", dst="b")
    twin.scale_channels("a", "b", "y")
    twin.compile()
    model = str(tmp_path / "sam.weights")
    _darknet_weights(model, twin)
    net = capi.Net.load_net(str(cfg), model, mode=capi.MODE_PREDICT)
    net.compile()
    assert net.num_nodes == 4
    assert [net.node_activation(k) for k in range(4)] == [capi.ACT_NONE, capi.ACT_HARD_SWISH, capi.ACT_LOGISTIC, -1]
    assert net.node_type(3) == capi.LAYER_SCALE_CHANNELS
    assert net.node_src(3, 0) == net.node_dst(0) and net.node_src(3, 1) == net.node_dst(2)
    assert net.shape(net.node_dst(3)) == (2, 6, 8, 8)
    for n in (net, twin):
        _feed(n, 9)
        n.forward()
        n.sync()
    a, b = net.node_dst(3), twin.node_dst(3)
    net.download(a, False)
    twin.download(b, False)
    assert np.array_equal(_bits(net.data(a)), _bits(twin.data(b)))
    x, gate = _out(twin, "a"), _out(twin, "b")
    assert np.array_equal(_bits(twin.data(b)), _bits(x * gate))
    assert gate.min() > 0 and gate.max() < 1   # a logistic, not a ReLU
    net.close()
    twin.close()

    bad = tmp_path / "bad.cfg"
    bad.write_text(SAM_DARKNET + "activation=relu\n")
    with pytest.raises(RuntimeError):
        capi.Net.load_net(str(bad), model, mode=capi.MODE_PREDICT)


@pytest.mark.parametrize("name,want", [("logistic", 9), ("sigmoid", 9), ("relu6", 10), ("hard_sigmoid", 11),
                                       ("hardsigmoid", 11), ("hard_swish", 12), ("hardswish", 12), ("hswish", 12),
                                       ("swish", 13), ("silu", 13), ("mish", 14), ("relu", 2), ("no_such_name", 2)])
def test_activation_names(tmp_path, name, want):
    from bcnn_amd import capi
    cfg = tmp_path / "a.cfg"
    cfg.write_text("[net]\ninput_width=4\ninput_height=4\ninput_channels=2\nbatch_size=1\n\n"
                   "[conv]\nfilters=2\nsize=1\nstride=1\npad=0\nsrc=input\ndst=c\n\n[activation]\nfunction=%s\nsrc=c\n" % name)
    net = capi.Net.load_net(str(cfg), None, mode=capi.MODE_PREDICT)
    assert net.num_nodes == 2 and net.node_activation(1) == want
    net.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_builder_refusals_add_nothing():
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=8, h=8, c=4, n=2)
    net.conv(4, 3, 1, 1, src="input", dst="a")
    net.conv(4, 3, 1, 1, src="input", dst="b")
    net.avgpool("a", "gap")
    net.conv(6, 1, 1, 0, src="gap", dst="wrong_c")       # [2,6,1,1]
    net.maxpool(2, 2, src="a", dst="half")               # [2,4,4,4]
    nodes, tensors = net.L.bcnn_get_num_nodes(net.net), _num_tensors(net)
    L, h = net.L, net.net
    tries = []
    for act in (capi.ACT_HARD_SWISH, capi.ACT_SWISH, capi.ACT_MISH):
        tries += [lambda act=act: L.bcnn_add_convolutional_layer(h, 4, 3, 1, 1, 1, 0, capi.FILLER_XAVIER, act, 0, b"a", b"x"),
                  lambda act=act: L.bcnn_add_convolutional_layer(h, 4, 3, 1, 1, 1, 1, capi.FILLER_XAVIER, act, 0, b"a", b"x"),
                  lambda act=act: L.bcnn_add_deconvolutional_layer(h, 4, 2, 2, 0, capi.FILLER_XAVIER, act, b"a", b"x"),
                  lambda act=act: L.bcnn_add_depthwise_conv_layer(h, 3, 1, 1, 0, capi.FILLER_XAVIER, act, b"a", b"x"),
                  lambda act=act: L.bcnn_add_fullc_layer(h, 5, capi.FILLER_XAVIER, act, 0, b"a", b"x"),
                  lambda act=act: L.bcnn_add_eltwise_layer(h, act, b"a", b"b", b"x")]
    tries += [lambda: L.bcnn_add_scale_channels_layer(h, b"a", b"wrong_c", b"x"),     # channels differ
              lambda: L.bcnn_add_scale_channels_layer(h, b"a", b"half", b"x"),        # neither 1 x 1 nor a's extent
              lambda: L.bcnn_add_scale_channels_layer(h, b"gap", b"a", b"x"),         # the roles swapped
              lambda: L.bcnn_add_scale_channels_layer(h, b"nobody", b"gap", b"x"),
              lambda: L.bcnn_add_scale_channels_layer(h, b"a", b"nobody", b"x")]
    for k, attempt in enumerate(tries):
        assert attempt() == 1, "attempt %d: BCNN_INVALID_PARAMETER expected" % k
        assert net.L.bcnn_get_num_nodes(net.net) == nodes and _num_tensors(net) == tensors, k
        assert net.index("x") < 0, k
    # what they refuse builds as the activation node; relu6 / hard_sigmoid build fused
    net.conv(4, 3, 1, 1, act=capi.ACT_RELU6, src="a", dst="r6")
    net.fullc(5, act=capi.ACT_HARD_SIGMOID, src="r6", dst="hs")
    net.activation(capi.ACT_MISH, "a")
    net.scale_channels("a", "gap", "ok1")
    net.scale_channels("a", "b", "ok2")
    assert net.L.bcnn_get_num_nodes(net.net) == nodes + 5
    net.close()


# ---- modes, resize, model files -------------------------------------------------------------------------------------------
def _saved(net, node, shape):
    from bcnn_amd import _lib
    got = torch.empty(shape, dtype=torch.float32, device=DEV)
    _lib.load().bcnn_hip_memcpy_d2d(got.data_ptr(), net.node_state(node, 0), got.numel() * 4)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("sam", [False, True])
def test_predict_forward_has_train_bits_and_keeps_nothing(sam):
    from bcnn_amd import capi
    kw = dict(act1=capi.ACT_SWISH, gate_act=capi.ACT_HARD_SIGMOID, sam=sam, bn=0)   # batch statistics differ by mode
    train, (n_act, _) = _new_net(capi.MODE_TRAIN, **kw)
    pred, _ = _new_net(capi.MODE_PREDICT, **kw)
    assert train.node_state(n_act, 0) and pred.node_state(n_act, 0) is None
    for n in (train, pred):
        _feed(n, 21)
        n.forward()
        n.sync()
    for name in ("c1", "g", "se", "sm"):
        assert np.array_equal(_bits(_out(train, name)), _bits(_out(pred, name))), name
    # a VALID forward stores nothing: the buffer still holds the TRAIN forward's input
    kept = _saved(train, n_act, train.shape(train.index("c1")))
    assert np.abs(kept).max() > 0
    assert train.set_mode(capi.MODE_VALID) == 0
    _feed(train, 22)
    train.forward()
    train.sync()
    assert np.array_equal(_bits(_saved(train, n_act, kept.shape)), _bits(kept))
    train.close()
    pred.close()


def test_resize_follows_the_saved_input_capacity():
    _resize_follows_the_capacity(bn=0)


def test_resize_follows_the_capacity_behind_a_fused_batchnorm():
    _resize_follows_the_capacity(bn=1)


def _resize_follows_the_capacity(bn):
    from bcnn_amd import capi
    # no fc (its weights are tied to the extent) and no global avgpool (bcnn_resize_net gives its output the source's extent,
    # as the reference does); bn=1: the fused batch-norm's workspace sits in front of the saved input and follows the same rule
    kw = dict(act1=capi.ACT_MISH, gate_act=capi.ACT_LOGISTIC, head=False, bn=bn, sam=True)
    net, (n_act, _) = _new_net(capi.MODE_TRAIN, shape=(2, 3, 12, 12), **kw)
    shapes = [net.shape(k) for k in range(_num_tensors(net))]
    # 1 x 16 x 20 x 20 > 2 x 16 x 12 x 12: refused without need_realloc, and nothing has changed
    assert net.resize(20, 20, 3, need_realloc=False) == 1
    assert [net.shape(k) for k in range(_num_tensors(net))] == shapes
    _feed(net, 1)
    net.forward()
    net.sync()
    again, _ = _new_net(capi.MODE_TRAIN, shape=(2, 3, 12, 12), **kw)
    _feed(again, 1)
    again.forward()
    again.sync()
    assert np.array_equal(_bits(_out(net, "se")), _bits(_out(again, "se")))
    again.close()
    # a smaller shape fits the buffer as it is
    assert net.resize(8, 8, 3, need_realloc=False) == 0 and net.shape(net.index("se")) == (1, 16, 8, 8)
    # with need_realloc the buffer grows; the forward matches a net built at that shape
    assert net.resize(20, 20, 3, need_realloc=True) == 0
    assert net.shape(net.index("se")) == (1, 16, 20, 20) and net.shape(net.index("g")) == (1, 16, 20, 20)
    big, _ = _new_net(capi.MODE_TRAIN, shape=(1, 3, 20, 20), **kw)
    for n in (net, big):
        _feed(n, 2)
        n.forward()
        n.sync()
    assert np.array_equal(_bits(_out(net, "se")), _bits(_out(big, "se")))
    assert np.array_equal(_bits(_saved(net, n_act, (1, 16, 20, 20))), _bits(_saved(big, n_act, (1, 16, 20, 20))))
    net.backward()   # the backward runs on the grown buffer
    net.sync()
    net.close()
    big.close()


def test_model_file_round_trip(tmp_path):
    from bcnn_amd import capi
    kw = dict(act1=capi.ACT_HARD_SWISH, gate_act=capi.ACT_HARD_SIGMOID)
    a, _ = _new_net(capi.MODE_TRAIN, **kw)
    rs = np.random.RandomState(3)
    params = [a.node_src(node, k) for node in (0, 3, 4, 6) for k in (1, 2)]
    for i in params:
        a.data(i)[...] = rs.uniform(-0.5, 0.5, a.shape(i))
        a.upload(i)
    path = str(tmp_path / "se.bcnnmodel")
    assert a.save_weights(path) == 0
    # the file holds the four weighted nodes and nothing for the activation and scale nodes
    floats = sum(int(np.prod(a.shape(i))) for i in params) + 3 * 16
    assert len(open(path, "rb").read()) == 16 + 4 * floats
    b, _ = _new_net(capi.MODE_TRAIN, **kw)
    assert b.load_weights(path) == 0
    for n in (a, b):
        _feed(n, 4)
        n.forward()
        n.sync()
    assert np.array_equal(_bits(_out(a, "sm")), _bits(_out(b, "sm")))
    a.close()
    b.close()
