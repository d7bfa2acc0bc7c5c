"""The pool2d node inside nets.

Against the unmodified reference (oracle/_ref/libbcnn_ref.so), which has no such node, through two identities:
  1. on even extents pool2d(max, 2, 2, 0, floor) is the reference's maxpool(2, 2, SAME): conv -> pool -> conv+BN -> pool ->
     fc -> softmax -> cost, N = 4 at 16 x 16, two SGD steps; every tensor, every gradient (1e-4 of the tensor maximum, the
     rule of tests/test_net_parity.py), the winners bit for bit, and the model file;
  2. pool2d(avg, size = H = W, 1, 0) is the reference's global avgpool: conv -> pool -> fc at 7 x 7, same rule.
Then what the reference cannot say: a pool whose source gradient has a second writer (add form == overwrite form + the
other writer, bit for bit), the [pool] / [local_avgpool] sections in both config dialects against the builder calls and
against torch, bcnn_resize_net over both kinds, and PREDICT == TRAIN forward bit for bit."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_bind as rb

pytestmark = pytest.mark.gpu
NET_TOL = 1e-4  # tests/test_net_parity.py
DEV = "cuda:0"


def _need_ref():
    if not rb.available():
        pytest.skip("oracle/_ref/libbcnn_ref.so not present")


def _compare(tag, a, b, tol=NET_TOL):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a64.shape == b64.shape, (tag, a64.shape, b64.shape)
    assert np.isfinite(a64).all(), tag
    diff = float(np.max(np.abs(a64 - b64))) if a64.size else 0.0
    assert diff <= tol * float(np.max(np.abs(b64))) + 1e-7, "%s: max abs diff %.3g" % (tag, diff)


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


def _node_indexes(net, node, shape):
    from bcnn_amd import _lib
    got = torch.empty(shape, dtype=torch.int32, device=DEV)
    _lib.load().bcnn_hip_memcpy_d2d(got.data_ptr(), net.node_state(node, 0), got.numel() * 4)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _train_parity(build_ref, build_hip, shp, classes, tmp_path, pool_nodes):
    """the same graph on both libraries but for the pooling builder; two SGD steps, everything compared"""
    from bcnn_amd import capi
    seed = 20260301
    C.CDLL(None).srand(seed)
    ref = rb.RefNet(mode=rb.MODE_TRAIN, **shp)
    ref.L.ref_set_threads(ref.net, 4)
    build_ref(ref)
    C.CDLL(None).srand(seed)
    hip = capi.Net(mode=capi.MODE_TRAIN, **shp)
    build_hip(hip)
    ref.compile()
    hip.compile()
    nt = ref.L.ref_num_tensors(ref.net)
    names = [ref.L.ref_tensor_name(ref.net, i).decode() for i in range(nt)]
    ref.L.bcnn_set_sgd_optimizer(ref.net, 0.01, 0.9)
    ref.L.bcnn_set_weight_regularizer(ref.net, 5e-4)
    hip.set_sgd(0.01, 0.9, 5e-4)
    rs = np.random.RandomState(11)
    for i, name in enumerate(names):
        assert hip.shape(i) == ref.shape(i), (name, hip.shape(i), ref.shape(i))
        if name.endswith("_b"):
            ref.data(i)[...] = rs.uniform(-0.2, 0.2, ref.shape(i))
        if i == 0:
            ref.data(i)[...] = rs.uniform(-1, 1, ref.shape(i))
        elif i == 1:
            lab = np.zeros(ref.shape(i), np.float32)
            lab.reshape(lab.shape[0], -1)[np.arange(lab.shape[0]), rs.randint(0, classes, lab.shape[0])] = 1
            ref.data(i)[...] = lab
        if ref.tensor(i).data:
            hip.data(i)[...] = ref.data(i)
            hip.upload(i)
    _trace(True)
    for it in range(2):
        ref.forward()
        hip.forward()
        ref.backward()
        hip.backward()
        for i, name in enumerate(names):
            if not ref.tensor(i).data:
                continue
            hip.download(i)
            _compare("it%d %s" % (it, name), hip.data(i), ref.data(i))
            if ref.grad(i) is not None and i > 1:
                _compare("it%d d%s" % (it, name), hip.grad(i), ref.grad(i))
        for node in pool_nodes:  # max pooling: the winners, bit for bit
            want = ref.maxpool_indexes(node)
            assert np.array_equal(_node_indexes(hip, node, want.shape), want), "winners differ in node %d" % node
        ref.L.bcnn_update(ref.net)
        hip.update()
    ran = _trace(False)
    outputs = {ref.node_dst(k) for k in range(ref.L.ref_num_nodes(ref.net))}
    for i, name in enumerate(names):  # parameters and batch-norm running statistics after the second update
        if i > 1 and i not in outputs and ref.tensor(i).data:
            hip.download(i)
            _compare("final %s" % name, hip.data(i), ref.data(i))
            ref.data(i)[...] = hip.data(i)
    pr, ph = str(tmp_path / "ref.bcnnmodel"), str(tmp_path / "hip.bcnnmodel")
    assert ref.save_weights(pr) == 0 and hip.save_weights(ph) == 0
    assert open(pr, "rb").read() == open(ph, "rb").read()   # the pooling node adds nothing to the file
    assert hip.load_weights(ph) == 0
    ref.close()
    hip.close()
    return ran


def test_max_2x2_is_the_references_same_maxpool(tmp_path):
    _need_ref()

    def graph(net, pool):
        net.conv(6, 3, 1, 1, act=rb.ACT_RELU, src="input", dst="c1")
        pool(net, "c1", "p1")
        net.conv(8, 3, 1, 1, bn=1, act=rb.ACT_RELU, src="p1", dst="c2")
        pool(net, "c2", "p2")
        net.fullc(5, src="p2", dst="f1")
        net.softmax("f1", "sm")
        net.cost("sm", "label", "cost")

    ran = _train_parity(lambda n: graph(n, lambda net, s, d: net.maxpool(2, 2, rb.PADDING_SAME, src=s, dst=d)),
                        lambda n: graph(n, lambda net, s, d: net.pool2d("max", 2, 2, 0, src=s, dst=d)),
                        dict(w=16, h=16, c=3, n=4), 5, tmp_path, pool_nodes=(1, 3))
    # the new node ran its own kernels: no kernel of the existing pooling nodes, no conv / batch-norm pooling fusion
    assert "pool2d_fwd_s2x4_kernel<max,2>:v4" in ran, ran
    assert "pool2d_bwd_vec4_kernel<max,2,2,0>:overwrite" in ran, ran   # each pool is its source gradient's only writer
    assert not [k for k in ran if k.startswith("maxpool_")], ran


def test_avg_over_the_plane_is_the_references_global_avgpool(tmp_path):
    _need_ref()

    def graph(net, pool):
        net.conv(6, 3, 1, 1, act=rb.ACT_RELU, src="input", dst="c1")
        pool(net, "c1", "a1")
        net.fullc(5, src="a1", dst="f1")
        net.softmax("f1", "sm")
        net.cost("sm", "label", "cost")

    ran = _train_parity(lambda n: graph(n, lambda net, s, d: net.avgpool(src=s, dst=d)),
                        lambda n: graph(n, lambda net, s, d: net.pool2d("avg", 7, 1, 0, src=s, dst=d)),
                        dict(w=7, h=7, c=3, n=4), 5, tmp_path, pool_nodes=())
    assert "pool2d_fwd_kernel<avg>" in ran and "pool2d_bwd_kernel<avg>:overwrite" in ran, ran
    assert not [k for k in ran if k.startswith("avgpool_")], ran


def test_shared_source_gradient_uses_the_add_form():
    """c1 feeds a pool2d node AND an eltwise node: the pool is not the only writer of c1's gradient, so the executor
    zero-fills it and the pool adds. With 2 x 2 / s2 windows every element gets at most one pooled gradient, so
    (other + g) == (0 + g) + other bit for bit whatever the values."""
    from bcnn_amd import capi, ops
    net = capi.Net(mode=capi.MODE_TRAIN, w=16, h=16, c=3, n=4)
    net.conv(6, 3, 1, 1, act=capi.ACT_RELU, src="input", dst="c1")
    net.conv(6, 3, 1, 1, act=capi.ACT_RELU, src="input", dst="cx")
    n_pool = net.pool2d("max", 2, 2, 0, src="c1", dst="p")
    n_elt = net.eltwise(capi.ACT_NONE, "c1", "cx", "e")
    net.pool2d("avg", 2, 2, 0, src="e", dst="pe")
    net.eltwise(capi.ACT_NONE, "p", "pe", "m")
    net.fullc(5, src="m", dst="f1")
    net.softmax("f1", "sm")
    net.cost("sm", "label", "cost")
    net.compile()
    rs = np.random.RandomState(5)
    net.data(0)[...] = rs.uniform(-1, 1, net.shape(0))
    net.upload(0)
    lab = np.zeros(net.shape(1), np.float32)
    lab.reshape(4, -1)[np.arange(4), rs.randint(0, 5, 4)] = 1
    net.data(1)[...] = lab
    net.upload(1)
    # the executor's choice, from the trace of a whole pass
    _trace(True)
    net.forward()
    net.backward()
    net.sync()
    ran = _trace(False)
    assert "pool2d_bwd_vec4_kernel<max,2,2,0>" in ran, ran              # c1's gradient has two writers: add
    assert "pool2d_bwd_vec4_kernel<max,2,2,0>:overwrite" not in ran, ran
    assert "pool2d_bwd_vec4_kernel<avg,2,2,0>:overwrite" in ran, ran    # e's gradient has one
    # the values, node by node on gradients of our own
    c1, p, e = net.index("c1"), net.index("p"), net.index("e")
    for i in (c1, p, e):
        net.download(i)
    dy_p = rs.uniform(-1, 1, net.shape(p)).astype(np.float32)
    dy_e = rs.uniform(-1, 1, net.shape(e)).astype(np.float32)
    net.grad(p)[...] = dy_p
    net.grad(e)[...] = dy_e
    net.upload(p, with_grad=True)
    net.upload(e, with_grad=True)

    def c1_grad_after(nodes):
        net.grad(c1)[...] = 0
        net.upload(c1, with_grad=True)
        for node in nodes:
            net.backward_node(node)
        net.download(c1)
        return net.grad(c1).copy()

    other = c1_grad_after([n_elt])
    assert np.abs(other).max() > 0
    total = c1_grad_after([n_elt, n_pool])   # the executor's order: the later node writes first
    idx = torch.tensor(_node_indexes(net, n_pool, net.shape(p)), device=DEV)
    over = torch.full(net.shape(c1), 7.0, device=DEV)
    ops.pool2d_backward(torch.tensor(dy_p, device=DEV), idx, over, "max", 2, 2, 0, overwrite=True)
    want = over.cpu().numpy() + other
    assert np.array_equal(total.view(np.int32), want.view(np.int32))
    net.close()


# ---- config files ------------------------------------------------------------------------------------------------------
def _avg_bound(x, k, s, p, ceil, cip):
    kw = dict(kernel_size=k, stride=s, padding=p, ceil_mode=bool(ceil), count_include_pad=bool(cip))
    x64 = torch.tensor(x, dtype=torch.float64)
    return F.avg_pool2d(x64, **kw).numpy(), 1.01 * k * k * 2.0 ** -24 * F.avg_pool2d(x64.abs(), **kw).numpy()


def _check_nodes_against_torch(net, specs):
    """every pool2d node's output against torch on that node's downloaded source: max bit for bit, average within the
    operator bound of tests/test_pool2d.py"""
    for node, (kind, k, s, p, ceil, cip) in enumerate(specs):
        src, dst = net.node_src(node, 0), net.node_dst(node)
        net.download(src, False)
        net.download(dst, False)
        x, y = net.data(src).copy(), net.data(dst).copy()
        if kind == "max":
            want = F.max_pool2d(torch.tensor(x), k, s, p, ceil_mode=bool(ceil)).numpy()
            assert y.shape == want.shape and np.array_equal(y.view(np.int32), want.view(np.int32)), node
        else:
            want, bound = _avg_bound(x, k, s, p, ceil, cip)
            assert y.shape == want.shape and (np.abs(y - want) <= bound).all(), node


def _feed_and_forward(net, seed):
    net.data(0)[...] = np.random.RandomState(seed).standard_normal(net.shape(0))
    net.upload(0)
    net.forward()
    net.sync()


BCNN_CFG = """
[net]
input_width=24
input_height=20
input_channels=3
batch_size=2

[pool]
type=max
size=3
stride=2
pad=1
src=input
dst=p1

[pool2d]
type=avg
size=3
stride=1
pad=1
count_include_pad=0
src=p1
dst=p2

[pool]
src=p2
dst=p3

[local_avgpool]
size=2
stride=1
src=p3
dst=p4

[pool]
type=avg
size=3
stride=2
ceil_mode=1
src=p4
dst=p5
"""
BCNN_SPECS = [("max", 3, 2, 1, 0, 1), ("avg", 3, 1, 1, 0, 0), ("max", 2, 2, 0, 0, 1), ("avg", 2, 1, 0, 0, 1),
              ("avg", 3, 2, 0, 1, 1)]
BCNN_SHAPES = [(2, 3, 10, 12), (2, 3, 10, 12), (2, 3, 5, 6), (2, 3, 4, 5), (2, 3, 2, 2)]

DARKNET_CFG = """
[net]
batch=2
width=24
height=20
channels=3

[pool]
type=max
size=3
stride=2
pad=1

[local_avgpool]
size=3
stride=1
pad=1

[pool]
type=avg
size=2
stride=2
"""
DARKNET_SPECS = [("max", 3, 2, 1, 0, 1), ("avg", 3, 1, 1, 0, 1), ("avg", 2, 2, 0, 0, 1)]
DARKNET_SHAPES = [(2, 3, 10, 12), (2, 3, 10, 12), (2, 3, 5, 6)]


def _built_like(specs, mode):
    from bcnn_amd import capi
    net = capi.Net(mode=mode, w=24, h=20, c=3, n=2)
    src = "input"
    for i, (kind, k, s, p, ceil, cip) in enumerate(specs):
        net.pool2d(kind, k, s, p, bool(ceil), bool(cip), src=src, dst="t%d" % i)
        src = "t%d" % i
    net.compile()
    return net


@pytest.mark.parametrize("dialect", ["bcnn", "darknet"])
def test_pool_sections_of_a_config_file(tmp_path, dialect):
    from bcnn_amd import capi
    if dialect == "bcnn":
        text, specs, shapes, model, mode = BCNN_CFG, BCNN_SPECS, BCNN_SHAPES, None, capi.MODE_TRAIN
    else:
        text, specs, shapes, mode = DARKNET_CFG, DARKNET_SPECS, DARKNET_SHAPES, capi.MODE_PREDICT
        model = str(tmp_path / "pools.weights")   # the extension selects the dialect; no layer of this net has weights
        with open(model, "wb") as fp:
            fp.write(struct.pack("<iii", 0, 2, 0) + struct.pack("<Q", 0))
    cfg = tmp_path / "pools.cfg"
    cfg.write_text(text)
    net = capi.Net.load_net(str(cfg), model, mode=mode)
    net.compile()
    twin = _built_like(specs, mode)
    assert net.num_nodes == twin.num_nodes == len(specs)
    for node, shape in enumerate(shapes):
        assert net.shape(net.node_dst(node)) == twin.shape(twin.node_dst(node)) == shape, node
    _feed_and_forward(net, 3)
    _feed_and_forward(twin, 3)
    _check_nodes_against_torch(net, specs)
    last = len(specs) - 1
    net.download(net.node_dst(last), False)
    twin.download(twin.node_dst(last), False)
    assert np.array_equal(net.data(net.node_dst(last)).view(np.int32), twin.data(twin.node_dst(last)).view(np.int32))
    net.close()
    twin.close()


def test_resize_shrinks_and_grows_both_kinds():
    """bcnn_resize_net re-shapes to batch 1; 8 x 12 shrinks below the built size, 20 x 28 grows past the index buffer's
    capacity, 16 x 16 returns inside it"""
    from bcnn_amd import capi
    specs = [("max", 3, 2, 1, 0, 1), ("avg", 3, 1, 1, 0, 0), ("max", 2, 2, 0, 1, 1)]
    net = capi.Net(mode=capi.MODE_TRAIN, w=16, h=16, c=3, n=2)
    src = "input"
    for i, (kind, k, s, p, ceil, cip) in enumerate(specs):
        net.pool2d(kind, k, s, p, bool(ceil), bool(cip), src=src, dst="t%d" % i)
        src = "t%d" % i
    net.compile()
    _feed_and_forward(net, 1)
    _check_nodes_against_torch(net, specs)
    for w, h in ((12, 8), (28, 20), (16, 16), (30, 22)):
        assert net.resize(w, h, 3) == 0
        assert net.shape(0) == (1, 3, h, w)
        x = torch.zeros(1, 3, h, w)
        for node, (kind, k, s, p, ceil, cip) in enumerate(specs):
            x = (F.max_pool2d(x, k, s, p, ceil_mode=bool(ceil)) if kind == "max"
                 else F.avg_pool2d(x, k, s, p, ceil_mode=bool(ceil)))
            assert net.shape(net.node_dst(node)) == tuple(x.shape), (w, h, node)
        _feed_and_forward(net, w)
        _check_nodes_against_torch(net, specs)
        if (w, h) != (12, 8):   # the winners of the grown buffer are whole: a backward pass through them is in bounds
            net.backward()
            net.sync()
    # a 1 x 1 input leaves the last node (2 x 2 window, no padding) a 1 x 1 source: refused, BCNN_INVALID_PARAMETER
    shapes = [net.shape(0)] + [net.shape(net.node_dst(node)) for node in range(len(specs))]
    assert net.resize(1, 1, 3) == 1
    # found at the last node, with need_realloc: the nodes in front of it were not resized on the way there
    assert [net.shape(0)] + [net.shape(net.node_dst(node)) for node in range(len(specs))] == shapes
    assert net.L.bcnn_get_batch_size(net.net) == 1
    _feed_and_forward(net, 5)
    _check_nodes_against_torch(net, specs)
    net.close()


def test_predict_forward_is_the_train_forward():
    from bcnn_amd import capi
    specs = [("max", 3, 2, 1, 0, 1), ("max", 5, 1, 2, 0, 1), ("avg", 3, 2, 1, 1, 0)]
    outs = {}
    for mode in (capi.MODE_TRAIN, capi.MODE_PREDICT):
        net = _built_like(specs, mode)
        _trace(True)
        _feed_and_forward(net, 9)
        ran = _trace(False)
        assert ran == ["pool2d_fwd_s2x4_kernel<max,3>:v4", "pool2d_fwd_kernel<max>", "pool2d_fwd_s2x4_kernel<avg,3>"], ran
        for node in range(len(specs)):
            assert (net.node_state(node, 0) is not None) == (mode == capi.MODE_TRAIN and specs[node][0] == "max")
        last = net.node_dst(len(specs) - 1)
        net.download(last, False)
        outs[mode] = net.data(last).copy()
        if mode == capi.MODE_TRAIN:   # the same net switched to PREDICT: its forward stores no winners, same values
            assert net.set_mode(capi.MODE_PREDICT) == 0
            _feed_and_forward(net, 9)
            net.download(last, False)
            assert np.array_equal(net.data(last).view(np.int32), outs[mode].view(np.int32))
        net.close()
    assert np.array_equal(outs[capi.MODE_TRAIN].view(np.int32), outs[capi.MODE_PREDICT].view(np.int32))
