"""bcnn_resize_net (reference src/bcnn_net.c:287-335): a fully convolutional PREDICT net built for one input extent and
resized to a smaller one has to give what a net built for that extent gives, with the same parameters -- shapes by the
reference's rules (batch 1; convolution and max-pooling outputs from their hyper-parameters, everything else a copy of its
source's shape), tensors re-allocated on host and device."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _build(capi, w, h, n):
    ctypes.CDLL(None).srand(11)
    net = capi.Net(mode=capi.MODE_PREDICT, w=w, h=h, c=3, n=n)
    net.conv(16, 3, 1, 1, 1, 1, capi.ACT_RELU, "input", "c1")
    net.maxpool(2, 2, capi.PADDING_SAME, "c1", "p1")
    net.conv(32, 3, 2, 1, 1, 0, capi.ACT_LRELU, "p1", "c2")
    net.activation(capi.ACT_RELU, "c2")
    net.conv(8, 1, 1, 0, 1, 0, capi.ACT_NONE, "c2", "c3")
    net.compile()
    return net


def test_resized_net_equals_a_net_built_for_that_extent():
    from bcnn_amd import capi
    big = _build(capi, 48, 40, 2)
    small = _build(capi, 32, 24, 1)          # same srand -> same Xavier draws -> same parameters
    assert big.resize(32, 24, 3, True) == 0
    names = ("input", "c1", "p1", "c2", "c3")
    for name in names:
        assert big.shape(big.index(name)) == small.shape(small.index(name)), name
    assert big.shape(big.index("input")) == (1, 3, 24, 32)
    assert big.shape(big.index("c2")) == (1, 32, 6, 8)
    x = np.random.RandomState(3).uniform(-1, 1, (1, 3, 24, 32)).astype(np.float32)
    for net in (big, small):
        net.data(0)[...] = x
        net.upload(0)
        net.forward()
    for name in ("c1", "p1", "c2", "c3"):
        a, b = big.index(name), small.index(name)
        big.download(a, False)
        small.download(b, False)
        assert np.array_equal(big.data(a), small.data(b)), name
    big.close()
    small.close()


def test_resize_rejects_nonsense():
    from bcnn_amd import capi
    net = _build(capi, 16, 16, 1)
    assert net.resize(0, 16, 3) != 0
    net.close()


def test_net_resized_to_a_larger_extent_equals_a_net_built_for_it():
    """the usual detection use of bcnn_resize_net: a batch-1 fully convolutional net grows (16 x 16 -> 48 x 40). The
    pooling node's index buffer and the batch-norm workspaces follow the new shapes (the reference leaves them at their old
    size and overruns them); results equal those of a net built for the larger extent."""
    from bcnn_amd import capi
    small = _build(capi, 16, 16, 1)
    big = _build(capi, 48, 40, 1)
    assert small.resize(48, 40, 3, True) == 0
    for name in ("input", "c1", "p1", "c2", "c3"):
        assert small.shape(small.index(name)) == big.shape(big.index(name)), name
    x = np.random.RandomState(5).uniform(-1, 1, (1, 3, 40, 48)).astype(np.float32)
    for net in (small, big):
        net.data(0)[...] = x
        net.upload(0)
        net.forward()
    for name in ("c1", "p1", "c2", "c3"):
        a, b = small.index(name), big.index(name)
        small.download(a, False)
        big.download(b, False)
        assert np.array_equal(small.data(a), big.data(b)), name
    # without need_realloc a shape that outgrew the layers' private buffers is refused, not run past them
    tiny = _build(capi, 16, 16, 1)
    assert tiny.resize(64, 64, 3, False) != 0
    for net in (small, big, tiny):
        net.close()


# ---- plan, then commit: a refusal changes nothing; private buffers follow by capacity -----------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _num_tensors(net):
    k = 0
    while net.L.bcnn_peek_tensor(net.net, k):
        k += 1
    return k


def _state(net):
    return [net.shape(k) for k in range(_num_tensors(net))], net.L.bcnn_get_batch_size(net.net)


def _six_nodes(net, capi):
    """one node of every kind that keeps a private buffer: conv + fused batch-norm, maxpool, stand-alone batch-norm, pool2d
    max, mish activation node. The conv / maxpool pair meets the conditions of bcnn_link_conv_maxpool (stride 2, size 3,
    width a multiple of 4, relu)"""
    net.conv(8, 3, 1, 1, bn=1, act=capi.ACT_RELU, src="input", dst="c1")
    net.maxpool(3, 2, capi.PADDING_SAME, "c1", "p1")
    net.conv(12, 3, 1, 1, src="p1", dst="c2")
    net.batchnorm("c2", "b2")
    net.pool2d("max", 3, 1, 1, src="b2", dst="q")
    net.activation(capi.ACT_MISH, "q")
    return ("c1", "p1", "c2", "b2", "q")


def _one_kind(kind):
    """a plain convolution (no buffer of its own) and behind it one buffer-owning node, the only one that can refuse"""
    def graph(net, capi):
        net.conv(8, 3, 1, 1, src="input", dst="c0")
        if kind == "conv_bn":
            net.conv(8, 3, 1, 1, bn=1, act=capi.ACT_RELU, src="c0", dst="y")
        elif kind == "maxpool":
            net.maxpool(2, 2, capi.PADDING_SAME, "c0", "y")
        elif kind == "batchnorm":
            # a second reader of c0: otherwise the node keeps no copy of its input (bcnn_link_depthwise_batchnorm) and has
            # no buffer to refuse with
            net.batchnorm("c0", "y")
            net.pool2d("avg", 1, 1, 0, src="c0", dst="side")
        elif kind == "pool2d":
            net.pool2d("max", 3, 2, 1, src="c0", dst="y")
        else:
            net.activation(capi.ACT_MISH, "c0")
            return ("c0",)
        return ("c0", "y")
    return graph


def _train_net(capi, graph, w, h, n, compile_now=True):
    ctypes.CDLL(None).srand(11)
    net = capi.Net(mode=capi.MODE_TRAIN, w=w, h=h, c=3, n=n)
    names = graph(net, capi)
    if compile_now:
        net.compile()
    return net, names


def _forward(net, seed, names):
    net.data(0)[...] = np.random.RandomState(seed).uniform(-1, 1, net.shape(0))
    net.upload(0)
    net.forward()
    net.sync()
    out = {}
    for name in names:
        i = net.index(name)
        net.download(i, False)
        out[name] = net.data(i).copy()
    return out


def _backward(net, seed, last, wanted):
    """a backward pass from a random gradient of tensor `last`; returns the gradient of tensor `wanted`"""
    i = net.index(last)
    net.download(i)
    net.grad(i)[...] = np.random.RandomState(seed).uniform(-1, 1, net.shape(i))
    net.upload(i, True)
    net.backward()
    net.sync()
    j = net.index(wanted)
    net.download(j)
    return net.grad(j).copy()


@pytest.mark.parametrize("kind", ["six_nodes", "conv_bn", "maxpool", "batchnorm", "pool2d", "activation"])
def test_a_refusal_changes_nothing_whichever_node_refuses(kind):
    from bcnn_amd import capi
    graph = _six_nodes if kind == "six_nodes" else _one_kind(kind)
    net, names = _train_net(capi, graph, 12, 12, 2)
    before = _state(net)
    assert net.resize(24, 24, 3, need_realloc=False) == 1   # 1 x 24 x 24 is past every capacity of a 2 x 12 x 12 build
    assert _state(net) == before
    fresh, _ = _train_net(capi, graph, 12, 12, 2)
    assert _state(fresh) == before
    got, want = _forward(net, 1, names), _forward(fresh, 1, names)
    for name in names:
        assert np.array_equal(_bits(got[name]), _bits(want[name])), name
    net.close()
    fresh.close()


def test_private_buffers_follow_their_capacity_not_the_last_shape():
    from bcnn_amd import capi
    net, names = _train_net(capi, _six_nodes, 16, 16, 2)

    def same_as_built(extent, seed):
        built, _ = _train_net(capi, _six_nodes, extent, extent, 1)
        assert _state(net) == _state(built)
        got, want = _forward(net, seed, names), _forward(built, seed, names)
        for name in names:
            assert np.array_equal(_bits(got[name]), _bits(want[name])), (extent, name)
        dg, dw = _backward(net, seed + 1, "q", "c1"), _backward(built, seed + 1, "q", "c1")
        assert np.array_equal(_bits(dg), _bits(dw)), extent
        built.close()

    assert net.resize(8, 8, 3, False) == 0
    assert net.resize(16, 16, 3, False) == 0    # one image of 16 x 16 is inside the capacity of the batch-2 build
    same_as_built(16, 2)
    assert net.resize(24, 24, 3, True) == 0     # the capacity follows the grow ...
    assert net.resize(8, 8, 3, False) == 0
    assert net.resize(24, 24, 3, False) == 0    # ... not the build
    same_as_built(24, 4)
    before = _state(net)
    assert net.resize(32, 32, 3, False) == 1
    assert _state(net) == before
    net.close()


def _trace(fn):
    from bcnn_amd import _lib
    L = _lib.load()
    L.bcnn_hip_trace_enable(1)  # clears the log
    fn()
    n = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return set(buf.value.decode().split())


def _conv_maxpool_pair(net, capi):
    net.conv(8, 3, 1, 1, src="input", dst="c0")
    net.conv(8, 3, 1, 1, bn=1, act=capi.ACT_RELU, src="c0", dst="c1")
    net.maxpool(3, 2, capi.PADDING_SAME, "c1", "p1")
    return ("c0", "p1")


def _batchnorm_conv_pair(net, capi):
    """[depthwise] -> [batchnorm] -> [conv 1x1 / 1, one group]: the chain bcnn_link_batchnorm_conv links"""
    net.conv(8, 3, 1, 1, src="input", dst="c0")
    net.depthwise(3, 1, 1, capi.ACT_RELU, "c0", "d1")
    net.batchnorm("d1", "b1")
    net.conv(12, 1, 1, 0, bn=1, act=capi.ACT_RELU, src="b1", dst="c2")
    return ("c0", "c2")


@pytest.mark.parametrize("pair", ["conv_maxpool", "batchnorm_conv"])
def test_buffers_a_link_pass_makes_at_a_shrunk_shape_hold_the_grown_one(pair):
    """the first compile sees the net shrunk below its build: what the link passes allocate then must still hold the shape
    the net may grow back to without need_realloc"""
    from bcnn_amd import capi
    graph = _conv_maxpool_pair if pair == "conv_maxpool" else _batchnorm_conv_pair
    net, (first, last) = _train_net(capi, graph, 16, 16, 2, compile_now=False)
    assert net.resize(8, 8, 3, False) == 0
    net.compile()
    assert net.resize(16, 16, 3, False) == 0
    built, _ = _train_net(capi, graph, 16, 16, 1)
    assert _state(net) == _state(built)
    ran = {}
    for n in (net, built):
        n.data(0)[...] = np.random.RandomState(6).uniform(-1, 1, n.shape(0))
        n.upload(0)
        ran[n] = _trace(n.forward)
        n.sync()
    if pair == "conv_maxpool":
        assert "maxpool_fwd_s2_bn_kernel" in ran[net] and "maxpool_fwd_s2_bn_kernel" in ran[built], sorted(ran[net])
    assert ran[net] == ran[built]
    got, want = _backward(net, 7, last, first), _backward(built, 7, last, first)
    assert np.abs(want).max() > 0
    assert np.array_equal(_bits(got), _bits(want))
    net.close()
    built.close()
