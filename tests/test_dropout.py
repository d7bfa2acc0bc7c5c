"""The in-place dropout node, bcnn_add_dropout_layer (reference bcnn_dropout_layer.c):
  - a NumPy Philox4x32-10 against the published known-answer vectors (CPU);
  - the device mask (bcnn_hip_dropout_forward / _backward) against the NumPy definition of include/bcnn_hip.h, bit
    for bit, sizes not a multiple of 4 included;
  - the node: the backward reuses the forward's mask (whole passes and bcnn_forward_node / bcnn_backward_node), the
    same seed gives the same masks, another step or seed another one, the drop fraction, VALID / PREDICT identity,
    the refusals, the INI `probability` key, and a Darknet-dialect cfg whose [dropout] sits in the implicit chain."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of 32-bit words, key: 2 words -> 4 uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) for v in ctr]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(W0)) & _M32, (k1 + np.uint64(W1)) & _M32
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & _M32, p1 & _M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & _M32,
             p0 & _M32]
    return [v.astype(np.uint32) for v in c]


def np_dropped(size, rate, key, step):
    """include/bcnn_hip.h: element i uses word i % 4 of Philox((i/4 lo, i/4 hi, step lo, step hi), key)"""
    q = np.arange((size + 3) // 4, dtype=np.uint64)
    words = philox4x32_10([q & _M32, q >> np.uint64(32), np.full_like(q, step & 0xFFFFFFFF),
                           np.full_like(q, step >> 32)], (key & 0xFFFFFFFF, key >> 32))
    w = np.stack(words, axis=1).reshape(-1)[:size]
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u < np.float32(rate)


def _splitmix64(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def dropout_key(seed, node, rank=0):
    """host/bcnn_layers_lrn_dropout.c: bcnn_dropout_key"""
    return _splitmix64(seed ^ _splitmix64(((rank & 0xFFFFFFFF) << 32) | (node & 0xFFFFFFFF)))


def np_dropout(x, rate, key, step):
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
    return np.where(np_dropped(x.size, rate, key, step).reshape(x.shape), np.float32(0), x * scale).astype(np.float32)


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 R=10 (Salmon et al., SC11)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in philox4x32_10(ctr, key)) == want
    hdr = "/opt/rocm/include/rocrand/rocrand_philox4x32_10.h"
    if os.path.exists(hdr):  # the multiplier and key-increment constants of the ROCm header (constants only, not output)
        text = open(hdr).read()
        got = [int(re.search(r"#define ROCRAND_PHILOX_%s\s+(0x[0-9A-Fa-f]+)" % n, text).group(1), 16)
               for n in ("M4x32_0", "M4x32_1", "W32_0", "W32_1")]
        assert got == [M0, M1, W0, W1]


def test_mask_definition_is_uniform_and_keyed():
    a = np_dropped(1 << 16, 0.5, dropout_key(0, 3), 0)
    assert abs(a.mean() - 0.5) < 5 * 0.5 / 256
    assert (a != np_dropped(1 << 16, 0.5, dropout_key(0, 3), 1)).any()
    assert (a != np_dropped(1 << 16, 0.5, dropout_key(0, 4), 0)).any()
    assert (a != np_dropped(1 << 16, 0.5, dropout_key(0, 3, 1), 0)).any()


# ---- device ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size,rate,key,step", [(1, 0.5, 1, 0), (7, 0.3, 0xDEADBEEF12345678, 5),
                                                (4097, 0.5, 42, 1 << 33), (1000003, 0.1, 7, 3),
                                                (65538, 0.9, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF)])
def test_device_mask_matches_numpy(size, rate, key, step):
    import torch
    from bcnn_amd import ops
    rs = np.random.RandomState(size)
    x = rs.uniform(-2, 2, size).astype(np.float32)
    t = torch.from_numpy(x).cuda()
    ops.dropout_forward(t, rate, key, step)
    np.testing.assert_array_equal(t.cpu().numpy(), np_dropout(x, rate, key, step))
    g = rs.uniform(-1, 1, size).astype(np.float32)
    tg = torch.from_numpy(g).cuda()
    ops.dropout_backward(tg, rate, key, step)
    np.testing.assert_array_equal(tg.cpu().numpy(), np_dropout(g, rate, key, step))
    # an unaligned start (scalar path) draws the same mask
    big = torch.zeros(size + 1, device="cuda")
    big[1:] = torch.from_numpy(x).cuda()
    ops.dropout_forward(big[1:], rate, key, step)
    np.testing.assert_array_equal(big[1:].cpu().numpy(), np_dropout(x, rate, key, step))


@pytest.mark.gpu
def test_drop_fraction_seeds_and_steps():
    import torch
    from bcnn_amd import ops
    n, rate = 10_000_000, 0.3
    masks = []
    for key, step in ((11, 0), (11, 0), (11, 1), (12, 0)):
        t = torch.ones(n, device="cuda")
        ops.dropout_forward(t, rate, key, step)
        masks.append((t == 0).cpu().numpy())
    assert np.array_equal(masks[0], masks[1])
    assert not np.array_equal(masks[0], masks[2]) and not np.array_equal(masks[0], masks[3])
    sigma = (rate * (1 - rate) / n) ** 0.5
    for m in masks:
        assert abs(m.mean() - rate) < 5 * sigma


def _net(mode, rate, seed=None, shp=dict(w=5, h=3, c=4, n=6)):
    from bcnn_amd import capi
    net = capi.Net(mode=mode, **shp)
    net.fullc(37, act=capi.ACT_RELU, src="input", dst="fc1")
    net.dropout(rate, "fc1")
    net.fullc(5, src="fc1", dst="fc2")
    if seed is not None:
        net.L.bcnn_set_dropout_seed(net.net, seed)
    net.compile()
    return net


@pytest.mark.gpu
def test_node_backward_reuses_the_forward_mask():
    from bcnn_amd import capi
    rate, seed = 0.5, 1234
    net = _net(capi.MODE_TRAIN, rate, seed)
    rs = np.random.RandomState(3)
    net.data(0)[...] = rs.uniform(-1, 1, net.shape(0))
    net.upload(0)
    i = net.index("fc1")
    for step in range(3):  # one node at a time: the mask of step `step` of node 1
        net.forward_node(0)
        net.download(i)
        pre = net.data(i).copy()
        net.forward_node(1)
        net.download(i)
        want = np_dropout(pre, rate, dropout_key(seed, 1), step)
        np.testing.assert_array_equal(net.data(i), want)
        g = rs.uniform(-1, 1, pre.shape).astype(np.float32)
        net.grad(i)[...] = g
        net.upload(i, with_grad=True)
        net.backward_node(1)
        net.download(i)
        np.testing.assert_array_equal(net.grad(i), np_dropout(g, rate, dropout_key(seed, 1), step))
    # whole passes continue the step count; the gradient reaching fc1 carries the same mask
    net.forward()
    net.download(i)
    dropped = np_dropped(pre.size, rate, dropout_key(seed, 1), 3).reshape(pre.shape)
    assert (net.data(i)[dropped] == 0).all()
    net.grad(net.index("fc2"))[...] = 1.0
    net.upload(net.index("fc2"), with_grad=True)
    net.backward()
    net.download(i)
    assert (net.grad(i)[dropped] == 0).all() and (net.grad(i)[~dropped] != 0).any()
    net.close()


@pytest.mark.gpu
def test_same_seed_same_run_and_valid_identity():
    from bcnn_amd import capi
    outs = []
    for seed in (5, 5, 6):
        ctypes.CDLL(None).srand(1)  # the same initial weights
        net = _net(capi.MODE_TRAIN, 0.4, seed)
        net.data(0)[...] = np.linspace(-1, 1, net.data(0).size).reshape(net.shape(0))
        net.upload(0)
        net.forward()
        net.forward()
        net.download(net.index("fc2"))
        outs.append(net.data(net.index("fc2")).copy())
        net.close()
    assert np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])
    for mode in (capi.MODE_VALID, capi.MODE_PREDICT):
        net = _net(mode, 0.4, 5)
        net.data(0)[...] = np.linspace(-1, 1, net.data(0).size).reshape(net.shape(0))
        net.upload(0)
        i = net.index("fc1")
        net.forward_node(0)
        net.download(i)
        before = net.data(i).copy()
        net.forward()
        net.download(i)
        assert np.array_equal(net.data(i).view(np.uint32), before.view(np.uint32))
        net.close()


@pytest.mark.gpu
def test_refusals_and_ini_probability_key(tmp_path):
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=4, h=3, c=2, n=2)
    assert net.L.bcnn_add_dropout_layer(net.net, 0.5, b"input") != 0  # not the first node (reference :36-38)
    net.fullc(8, src="input", dst="fc1")
    nodes = net.L.bcnn_get_num_nodes(net.net)
    for rate in (-0.1, 1.0, 1.5, float("nan")):
        assert net.L.bcnn_add_dropout_layer(net.net, rate, b"fc1") != 0, rate
        assert net.L.bcnn_get_num_nodes(net.net) == nodes
    assert net.L.bcnn_add_dropout_layer(net.net, 0.5, b"nosuch") != 0
    net.dropout(0.0, "fc1")
    net.close()
    cfg = tmp_path / "drop.conf"
    cfg.write_text("[network]\ninput_width=4\ninput_height=3\ninput_channels=2\nbatch_size=2\n\n"
                   "[connected]\noutput=16\nsrc=input\ndst=fc1\n\n[dropout]\nprobability=0.5\nsrc=fc1\n\n"
                   "[connected]\noutput=3\nsrc=fc1\ndst=fc2\n")
    net = capi.Net.load_net(str(cfg), mode=capi.MODE_TRAIN)
    assert net.num_nodes == 3
    net.L.bcnn_compile_net(net.net)
    net.data(0)[...] = 1.0
    net.upload(0)
    net.forward()
    i = net.index("fc1")
    net.download(i)
    v = net.data(i)
    assert (v == 0).any()
    net.close()


DARKNET_DROPOUT_CFG = """
[net]
batch=2
width=4
height=3
channels=2

[connected]
output=16
activation=relu
%s
[route]
layers=-1

[connected]
output=3
activation=linear
"""


@pytest.mark.gpu
def test_darknet_cfg_chains_through_dropout(tmp_path):
    """Darknet sections name no tensors: an in-place [dropout] stands for its source in the implicit chain and in the
    `layers=` offsets. With the dropout section the net computes what the same cfg without it computes (PREDICT), and
    it drops in TRAIN."""
    from bcnn_amd import capi
    rs = np.random.RandomState(6)
    model = tmp_path / "fc.weights"
    with open(model, "wb") as fp:
        fp.write(struct.pack("<iii", 0, 2, 0) + struct.pack("<Q", 0))
        for cnt in (16, 16 * 24, 3, 3 * 16):
            fp.write(rs.uniform(-1, 1, cnt).astype(np.float32).tobytes())
    x = rs.uniform(-1, 1, (2, 2, 3, 4)).astype(np.float32)
    outs = []
    for with_dropout in (True, False):
        cfg = tmp_path / ("d%d.cfg" % with_dropout)
        cfg.write_text(DARKNET_DROPOUT_CFG % ("\n[dropout]\nprobability=.5\n" if with_dropout else ""))
        net = capi.Net.load_net(str(cfg), str(model), mode=capi.MODE_PREDICT)
        assert net.num_nodes == (4 if with_dropout else 3)
        fc1 = net.L.bcnn_get_node_tensor(net.net, 0, 1, 0)
        assert net.L.bcnn_get_node_tensor(net.net, net.num_nodes - 2, 0, 0) == fc1  # the route reads fc1's tensor
        net.compile()
        net.data(0)[...] = x
        net.upload(0)
        net.forward()
        out = net.L.bcnn_get_node_tensor(net.net, net.num_nodes - 1, 1, 0)
        net.download(out)
        outs.append(net.data(out).copy())
        if with_dropout:
            assert net.set_mode(capi.MODE_TRAIN) == 0
            net.compile()
            net.forward_node(0)
            net.download(fc1)
            pre = net.data(fc1).copy()
            net.forward_node(1)
            net.download(fc1)
            want = np_dropout(pre, 0.5, dropout_key(0, 1), 0)
            np.testing.assert_array_equal(net.data(fc1), want)
            assert (want == 0).sum() > (pre == 0).sum()
        net.close()
    assert np.array_equal(outs[0], outs[1])
