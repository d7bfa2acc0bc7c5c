"""The window-attention node inside a net built from a config string: [window_attention] (shift > 0, rel_bias=1) behind three
1x1 convolutions and in front of an in-place relu. Forward and source gradients of one TRAIN step against the float64
formulas of tests/test_window_attention.py (bar 1e-5 of the largest value, dtable its DTABLE_TOL), the SGD step of the table,
the native model file, bcnn_resize_net, and every refusal of the builder."""
import ctypes as C

import numpy as np
import pytest

from tests.test_attention_net import _bits, _data, _feed, _grad, _t
from tests.test_window_attention import DTABLE_TOL, reference

SEED = 20261126
INVALID_PARAMETER = 1
HEADS, WS, SHIFT = 2, 2, 1
CFG = "[net]\ninput_width=6\ninput_height=4\ninput_channels=4\nbatch_size=2\n" + "".join(
    "\n[conv]\nfilters=%d\nsize=1\nstride=1\npad=0\nactivation=linear\nsrc=input\ndst=%s\n" % (f, n)
    for n, f in (("a", 4), ("b", 4), ("c", 6))) + """
[window_attention]
heads=2
window=2
shift=1
rel_bias=1
src=a,b,c
dst=att

[activation]
function=relu
src=att

[cost]
src=att
dst=cost
"""


def _net(tmp_path, mode):
    from bcnn_amd import capi
    cfg = tmp_path / "window.cfg"
    cfg.write_text(CFG)
    C.CDLL(None).srand(SEED)
    net = capi.Net.load_net(str(cfg), None, mode=mode)
    net.compile()
    table = net.index("att_relbias")
    net.data(table)[...] = np.random.RandomState(9).standard_normal(net.shape(table))
    net.upload(table)
    return net, 3, table


def _reference(net, node, dy):
    q, k, v = [_data(net, net.node_src(node, i)).astype(np.float64) for i in range(3)]
    split = lambda a: a.reshape(a.shape[0], HEADS, -1, *a.shape[2:])
    table = _data(net, net.node_src(node, 3)).astype(np.float64).reshape(HEADS, -1)
    ref, _ = reference(split(q), split(k), split(v), split(dy.astype(np.float64)), table, WS, SHIFT, 1.0 / np.sqrt(q.shape[1] // HEADS))
    return ref


@pytest.mark.gpu
def test_train_step_model_file_and_resize(tmp_path):
    from bcnn_amd import capi, ops
    net, node, table = _net(tmp_path, capi.MODE_TRAIN)
    att = net.index("att")
    assert net.node_type(node) == capi.LAYER_WINDOW_ATTENTION and net.shape(att) == (2, 6, 4, 6)
    assert net.shape(table) == (1, 1, 1, HEADS * 9) and net.node_src(node, 3) == table
    lr, momentum, decay = 0.05, 0.9, 0.0
    net.set_sgd(lr, momentum, decay)
    _feed(net, 3)
    _feed(net, 4, 1)
    for i in range(node + 1):
        net.forward_node(i)
    net.sync()
    out = _data(net, att)   # before the in-place relu rewrites it
    net.forward()
    net.backward()
    net.sync()
    dy, before = _grad(net, att), _data(net, table)
    ref = _reference(net, node, dy)
    assert (_data(net, att) == 0).any() and (out < 0).any(), "the relu did rewrite the output"
    got = dict(o=out, dtable=_grad(net, table), **{name: _grad(net, net.node_src(node, i)) for i, name in enumerate(("dq", "dk", "dv"))})
    for name, value in got.items():
        err, bar = np.abs(value.reshape(ref[name].shape) - ref[name]).max(), (DTABLE_TOL if name == "dtable" else 1e-5) * np.abs(ref[name]).max()
        print("%s: max error %.3g, bar %.3g" % (name, err, bar))
        assert err <= bar and np.abs(value).max() > 0, (name, err, bar)
    # the table moves by the learner's SGD rule on dtable: the bits of ops.sgd_update, against the gradient
    tw = _t(before.ravel())
    ops.sgd_update(tw, None, _t(got["dtable"].ravel()), None, 2, lr, momentum, decay)
    net.update()
    net.sync()
    after = _data(net, table)
    assert np.array_equal(_bits(after.ravel()), _bits(tw.cpu().numpy()))
    step = (after - before).ravel()
    assert (np.sign(step) == -np.sign(got["dtable"].ravel())).all() and np.abs(step).max() > 0
    # the native model file holds the table, bit for bit
    path = str(tmp_path / "window.bcnnmodel")
    assert net.save_weights(path) == 0
    other, node_o, table_o = _net(tmp_path, capi.MODE_PREDICT)
    assert not np.array_equal(_bits(_data(other, table_o)), _bits(after))
    assert other.load_weights(path) == 0 and np.array_equal(_bits(_data(other, table_o)), _bits(after))
    other.close()
    # bcnn_resize_net: another multiple of the window runs, a non-multiple is refused and changes nothing
    assert net.resize(8, 6, 4, need_realloc=True) == 0 and net.shape(att) == (1, 6, 6, 8)
    assert net.resize(7, 6, 4, need_realloc=True) == INVALID_PARAMETER and net.shape(att) == (1, 6, 6, 8)
    _feed(net, 5)
    for i in range(node + 1):
        net.forward_node(i)
    net.sync()
    ref = _reference(net, node, np.zeros(net.shape(att)))
    assert np.abs(_data(net, att) - ref["o"].reshape(net.shape(att))).max() <= 1e-5 * np.abs(ref["o"]).max()
    net.close()


def test_builder_refusals_leave_the_node_count():
    """no node is built, so no device is needed: q, k, v are the input [2][8][4][4] and the label tensor in a shape set here"""
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_PREDICT, w=4, h=4, c=8, n=2)
    L, label = net.L, net.tensor(1)
    same = (b"input", b"input", b"input")
    cases = [((2, 8, 4, 4), 2, 2, 0, (b"nope", b"input", b"input")),     # an unknown source, in each slot
             ((2, 8, 4, 4), 2, 2, 0, (b"input", b"nope", b"input")),
             ((2, 8, 4, 4), 2, 2, 0, (b"input", b"input", b"nope")),
             ((3, 8, 4, 4), 2, 2, 0, (b"input", b"input", b"label")),    # different N
             ((2, 8, 2, 4), 2, 2, 0, (b"input", b"input", b"label")),    # v of another extent
             ((2, 8, 4, 2), 2, 2, 0, (b"input", b"label", b"input")),    # k of another extent
             ((2, 4, 4, 4), 2, 2, 0, (b"input", b"label", b"input")),    # q and k of different depth
             ((2, 8, 4, 4), 0, 2, 0, same), ((2, 8, 4, 4), 3, 2, 0, same),   # heads: none, dividing neither depth
             ((2, 6, 4, 4), 4, 2, 0, (b"input", b"input", b"label")),    # ... and only q's and k's
             ((2, 8, 4, 4), 2, 0, 0, same),                              # window < 1
             ((2, 8, 9, 9), 2, 9, 0, (b"label", b"label", b"label")),    # window^2 > 64
             ((2, 8, 4, 4), 2, 3, 0, same),                              # H and W no multiple of the window
             ((2, 8, 4, 6), 2, 4, 0, (b"label", b"label", b"label")),    # W alone
             ((2, 8, 4, 4), 2, 2, -1, same), ((2, 8, 4, 4), 2, 2, 2, same),   # shift outside [0, window)
             ((2, 130, 4, 4), 2, 2, 0, (b"label", b"label", b"input")),  # d = 65
             ((2, 65, 4, 4), 1, 2, 0, (b"input", b"input", b"label")),   # c = 65
             ((2, 8, 32768, 8192), 2, 2, 0, (b"label", b"label", b"label"))]   # 2^32 elements
    for shape, heads, window, shift, (q, k, v) in cases:
        label.n, label.c, label.h, label.w = shape
        status = L.bcnn_add_window_attention_layer(net.net, heads, window, shift, 1, 0.0, q, k, v, b"att")
        assert status == INVALID_PARAMETER, (shape, heads, window, shift, q, k, v)
        assert L.bcnn_get_num_nodes(net.net) == 0 and not L.bcnn_peek_tensor(net.net, 2), "nothing was added"
    label.n = label.c = label.h = label.w = 0   # (the net owns no device memory; bcnn_end_net would ask for the device)
