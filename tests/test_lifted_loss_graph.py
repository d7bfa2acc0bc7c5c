"""The lifted-structure loss inside a TRAIN graph, against the unmodified reference (oracle/_ref/libbcnn_ref.so): a cut-down
version of the reference's metric-learning example (conv+bn+relu, maxpool, conv+bn, maxpool, a 64-wide fc embedding, the
lifted cost; batch 32 of 16 x 16 images), built through the builders and through an INI file with
loss=lifted_struct_similarity. Both nets start from one model file written by the reference, take three SGD steps on the
same batch, and every parameter tensor is compared after each step at NET_TOL."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_bind as rb
from tests.test_lifted_loss import LOSS_LIFTED, labels, model, one_hot

pytestmark = pytest.mark.gpu
NET_TOL = 1e-4  # tests/test_net_parity.py
SHAPE = dict(w=16, h=16, c=3, n=32)
PARAM_ENDS = ("_w", "_b", "_scales", "_run_mean", "_run_var")

CFG = """
[network]
input_width=16
input_height=16
input_channels=3
batch_size=32
optimizer=sgd
momentum=0.9
decay=0.0005
learning_rate=0.01

[convolutional]
filters=8
size=3
stride=1
pad=1
bn=1
init=xavier
function=relu
src=input
dst=c1

[maxpool]
size=2
stride=2
src=c1
dst=p1

[convolutional]
filters=8
size=3
stride=1
pad=1
bn=1
init=xavier
function=none
src=p1
dst=c2

[maxpool]
size=2
stride=2
src=c2
dst=p2

[connected]
output=64
init=xavier
function=none
src=p2
dst=fc

[cost]
src=fc
dst=out
loss=lifted_struct_similarity
metric=error
scale=1.0
"""


def _graph(net, is_ref):
    net.conv(8, 3, 1, 1, bn=1, act=rb.ACT_RELU, src="input", dst="c1")
    net.maxpool(2, 2, src="c1", dst="p1")
    net.conv(8, 3, 1, 1, bn=1, act=rb.ACT_NONE, src="p1", dst="c2")
    net.maxpool(2, 2, src="c2", dst="p2")
    net.fullc(64, src="p2", dst="fc")
    if is_ref:
        assert net.L.bcnn_add_cost_layer(net.net, LOSS_LIFTED, 0, 1.0, b"fc", b"label", b"out") == 0
    else:
        from bcnn_amd import capi
        net.cost("fc", dst="out", loss=capi.LOSS_LIFTED_STRUCT)


def _compare(tag, a, b, tol=NET_TOL):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a64.shape == b64.shape, (tag, a64.shape, b64.shape)
    assert np.isfinite(a64).all(), tag
    diff = float(np.max(np.abs(a64 - b64))) if a64.size else 0.0
    assert diff <= tol * float(np.max(np.abs(b64))) + 1e-7, "%s: max abs diff %.3g" % (tag, diff)


def _three_steps(ref, hip, tmp_path):
    nt = ref.L.ref_num_tensors(ref.net)
    names = [ref.L.ref_tensor_name(ref.net, i).decode() for i in range(nt)]
    for i, name in enumerate(names):
        assert hip.index(name) == i, name
    rs = np.random.RandomState(11)
    for i, name in enumerate(names):  # distinctive parameters on the reference, handed over through its model file
        if name.endswith(("_w", "_b")):
            ref.data(i)[...] = rs.uniform(-0.3, 0.3, ref.shape(i))
    path = str(tmp_path / "start.bcnnmodel")
    assert ref.save_weights(path) == 0 and hip.load_weights(path) == 0
    cls = labels(32, 4, "uniform", rs)
    ref.data(0)[...] = rs.uniform(-1, 1, ref.shape(0))
    ref.data(1)[...] = one_hot(cls, 64).reshape(ref.shape(1))
    for i in (0, 1):
        hip.data(i)[...] = ref.data(i)
        hip.upload(i)
    fc, out = names.index("fc"), names.index("out")
    params = [i for i, name in enumerate(names) if name.endswith(PARAM_ENDS)]
    assert len(params) >= 8
    for it in range(3):
        ref.forward()
        hip.forward()
        ref.backward()
        hip.backward()
        hip.download(fc)
        hip.download(out, False)
        _compare("it%d fc" % it, hip.data(fc), ref.data(fc))
        _compare("it%d dfc" % it, hip.grad(fc), ref.grad(fc))
        assert hip.data(out).ravel()[0] == ref.data(out).ravel()[0]  # the metric
        want_loss, P, _ = model(ref.data(fc).reshape(32, 64), cls)
        loss, got_P = hip.lifted_struct_loss()
        assert got_P == P and abs(loss - want_loss) <= 1e-4 * want_loss
        for i in params:
            # (not the biases: in front of a batch-norm their gradient is analytically zero, rounding noise on both sides;
            # they are compared as values after the update)
            if names[i].endswith(("_w", "_scales")):
                hip.download(i)
                _compare("it%d d%s" % (it, names[i]), hip.grad(i), ref.grad(i))
        ref.L.bcnn_update(ref.net)
        hip.update()
        for i in params:
            hip.download(i)
            _compare("it%d %s" % (it, names[i]), hip.data(i), ref.data(i))
    assert np.abs(ref.grad(fc)).max() > 0


def test_builder_graph_trains_like_the_reference(tmp_path):
    if not rb.available():
        pytest.skip("oracle/_ref not present")
    from bcnn_amd import capi
    ref = rb.RefNet(mode=rb.MODE_TRAIN, **SHAPE)
    ref.L.ref_set_threads(ref.net, 4)
    _graph(ref, True)
    hip = capi.Net(mode=capi.MODE_TRAIN, **SHAPE)
    _graph(hip, False)
    ref.compile()
    hip.compile()
    ref.L.bcnn_set_sgd_optimizer(ref.net, 0.01, 0.9)
    ref.L.bcnn_set_weight_regularizer(ref.net, 5e-4)
    hip.set_sgd(0.01, 0.9, 5e-4)
    _three_steps(ref, hip, tmp_path)
    ref.close()
    hip.close()


def test_ini_graph_trains_like_the_reference(tmp_path):
    if not rb.available():
        pytest.skip("oracle/_ref not present")
    from tests.test_load_net import load_both, same_graph
    cfg = tmp_path / "lifted.conf"
    cfg.write_text(CFG)
    C.CDLL(None).srand(20240607)
    ref, st_ref, hip, st = load_both(str(cfg), None, rb.MODE_TRAIN)
    assert st_ref == 0 and st == 0
    same_graph(ref, hip)
    assert ref.L.bcnn_compile_net(ref.net) == 0 and hip.L.bcnn_compile_net(hip.net) == 0
    _three_steps(ref, hip, tmp_path)
    assert ref.L.bcnn_get_tensor_index_by_name(ref.net, b"out") == hip.index("out")
