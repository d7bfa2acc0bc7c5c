"""GPU: the classifier loaders on a net that ends in the softmax-loss node. Its label tensor is [n][1][1][1], and the
MNIST, CIFAR-10 and classification-list readers write the class number itself into the one float of the slot (a one-hot
write into one float turns class 0 into 1.0 and every other class into 0.0). Host route, device route, and device decode
of a JPEG list; the node then counts every sample valid. The same files on a [softmax] -> [cost] net keep their one-hot
rows."""
import io

import numpy as np
import pytest
from PIL import Image

from tests.test_data_loader import _next, _set_loader, _write_cifar, _write_mnist

pytestmark = pytest.mark.gpu
TRAIN = 1


def _loss_net(w, h, c, n, device=False, decode=False):
    from bcnn_amd import capi
    net = capi.Net(mode=TRAIN, w=w, h=h, c=c, n=n)
    net.conv(4, 3, 2, 1, dst="c1")
    net.fullc(10, capi.ACT_NONE, "c1", "fc")
    node = net.softmax_loss("fc", "prob")
    assert net.shape(1) == (n, 1, 1, 1)
    assert net.set_loader_on_device(device) == 0 and net.set_loader_decode_on_device(decode) == 0
    return net, node


def _cost_net(w, h, c, n):
    from bcnn_amd import capi
    net = capi.Net(mode=TRAIN, w=w, h=h, c=c, n=n)
    net.fullc(10, capi.ACT_NONE, "input", "fc")
    net.softmax("fc", "prob")
    net.cost("prob", "label", "cost", 1.0)
    return net


def _mnist_labels(path, n):
    return np.frombuffer(open(path, "rb").read()[8:8 + n], np.uint8)


def _check(net, node, want):
    """one batch: tensor 1 holds the class numbers as floats, on the host and on the device, and every sample is valid"""
    n = len(want)
    _, lab = _next(net)
    assert np.array_equal(lab.reshape(-1), np.asarray(want, np.float32)), (lab.reshape(-1), want)
    net.data(1)[...] = -1.0
    net.download(1, False)
    assert np.array_equal(net.data(1).reshape(-1), np.asarray(want, np.float32))
    net.forward()
    net.sync()
    stats = net.softmax_loss_stats(node)
    assert stats["valid"] == n and stats["ignored"] == 0 and stats["out_of_range"] == 0, stats


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_mnist_writes_class_numbers(tmp_path, device):
    pi, pl = _write_mnist(tmp_path, "train", 12)
    digits = _mnist_labels(pl, 12)
    assert len(set(digits)) > 2 and (digits > 1).any()
    net, node = _loss_net(28, 28, 1, 6, device)
    assert _set_loader(net, 0, pi, pl, None, None) == 0
    net.compile()
    _check(net, node, digits[:6])
    _check(net, node, digits[6:])
    net.close()
    cost = _cost_net(28, 28, 1, 6)
    assert _set_loader(cost, 0, pi, pl, None, None) == 0
    cost.compile()
    _, lab = _next(cost)
    assert np.array_equal(lab.reshape(6, 10), np.eye(10, dtype=np.float32)[digits[:6]])
    cost.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_cifar_writes_class_numbers(tmp_path, device):
    p = _write_cifar(tmp_path, "data_batch_1", 8)
    raw = np.frombuffer(open(p, "rb").read(), np.uint8).reshape(8, 3073)
    classes = raw[:, 0]
    net, node = _loss_net(32, 32, 3, 4, device)
    assert _set_loader(net, 1, p, None, None, None) == 0
    net.compile()
    _check(net, node, classes[:4])
    _check(net, node, classes[4:])
    net.close()
    cost = _cost_net(32, 32, 3, 4)
    assert _set_loader(cost, 1, p, None, None, None) == 0
    cost.compile()
    _, lab = _next(cost)
    assert np.array_equal(lab.reshape(4, 10), np.eye(10, dtype=np.float32)[classes[:4]])
    cost.close()


@pytest.mark.parametrize("route", ["host", "device", "device_decode"])
def test_classification_list_writes_class_numbers(tmp_path, route):
    rs = np.random.RandomState(2)
    classes = [3, 0, 9, 1, 7, 2, 5, 0]
    rows = []
    for k, cls in enumerate(classes):
        img = Image.fromarray(rs.randint(0, 256, (16, 16, 3)).astype(np.uint8), "RGB")
        p = tmp_path / ("im%d.%s" % (k, "jpg" if route == "device_decode" else "png"))
        img.save(p, **(dict(format="JPEG", quality=90) if route == "device_decode" else {}))
        rows.append("%s %d" % (p, cls))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(rows) + "\n")
    net, node = _loss_net(16, 16, 3, 4, device=route != "host", decode=route == "device_decode")
    assert _set_loader(net, 2, str(lst), None, None, None) == 0
    net.compile()
    _check(net, node, classes[:4])
    if route == "device_decode":
        assert net.loader_device_decoded() == 4
    _check(net, node, classes[4:])
    net.close()
    cost = _cost_net(16, 16, 3, 4)
    assert _set_loader(cost, 2, str(lst), None, None, None) == 0
    cost.compile()
    _, lab = _next(cost)
    assert np.array_equal(lab.reshape(4, 10), np.eye(10, dtype=np.float32)[classes[:4]])
    cost.close()


def test_a_negative_class_is_written_as_it_is(tmp_path):
    rs = np.random.RandomState(4)
    rows = []
    for k, cls in enumerate([-1, 4, -3, 9]):
        p = tmp_path / ("im%d.png" % k)
        Image.fromarray(rs.randint(0, 256, (16, 16, 3)).astype(np.uint8), "RGB").save(p)
        rows.append("%s %d" % (p, cls))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(rows) + "\n")
    net, node = _loss_net(16, 16, 3, 4)
    assert _set_loader(net, 2, str(lst), None, None, None) == 0
    net.compile()
    _, lab = _next(net)
    assert np.array_equal(lab.reshape(-1), np.float32([-1, 4, -3, 9]))
    net.forward()
    net.sync()
    stats = net.softmax_loss_stats(node)
    assert stats["valid"] == 2 and stats["out_of_range"] == 2, stats
    net.close()
