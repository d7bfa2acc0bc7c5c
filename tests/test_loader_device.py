"""The device loader path (bcnn_set_loader_on_device, bcnn_amd/csrc/augment.hip): with the switch on,
bcnn_loader_next leaves reading, decoding and the rand() draws on the host and makes the float input batch on the device.
The bar is the one tests/test_data_loader.py holds the host path to: BIT-EXACT. The device tensor after every batch is
compared with

  (a) this library's host path on a second net with the switch off: same files, same libc srand() seed -- always;
  (b) the unmodified reference (oracle/_ref) wherever it is present;

with np.array_equal, together with the labels and with the value of rand() after the batches (the same number of draws).

The kernels take one route whatever the sample size (a lane per pixel, then a lane per 8 pixels of a row; no LDS-resident
image), so there is no size threshold to straddle and no case for one: the shapes below are the smallest that run every
stage, every loader, more than one block per sample, and widths that are and are not a multiple of 4."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from oracle import ref_bind as rb
from tests.test_data_loader import LIB, _augment, _next, _set_loader, _u8, _write_cifar, _write_mnist, libc

pytestmark = pytest.mark.gpu

TRAIN, VALID = rb.MODE_TRAIN, rb.MODE_VALID
RAND_MAX = 2147483647


def _graph(net, mod, classes):
    net.fullc(classes, mod.ACT_NONE, "input", "fc")
    net.softmax("fc", "prob")
    net.cost("prob", "label", "cost", 1.0)
    return net


def _trio(w, h, c, n, classes, with_ref=True):
    """the same one-layer graph three times: this build with the switch on, with it off, and the reference (or None)"""
    from bcnn_amd import capi
    dev = _graph(capi.Net(mode=TRAIN, w=w, h=h, c=c, n=n), capi, classes)
    host = _graph(capi.Net(mode=TRAIN, w=w, h=h, c=c, n=n), capi, classes)
    assert dev.set_loader_on_device(True) == 0 and dev.get_loader_on_device() == 1 and host.get_loader_on_device() == 0
    ref = _graph(rb.RefNet(mode=TRAIN, w=w, h=h, c=c, n=n), rb, classes) if with_ref and rb.available() else None
    return [x for x in (dev, host, ref) if x is not None]


def _dev_next(net):
    """one batch; the input as the DEVICE holds it (the host copy of tensor 0 is not written in this mode)"""
    net.L.bcnn_loader_next.argtypes = [C.c_void_p]
    net.L.bcnn_loader_next.restype = C.c_int
    assert net.L.bcnn_loader_next(net.net) == 0
    net.download(0, False)
    return net.data(0).copy(), net.data(1).copy()


def _play(net, script, seed, toggle=None):
    """script: (mode, batches) pairs. Returns the batches and the next value of rand(). toggle: per batch, the switch"""
    from bcnn_amd import capi
    libc.srand(seed)
    out, k = [], 0
    for mode, batches in script:
        net.L.bcnn_set_mode(net.net, mode)
        for _ in range(batches):
            if toggle is not None:
                assert net.set_loader_on_device(toggle[k % len(toggle)]) == 0
            mine = isinstance(net, capi.Net)
            out.append(_dev_next(net) if mine and net.get_loader_on_device() else _next(net))
            k += 1
    return out, libc.rand()


def _same(nets, script, seed):
    """plays the script on every net; the first one is the device path. Returns its batches."""
    runs = [_play(n, script, seed) for n in nets]
    for who, (out, nxt) in zip(("host path", "reference"), runs[1:]):
        assert len(out) == len(runs[0][0])
        for k, ((xa, ya), (xb, yb)) in enumerate(zip(runs[0][0], out)):
            assert np.array_equal(xa, xb), (who, "input", k, int((xa != xb).sum()))
            assert np.array_equal(ya, yb), (who, "label", k)
        assert nxt == runs[0][1], (who, "rand() draws")
    return runs[0][0]


def _close(nets):
    for n in nets:
        n.close()


@pytest.mark.parametrize("side", [28, 24], ids=["native_size", "centre_crop_to_24"])
def test_mnist(tmp_path, side):
    tr = _write_mnist(tmp_path, "train", 37, seed=1)      # 37 samples, batches of 16: wraps around inside the 3rd batch
    te = _write_mnist(tmp_path, "t10k", 20, seed=2)
    nets = _trio(side, side, 1, 16, 10)
    for n in nets:
        assert _set_loader(n, 0, tr[0], tr[1], te[0], te[1]) == 0
        _augment(n, shift=(5, 5), rotation=30.0)           # examples/mnist
        n.compile()
    got = _same(nets, [(TRAIN, 5), (VALID, 2), (TRAIN, 1), (VALID, 2)], seed=123)
    assert len({g[0].tobytes() for g in got[:5]}) == 5     # augmentation + wrap-around: no two batches alike
    assert np.array_equal(got[5][0], got[8][0]) and np.array_equal(got[6][0], got[9][0])   # VALID rewinds
    assert not np.array_equal(got[5][0], got[6][0])
    _close(nets)


@pytest.mark.parametrize("side", [32, 28])
def test_cifar10(tmp_path, side):
    tr, te = _write_cifar(tmp_path, "data_batch_1", 21, seed=3), _write_cifar(tmp_path, "test_batch", 9, seed=4)
    nets = _trio(side, side, 3, 8, 10)
    for n in nets:
        assert _set_loader(n, 1, tr, None, te, None) == 0
        _augment(n, flip=(1, 0), color=(-20, 20, 0.8, 1.2), shift=(4, 4))   # examples/cifar10 (+ a shift)
        n.compile()
    _same(nets, [(TRAIN, 4), (VALID, 2)], seed=77)
    _close(nets)


def test_every_stage_at_once(tmp_path):
    tr, te = _write_cifar(tmp_path, "data_batch_1", 21, seed=5), _write_cifar(tmp_path, "test_batch", 9, seed=6)
    seed, batches = 41, 3
    # the draws of a sample, in order: shift x, shift y, scale, rotation, contrast, brightness (the flip draws nothing)
    libc.srand(seed)
    scales = []
    for _ in range(8 * batches):
        r = [libc.rand() for _ in range(6)]
        scales.append(np.float32(np.float32(r[2]) / np.float32(RAND_MAX)) * np.float32(np.float32(1.1) - np.float32(0.9))
                      + np.float32(0.9))
    extents = [int(np.float32(32) * s) for s in scales]
    assert min(extents) < 32 < max(extents), extents       # pasted inside the sample, and cropped out of a larger image
    nets = _trio(32, 32, 3, 8, 10)
    for n in nets:
        assert _set_loader(n, 1, tr, None, te, None) == 0
        _augment(n, shift=(4, 0), scale=(0.9, 1.1), rotation=10.0, color=(-50, 10, 0.5, 1.5), flip=(1, 0))
        n.compile()
    _same(nets, [(TRAIN, batches), (VALID, 1)], seed=seed)
    _close(nets)


def test_shift_origins_beyond_the_image(tmp_path):
    tr = _write_mnist(tmp_path, "train", 37, seed=7)
    nets = _trio(28, 28, 1, 16, 10)
    for n in nets:
        assert _set_loader(n, 0, tr[0], tr[1], None, None) == 0
        _augment(n, shift=(70, 70))
        n.compile()
    got = _same(nets, [(TRAIN, 3)], seed=9)
    canvas = np.float32((np.float32(128) - np.float32(127.5)) * np.float32(1 / 127.5))
    blank = [bool(np.all(x[b] == canvas)) for x, _ in got for b in range(16)]
    assert any(blank) and not all(blank), blank
    _close(nets)


def _write_list_files(tmp_path, sizes, missing_at=(3,)):
    bip = C.CDLL(os.path.join(LIB, "libbip.so"))
    rs = np.random.RandomState(8)
    lines_c, lines_r = [], []
    for k in range(7):
        h, w = sizes[k % 2]
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        p = str(tmp_path / ("img%d.png" % k))
        assert bip.bip_write_image(p.encode(), _u8(img), w, h, 3, w * 3) == 0
        lines_c.append("%s %d" % (p, k % 4))
        lines_r.append("%s %.3f %.3f %.3f" % (p, *rs.uniform(-1, 1, 3)))
    try:      # JPEG files, decoded to the same pixels as the reference's stb_image (tests/test_bip.py)
        from PIL import Image
        for k in range(3):
            p = str(tmp_path / ("photo%d.jpg" % k))
            h, w = sizes[1]
            Image.fromarray(rs.randint(0, 256, (h + 2 * k, w + 1, 3)).astype(np.uint8)).save(
                p, "JPEG", quality=70 + 10 * k, subsampling=k, progressive=bool(k & 1))
            lines_c.append("%s %d" % (p, k))
            lines_r.append("%s %.3f %.3f %.3f" % (p, *rs.uniform(-1, 1, 3)))
    except ImportError:
        pass
    for at in missing_at:   # an unreadable sample: the sample buffer keeps what it held and is augmented again
        lines_c.insert(at, str(tmp_path / "missing.png") + " 1")
    (tmp_path / "c.txt").write_text("\n".join(lines_c) + "\n")
    (tmp_path / "r.txt").write_text("\n".join(lines_r) + "\n")


@pytest.mark.parametrize("kind,path,classes", [(2, "c.txt", 4), (3, "r.txt", 3)], ids=["classification", "regression"])
def test_list_loaders(tmp_path, kind, path, classes):
    _write_list_files(tmp_path, ((16, 16), (20, 24)))     # some images are larger than the net input: cropped at random
    nets = _trio(16, 16, 3, 4, classes)
    for n in nets:
        assert _set_loader(n, kind, str(tmp_path / path), None, str(tmp_path / path), None) == 0
        _augment(n, color=(-10, 30, 0.7, 1.3), rotation=20.0)
        n.compile()
    _same(nets, [(TRAIN, 5), (VALID, 2)], seed=31)
    _close(nets)


def test_input_width_that_is_no_multiple_of_4(tmp_path):
    """17 x 23 x 3: every row of every plane starts at another alignment, so the scalar head and tail of the stores run"""
    _write_list_files(tmp_path, ((23, 17), (27, 22)), missing_at=(0, 5))
    nets = _trio(17, 23, 3, 3, 4)
    for n in nets:
        assert _set_loader(n, 2, str(tmp_path / "c.txt"), None, str(tmp_path / "c.txt"), None) == 0
        _augment(n, shift=(3, 2), scale=(0.8, 1.2), color=(-10, 30, 0.7, 1.3), rotation=20.0)
        n.compile()
    _same(nets, [(TRAIN, 6), (VALID, 2)], seed=57)
    _close(nets)


NET_CONF = """[net]
batch=8
width=32
height=32
channels=3
%s
[connected]
output=10
src=input
dst=fc
[softmax]
src=fc
dst=prob
[cost]
src=prob
dst=out
loss=euclidean
metric=error
"""


def test_draws_of_the_effects_that_are_not_built(tmp_path):
    """max_distortion / max_spots: the draws are consumed and the pixels left alone, on both paths of this build (the
    reference applies the two effects, so it is no yardstick here). The nets come from config files, which is also how
    the [net] key loader_on_device reaches a net with layers."""
    from bcnn_amd import capi
    tr = _write_cifar(tmp_path, "data_batch_1", 21, seed=5)
    keys = "max_distortion=0.3\nmax_spots=3\nrange_shift_x=4\nrange_shift_y=4\nmin_contrast=0.8\nmax_contrast=1.2\nflip_h=1\n"
    nets = []
    for extra in ("loader_on_device=1\n", ""):
        cfg = tmp_path / ("net%d.conf" % len(nets))
        cfg.write_text(NET_CONF % (keys + extra))
        net = capi.Net.load_net(str(cfg), None, mode=capi.MODE_TRAIN)
        assert _set_loader(net, 1, tr, None, tr, None) == 0
        _augment(net, flip=(1, 0))
        net.compile()
        nets.append(net)
    assert [n.get_loader_on_device() for n in nets] == [1, 0]
    got = _same(nets, [(TRAIN, 4), (VALID, 1)], seed=3)
    # the spots' draws vary in number from sample to sample: a net without the two keys sees other samples
    cfg = tmp_path / "plain.conf"
    cfg.write_text(NET_CONF % keys.replace("max_distortion=0.3\nmax_spots=3\n", ""))
    plain = capi.Net.load_net(str(cfg), None, mode=capi.MODE_TRAIN)
    assert _set_loader(plain, 1, tr, None, tr, None) == 0
    _augment(plain, flip=(1, 0))
    plain.compile()
    other, _ = _play(plain, [(TRAIN, 4)], seed=3)
    assert np.array_equal(other[0][0][0], got[0][0][0]) and not np.array_equal(other[0][0], got[0][0])
    _close(nets + [plain])


def test_darknet_net_section_sets_the_switch(tmp_path):
    from bcnn_amd import capi
    from tests.test_load_net import DARKNET_CFG
    rs = np.random.RandomState(1)
    model = tmp_path / "tiny.weights"
    with open(model, "wb") as fp:
        fp.write(struct.pack("<iii", 0, 2, 0) + struct.pack("<Q", 7))
        for cnt in (4, 4, 4, 4, 4 * 3 * 9, 4, 4 * 4):
            fp.write(rs.uniform(-1, 1, cnt).astype(np.float32).tobytes())
    for text, want in ((DARKNET_CFG.replace("channels=3\n", "channels=3\nloader_on_device=1\n"), 1), (DARKNET_CFG, 0)):
        cfg = tmp_path / "tiny.cfg"
        cfg.write_text(text)
        net = capi.Net.load_net(str(cfg), str(model), mode=capi.MODE_PREDICT)
        assert net.get_loader_on_device() == want
        net.close()


@pytest.mark.parametrize("loader", ["mnist", "list"])
def test_toggling_between_batches(tmp_path, loader):
    """off -> on -> off -> on ... on one net gives the batches of a net that never toggled. The list file has unreadable
    entries, whose slots show the previous sample augmented twice: the path that decoded that sample must not matter."""
    if loader == "mnist":
        tr = _write_mnist(tmp_path, "train", 37, seed=1)
        nets = _trio(28, 28, 1, 16, 10, with_ref=False)
        for n in nets:
            assert _set_loader(n, 0, tr[0], tr[1], tr[0], tr[1]) == 0
            _augment(n, shift=(5, 5), rotation=30.0)
            n.compile()
    else:
        _write_list_files(tmp_path, ((16, 16), (20, 24)), missing_at=(0, 4, 4, 9))
        nets = _trio(16, 16, 3, 4, 4, with_ref=False)
        for n in nets:
            assert _set_loader(n, 2, str(tmp_path / "c.txt"), None, str(tmp_path / "c.txt"), None) == 0
            _augment(n, color=(-10, 30, 0.7, 1.3), rotation=20.0, shift=(3, 3))
            n.compile()
    toggled, host = nets
    script = [(TRAIN, 7), (VALID, 2), (TRAIN, 2)]
    a, ra = _play(toggled, script, seed=11, toggle=(False, True, True, False))
    b, rb_ = _play(host, script, seed=11)
    assert ra == rb_
    for k, ((xa, ya), (xb, yb)) in enumerate(zip(a, b)):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb), k
    _close(nets)


def test_host_copy_of_the_input_is_left_alone(tmp_path):
    tr = _write_mnist(tmp_path, "train", 37, seed=1)
    dev, host = _trio(28, 28, 1, 16, 10, with_ref=False)
    for n in (dev, host):
        assert _set_loader(n, 0, tr[0], tr[1], None, None) == 0
        _augment(n, shift=(5, 5), rotation=30.0)
        n.compile()
    dev.data(0)[...] = 7.25
    libc.srand(5)
    dev.L.bcnn_loader_next.argtypes = [C.c_void_p]
    assert dev.L.bcnn_loader_next(dev.net) == 0
    assert np.all(dev.data(0) == 7.25)                     # not written, and not uploaded over the device's batch
    libc.srand(5)
    want, labels = _next(host)
    assert np.array_equal(dev.data(1), labels)
    dev.download(0, False)
    assert np.array_equal(dev.data(0), want)
    t = dev.L.bcnn_get_tensor_by_index(dev.net, 0).contents   # the reference's accessor refreshes too
    assert np.array_equal(np.ctypeslib.as_array(t.data, shape=(want.size,)), want.ravel())
    _close([dev, host])


@pytest.mark.skipif(not rb.available(), reason="oracle/_ref not present")
def test_mnist_example_graph_trains_from_the_device_loader_like_the_reference(tmp_path):
    """the graph and the set-up of tests/test_data_loader.py's example test, six bcnn_train_on_batch steps, switch on"""
    from bcnn_amd import capi
    tr = _write_mnist(tmp_path, "train", 64, seed=11)
    te = _write_mnist(tmp_path, "t10k", 32, seed=12)
    nets = []
    for mod, cls in ((rb, rb.RefNet), (capi, capi.Net)):
        libc.srand(2024)
        net = cls(mode=mod.MODE_TRAIN, w=28, h=28, c=1, n=16)
        net.conv(32, 3, 1, 1, 1, 0, mod.ACT_RELU, "input", "conv1")
        net.batchnorm("conv1", "bn1")
        net.maxpool(2, 2, mod.PADDING_SAME, "bn1", "pool1")
        net.conv(32, 3, 1, 1, 1, 0, mod.ACT_RELU, "pool1", "conv2")
        net.batchnorm("conv2", "bn2")
        net.maxpool(2, 2, mod.PADDING_SAME, "bn2", "pool2")
        net.fullc(256, mod.ACT_RELU, "pool2", "fc1")
        net.batchnorm("fc1", "bn3")
        net.fullc(10, mod.ACT_RELU, "bn3", "fc2")
        net.softmax("fc2", "softmax")
        net.cost("softmax", "label", "cost", 1.0)
        L = net.L
        L.bcnn_set_sgd_optimizer.argtypes = [C.c_void_p, C.c_float, C.c_float]
        L.bcnn_set_learning_rate_policy.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]
        L.bcnn_set_weight_regularizer.argtypes = [C.c_void_p, C.c_float]
        L.bcnn_set_sgd_optimizer(net.net, 0.003, 0.9)
        L.bcnn_set_learning_rate_policy(net.net, 5, 0.00002, 0.0, 0.0, 50000, 40000)
        L.bcnn_set_weight_regularizer(net.net, 0.0005)
        assert _set_loader(net, 0, tr[0], tr[1], te[0], te[1]) == 0
        _augment(net, shift=(5, 5), rotation=30.0)
        if mod is capi:
            assert net.set_loader_on_device(True) == 0
        net.compile()
        nets.append(net)
    losses = []
    for net in nets:
        libc.srand(7)
        net.L.bcnn_train_on_batch.argtypes = [C.c_void_p]
        net.L.bcnn_train_on_batch.restype = C.c_float
        losses.append([net.L.bcnn_train_on_batch(net.net) for _ in range(6)])
    nets[1].download(0, False)
    assert np.array_equal(nets[0].data(0), nets[1].data(0))          # both saw the same sixth batch
    a, b = np.array(losses[0]), np.array(losses[1])
    assert np.all(np.isfinite(b)) and np.abs(a - b).max() <= 1e-3 * np.abs(a).max(), (a, b)
    _close(nets)


def test_statuses():
    from bcnn_amd import capi
    L = capi.lib()
    assert L.bcnn_set_loader_on_device(None, 1) == 1       # BCNN_INVALID_PARAMETER
    assert L.bcnn_get_loader_on_device(None) == 0
    net = _graph(capi.Net(mode=TRAIN, w=8, h=8, c=3, n=2), capi, 4)
    assert net.set_loader_on_device(True) == 0             # no loader: accepted ...
    net.compile()
    x = np.random.RandomState(0).uniform(-1, 1, net.data(0).shape).astype(np.float32)
    y = np.random.RandomState(1).uniform(0, 1, net.data(1).shape).astype(np.float32)
    net.data(0)[...] = x
    net.data(1)[...] = y
    L.bcnn_loader_next.argtypes = [C.c_void_p]
    assert L.bcnn_loader_next(net.net) == 0                # ... and bcnn_loader_next still only uploads the caller's values
    net.data(0)[...] = 0
    net.data(1)[...] = 0
    net.download(0, False)
    net.download(1, False)
    assert np.array_equal(net.data(0), x) and np.array_equal(net.data(1), y)
    net.close()
