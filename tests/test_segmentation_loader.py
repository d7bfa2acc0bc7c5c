"""GPU: the segmentation-list loader (BCNN_LOAD_SEGMENTATION_LIST, bcnn_amd/host/bcnn_data_segmentation.c) through the
public API. Six image / mask pairs (20 x 18 RGB images, palette-PNG masks of three classes and a 255 border) feed a
16 x 12 conv -> softmax-loss net in batches of 4. The label tensor of every batch is held to the numpy restatement of the
warp rule (tests/_label_warp_ref.py) applied to the cropped masks with the draws replayed from the seed; the input tensor
to what the classification list makes of the same image files; the host route and the device route to each other, bit for
bit. Then: skipped lines, VALID and PREDICT mode, the refusals, the fill byte, and three training steps fed by the loader
against three fed by hand."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

from tests import _label_cases as LC
from tests import _label_warp_ref as ref
from tests.test_data_loader import _augment, _next, _set_loader, libc

pytestmark = pytest.mark.gpu

W, H, N = 16, 12, 4          # net input and batch
WI, HI = 20, 18              # the files
PAIRS = 6
SEG, CLASSIF = 6, 2
TRAIN, VALID, PREDICT = 1, 2, 0
RAND_MAX_F = np.float32(2147483647)      # (float)RAND_MAX
AUG = dict(shift=(6, 4), scale=(0.8, 1.3), rotation=20.0, flip=(1, 0))

CFG = """
[net]
input_width=%d
input_height=%d
input_channels=3
batch_size=%d
%s
[conv]
filters=3
size=3
stride=%d
pad=1
activation=linear
src=input
dst=c1

[softmax_loss]
ignore_label=%d
src=c1
dst=prob
"""


def _net(tmp_path, keys="flip_h=1\n", device=False, ignore=255, stride=1, mode=TRAIN, w=W, h=H):
    from bcnn_amd import capi
    cfg = tmp_path / "seg.cfg"
    cfg.write_text(CFG % (w, h, N, keys, stride, ignore))
    net = capi.Net.load_net(str(cfg), None, mode=mode)
    assert net.set_loader_on_device(device) == 0
    net.compile()                                           # the input tensor gets its buffers here
    return net


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the pairs, their lists, and the class maps as arrays"""
    d = tmp_path_factory.mktemp("seg")
    rs = np.random.RandomState(17)
    pal = rs.randint(0, 256, (256, 3)).astype(np.uint8)
    images, masks, lines, img_lines = [], [], [], []
    for k in range(PAIRS):
        img = rs.randint(0, 256, (HI, WI, 3)).astype(np.uint8)
        m = rs.randint(0, 3, (HI, WI)).astype(np.uint8)
        m[0, :] = m[-1, :] = 255
        m[:, 0] = m[:, -1] = 255
        pi, pm = d / ("img%d.png" % k), d / ("mask%d.png" % k)
        Image.fromarray(img, "RGB").save(pi)
        pim = Image.fromarray(m, "P")
        pim.putpalette(pal.reshape(-1).tolist())
        pim.save(pm)
        images.append(img)
        masks.append(m)
        lines.append("%s %s" % (pi, pm))
        img_lines.append("%s %d" % (pi, k % 3))
    out = dict(dir=d, images=images, masks=masks, lines=lines)
    for name, rows in (("seg.txt", lines), ("classif.txt", img_lines), ("predict.txt", [l.split()[0] for l in lines])):
        (d / name).write_text("\n".join(rows) + "\n")
        out[name] = str(d / name)
    # the bad lines: a missing mask, a mask of other extents, an RGB mask
    Image.fromarray(np.zeros((10, 10), np.uint8), "L").save(d / "small_mask.png")
    Image.fromarray(np.zeros((HI, WI, 3), np.uint8), "RGB").save(d / "rgb_mask.png")
    first = lines[0].split()[0]
    bad = ["%s %s" % (first, d / "nowhere.png"), "%s %s" % (first, d / "small_mask.png"), "%s %s" % (first, d / "rgb_mask.png")]
    (d / "dirty.txt").write_text("\n".join(lines[:2] + bad + lines[2:]) + "\n")
    out["dirty.txt"] = str(d / "dirty.txt")
    return out


# ---- the draws of one sample, replayed from libc rand() with the loader's float arithmetic ---------------------------
def _f(x):
    return np.float32(x)


def _rand_between(lo, hi):
    return int(_f(_f(_f(_f(libc.rand()) / RAND_MAX_F) * _f(hi - lo)) + _f(lo)) + _f(0.5))


def _rand_centred(rng):
    return _f(_f(_f(libc.rand() - 2147483647 // 2) / RAND_MAX_F) * _f(rng))


def _rand_span(a, b):
    return _f(_f(_f(_f(libc.rand()) / RAND_MAX_F) * _f(_f(b) - _f(a))) + _f(a))


def _replay(batches):
    """(crop x, crop y, record, taps) per sample, consuming rand() as a TRAIN batch of the loader does"""
    out = []
    for _ in range(batches * N):
        x0, y0 = _rand_between(0, WI - W), _rand_between(0, HI - H)
        sx, sy = int(_rand_centred(AUG["shift"][0])), int(_rand_centred(AUG["shift"][1]))
        scale = _rand_span(*AUG["scale"])
        theta = _f(_rand_centred(AUG["rotation"]) * _f(0.01745329252))
        rec, taps = LC.loader_record(W, H, flip=True, shift=(sx, sy), scale=float(scale), theta=float(theta))
        out.append((x0, y0, rec, taps))
    return out


def _play(net, batches, seed, device):
    """input and label of `batches` batches as the DEVICE holds them, the route counter, and the next rand()"""
    libc.srand(seed)
    out = []
    for _ in range(batches):
        _next(net)
        net.download(0, False)
        net.download(1, False)
        out.append((net.data(0).copy(), net.data(1).copy(), net.loader_device_labels()))
    return out, libc.rand()


def _seg_net(tmp_path, files, device, lst="seg.txt", **kw):
    net = _net(tmp_path, device=device, **kw)
    assert net.set_data_loader(SEG, files[lst], None, files[lst], None) == 0
    _augment(net, **AUG)
    return net


@pytest.fixture(scope="module")
def runs(tmp_path_factory, files):
    """three TRAIN batches on the host route and on the device route, computed once"""
    tmp = tmp_path_factory.mktemp("runs")
    got = {}
    for device in (False, True):
        net = _seg_net(tmp, files, device)
        got[device] = _play(net, 3, seed=31, device=device)
        net.close()
    return got


def test_labels_equal_the_restatement_on_both_routes(files, runs):
    libc.srand(31)
    draws = _replay(3)
    nxt = libc.rand()
    stages = set()
    for device in (False, True):
        batches, after = runs[device]
        assert after == nxt, "the loader drew another number of rand() values than the classification list's rule"
        for b, (_, lab, _) in enumerate(batches):
            assert lab.shape == (N, 1, H, W)
            for i in range(N):
                k = b * N + i
                x0, y0, rec, taps = draws[k]
                crop = files["masks"][k % PAIRS][y0:y0 + H, x0:x0 + W]
                want = ref.warp(crop, rec, taps, 255).astype(np.float32)
                assert np.array_equal(lab[i, 0], want), (device, b, i, int((lab[i, 0] != want).sum()))
                stages.add(int(rec[0]) & 15)
    assert stages == {15}                                   # flip, shift, scale and rotation on every sample
    labs = np.concatenate([lab for _, lab, _ in runs[True][0]])
    assert set(np.unique(labs)) <= {0.0, 1.0, 2.0, 255.0} and (labs == 255).any() and (labs < 3).mean() > 0.3


def test_the_two_routes_are_bit_identical_and_count_their_labels(runs):
    for (xh, yh, nh), (xd, yd, nd) in zip(runs[False][0], runs[True][0]):
        assert np.array_equal(xh.view(np.uint32), xd.view(np.uint32))
        assert np.array_equal(yh.view(np.uint32), yd.view(np.uint32))
        assert nh == 0 and nd == N
    assert len({x.tobytes() for x, _, _ in runs[True][0]}) == 3


def test_input_equals_the_classification_list(tmp_path, files, runs):
    for device in (False, True):
        twin = _net(tmp_path, device=device)
        assert twin.set_data_loader(CLASSIF, files["classif.txt"], None, files["classif.txt"], None) == 0
        _augment(twin, **AUG)
        got, after = _play(twin, 3, seed=31, device=device)
        assert after == runs[device][1]
        for (xa, _, _), (xb, _, nlab) in zip(runs[device][0], got):
            assert np.array_equal(xa.view(np.uint32), xb.view(np.uint32))
            assert nlab == 0                                # the counter is 0 for every other loader type
        twin.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_skipped_lines_consume_no_draw(tmp_path, files, runs, device):
    net = _seg_net(tmp_path, files, device, lst="dirty.txt")
    got, after = _play(net, 3, seed=31, device=device)
    assert after == runs[device][1]                         # rand() was consumed as if the three lines were absent
    for (xa, ya, na), (xb, yb, nb) in zip(runs[device][0], got):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb) and na == nb
    net.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_valid_mode_is_centre_crop_and_identity(tmp_path, files, device):
    net = _seg_net(tmp_path, files, device)
    net.set_mode(VALID)
    libc.srand(5)
    first = libc.rand()
    libc.srand(5)
    x0, y0 = (WI - W) // 2, (HI - H) // 2
    for b in range(2):
        _next(net)
        net.download(0, False)
        net.download(1, False)
        x, lab = net.data(0), net.data(1)
        for i in range(N):
            k = (b * N + i) % PAIRS
            assert np.array_equal(lab[i, 0], files["masks"][k][y0:y0 + H, x0:x0 + W].astype(np.float32)), (b, i)
            img = files["images"][k][y0:y0 + H, x0:x0 + W].astype(np.float32).transpose(2, 0, 1)
            assert np.array_equal(x[i], (img - np.float32(127.5)) * np.float32(1 / 127.5)), (b, i)
        assert net.loader_device_labels() == (N if device else 0)
    assert libc.rand() == first                             # nothing is drawn outside TRAIN mode
    net.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_predict_mode_reads_no_mask_and_leaves_the_label_alone(tmp_path, files, device):
    net = _seg_net(tmp_path, files, device)
    assert net.set_data_loader(SEG, files["seg.txt"], None, files["predict.txt"], None) == 0
    net.set_mode(PREDICT)
    net.data(1)[...] = -3.0
    net.upload(1)
    _next(net)
    net.download(0, False)
    net.download(1, False)
    assert np.all(net.data(1) == -3.0) and net.loader_device_labels() == 0
    x0, y0 = (WI - W) // 2, (HI - H) // 2
    img = files["images"][1][y0:y0 + H, x0:x0 + W].astype(np.float32).transpose(2, 0, 1)
    assert np.array_equal(net.data(0)[1], (img - np.float32(127.5)) * np.float32(1 / 127.5))
    net.close()


def test_label_extents_other_than_the_input_are_refused(tmp_path, files):
    net = _net(tmp_path, stride=2)                          # the label map is [4][1][6][8]
    assert net.shape(1) == (N, 1, H // 2, W // 2)
    assert net.set_data_loader(SEG, files["seg.txt"], None, None, None) == 0
    libc.srand(3)
    first = libc.rand()
    libc.srand(3)
    assert net.loader_next() == 1                           # BCNN_INVALID_PARAMETER
    assert libc.rand() == first
    net.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_distortion_is_refused_before_any_draw_and_spotlights_are_not(tmp_path, files, device):
    net = _net(tmp_path, keys="max_distortion=0.3\nmax_spots=2\nrange_shift_x=4\n", device=device)
    assert net.set_data_loader(SEG, files["seg.txt"], None, None, None) == 0
    libc.srand(3)
    first = libc.rand()
    libc.srand(3)
    assert net.loader_next() == 0                           # effects off: the draws are made and dropped, as ever
    assert net.set_loader_effects(True) == 0
    libc.srand(3)
    assert net.loader_next() == 1                           # BCNN_INVALID_PARAMETER ...
    assert libc.rand() == first                             # ... before any draw: rand() continues where it was
    net.close()
    net = _net(tmp_path, keys="max_spots=2\nrange_shift_x=4\n", device=device)
    assert net.set_data_loader(SEG, files["seg.txt"], None, None, None) == 0
    assert net.set_loader_effects(True) == 0
    assert net.loader_next() == 0                           # spotlights are photometric: allowed
    net.download(1, False)
    assert net.loader_device_labels() == (N if device else 0)
    assert set(np.unique(net.data(1))) <= {0.0, 1.0, 2.0, 255.0}
    net.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("ignore,fill", [(-1, 255), (7, 7), (300, 255)])
def test_the_fill_byte_outside_a_file_smaller_than_the_input(tmp_path, files, device, ignore, fill):
    w, h = WI + 4, HI + 2                                   # the input is larger than every file
    net = _net(tmp_path, keys="", device=device, ignore=ignore, w=w, h=h)
    assert net.set_data_loader(SEG, files["seg.txt"], None, None, None) == 0
    _next(net)                                              # TRAIN mode, no augmentation, no draw for a smaller file: origin (0, 0)
    net.download(0, False)
    net.download(1, False)
    lab, x = net.data(1), net.data(0)
    for i in range(N):
        want = np.full((h, w), fill, np.float32)
        want[:HI, :WI] = files["masks"][i]
        assert np.array_equal(lab[i, 0], want), (i, ignore)
        zero = (np.float32(0) - np.float32(127.5)) * np.float32(1 / 127.5)                 # the image gets 0
        assert np.all(x[i, :, HI:, :] == zero) and np.all(x[i, :, :, WI:] == zero)
    net.close()


def _weights(net):
    return [net.node_src(0, 1), net.node_src(0, 2)]


def test_three_steps_from_the_loader_equal_three_steps_fed_by_hand(tmp_path, files):
    """no threshold: net A is stepped from the loader on the device route, net B (the same weights) from A's downloaded
    input and label through bcnn_upload_tensor; the statistics record and the loss of every step are equal bit for bit"""
    a = _seg_net(tmp_path, files, True)
    b = _net(tmp_path)
    for net in (a, b):
        net.set_sgd(0.1, 0.9, 0.0)
    for i in _weights(a):
        a.download(i, False)
        b.data(i)[...] = a.data(i)
        b.upload(i)
    libc.srand(77)
    for step in range(3):
        assert a.loader_next() == 0 and a.loader_device_labels() == N
        a.download(0, False)
        a.download(1, False)
        b.data(0)[...] = a.data(0)
        b.data(1)[...] = a.data(1)
        b.upload(0)
        b.upload(1)
        stats = []
        for net in (a, b):
            net.forward()
            net.backward()
            stats.append(net.softmax_loss_stats(1))
            net.update()
            net.sync()
        assert stats[0]["valid"] > 0 and stats[0]["ignored"] > 0 and stats[0]["out_of_range"] == 0, stats[0]
        for key in stats[0]:
            assert stats[0][key] == stats[1][key], (step, key, stats[0][key], stats[1][key])   # no NaN: == is bit equality
    for i in _weights(a):
        a.download(i, False)
        b.download(i, False)
        assert np.array_equal(a.data(i).view(np.uint32), b.data(i).view(np.uint32))
    a.close()
    b.close()
