"""bcnn_set_loader_detection_on_device: a BCNN_LOAD_DETECTION_LIST batch that is resized, pasted
on its grey canvas, augmented and converted on the device against the host path of this build and, where the reference's
integer aspect ratio is the true one, against the unmodified reference -- inputs, labels and the state of rand(), byte
for byte. Tensor 0 is read after download(0, False): the device path does not write the host copy. The entry behind it
(bcnn_hip_augment_letterbox_batch) is also driven alone through ops.py against bip_resize_bilinear + paste +
bcnn_convert_img_to_float composed here, and, for the records, against bcnn_hip_augment_batch on the composed canvases
(tests/test_loader_device.py pins that entry to the host loader)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import ref_bind as rb
from tests.test_detection_loader import CONFIG, MAX_BOXES, N, _boxes, _dataset, _nets, _set_loader, libc

pytestmark = pytest.mark.gpu

CONFIG_GREY = CONFIG.replace("input_channels=3", "input_channels=1")
CONFIG_ODD = (CONFIG.replace("input_width=16", "input_width=19").replace("input_height=16", "input_height=13")
              .replace("train_detector=1\n", "train_detector=1\nrange_shift_x=4\nrange_shift_y=3\nmin_scale=0.8\nmax_scale=1.2\n"
                                             "rotation_range=20\nswap_to_bgr=1\n"))
INVALID_DATA = 2
u8p = C.POINTER(C.c_uint8)


def _net(tmp, text, mode, device, name="det"):
    from bcnn_amd import capi
    cfg = tmp / (name + ".cfg")
    cfg.write_text(text)
    libc.srand(5)
    net = capi.Net.load_net(str(cfg), None, mode=mode)
    if device:
        assert net.set_loader_on_device(True) == 0 and net.set_loader_detection_on_device(True) == 0
    return net


def _next(net):
    net.L.bcnn_loader_next.argtypes = [C.c_void_p]
    net.L.bcnn_loader_next.restype = C.c_int
    assert net.L.bcnn_loader_next(net.net) == 0
    if not isinstance(net, rb.RefNet):
        net.download(0, False)
    return net.data(0).copy(), (net.data(1).copy() if net.tensor(1).data else None)


def _play(net, batches, seed, counters=None):
    """`batches` batches from srand(seed): ([(input, labels)], the next rand()); counters = (letterboxed, decoded) after
    every batch"""
    libc.srand(seed)
    out = []
    for _ in range(batches):
        out.append(_next(net))
        if counters is not None:
            assert (net.loader_device_letterboxed(), net.loader_device_decoded()) == counters
    return out, libc.rand()


def _assert_same(a, b, what):
    (xa, ra), (xb, rb_) = a, b
    assert len(xa) == len(xb)
    for k, ((ia, la), (ib, lb)) in enumerate(zip(xa, xb)):
        assert np.array_equal(ia, ib), (what, "input", k)
        assert (la is None and lb is None) or np.array_equal(la, lb), (what, "label", k)
    assert ra == rb_, (what, "rand")


def _close(nets):
    for net in nets:
        net.close()


def _write_pnm(path, img):
    """P6 for h x w x 3, P5 for h x w"""
    with open(path, "wb") as f:
        f.write(b"P%d\n%d %d\n255\n" % (6 if img.ndim == 3 else 5, img.shape[1], img.shape[0]) + img.tobytes())


MIXED = [(15, 20), (20, 15), (9, 1), (1, 17), (1, 9), (1, 16), (1, 20), (12, 12), (30, 40)]
# every letterbox fits the 19 x 13 canvas: wider than 19:13, or portrait (the loader's extent formula is the square
# input's: a 4:3 image comes out 19 x 14 there, is cropped by the host path's paste, and its batch stays on the host)
WIDE = [(10, 20), (20, 15), (9, 1), (1, 17), (1, 9), (8, 16), (1, 20), (3, 6), (20, 40), (5, 19)]


def _mixed_list(tmp, rs, channels, shapes=MIXED):
    """4:3 and 3:4 images, one-sample axes, an extent that resizes to one row, two that resize to none (17 x 1 on the 16
    wide input, 20 x 1 on the 19 wide one: skipped) and a file of the other channel count (skipped)"""
    lines = []
    for k, (h, w) in enumerate(shapes):
        img = rs.randint(0, 256, (h, w, 3) if channels == 3 else (h, w)).astype(np.uint8)
        p = str(tmp / ("m%d.pnm" % k))
        _write_pnm(p, img)
        lines.append("%s %s" % (p, _boxes(rs, 1 + k % 3)))
    other = str(tmp / "other.pnm")
    _write_pnm(other, rs.randint(0, 256, (16, 16) if channels == 3 else (16, 16, 3)).astype(np.uint8))
    lines.insert(2, "%s %s" % (other, _boxes(rs, 2)))
    lst = tmp / "mixed.txt"
    lst.write_text("\n".join(lines) + "\n")
    return str(lst)


# ---- 1. against the unmodified reference ---------------------------------------------------------------------------------
def test_three_ways_match_the_reference(tmp_path):
    from bcnn_amd import capi
    rs = np.random.RandomState(31)
    lst, _ = _dataset(tmp_path, [(16, 16), (8, 8), (40, 40), (16, 32), (3, 6)], rs)   # + 60 boxes, a malformed row, a missing file
    ref, host = _nets(tmp_path, rb.MODE_TRAIN)
    dev = _net(tmp_path, CONFIG, capi.MODE_TRAIN, True, "dev")
    nets = (ref, host, dev)
    for net in nets:
        assert _set_loader(net, lst, lst) == 0
        net.compile()
    assert dev.get_loader_detection_on_device() == 1 and host.get_loader_detection_on_device() == 0
    train = [_play(ref, 3, 77), _play(host, 3, 77, (0, 0)), _play(dev, 3, 77, (N, 0))]   # 12 samples over 6 readable rows: wraps
    for net in nets:
        assert net.L.bcnn_set_mode(net.net, rb.MODE_VALID) == 0
    valid = [_play(ref, 1, 78), _play(host, 1, 78, (0, 0)), _play(dev, 1, 78, (N, 0))]
    for runs in (train, valid):
        _assert_same(runs[0], runs[1], "host against reference")
        _assert_same(runs[0], runs[2], "device against reference")
    assert len({x.tobytes() for x, _ in train[2][0]}) == 3
    assert train[2][0][0][1].shape == (N, 1, 1, 5 * MAX_BOXES)
    ref.close()
    _close((host, dev))


# ---- 2. against this build's host path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,text,channels,shapes", [
    pytest.param(*p, id=p[0]) for p in (("colour", CONFIG, 3, MIXED), ("grey", CONFIG_GREY, 1, MIXED),
                                        ("odd_every_stage", CONFIG_ODD, 3, WIDE),
                                        ("odd_every_stage_cropped", CONFIG_ODD, 3, MIXED))])
def test_device_path_matches_host_path(tmp_path, name, text, channels, shapes):
    from bcnn_amd import capi
    lst = _mixed_list(tmp_path, np.random.RandomState(4), channels, shapes)
    host, dev = _net(tmp_path, text, capi.MODE_TRAIN, False, "host"), _net(tmp_path, text, capi.MODE_TRAIN, True, "dev")
    for net in (host, dev):
        assert _set_loader(net, lst, lst) == 0
        net.compile()
    # a batch with an image whose letterbox is taller than the canvas is refused by the entry and made on the host from
    # the decoded images and the draws already made: same bytes, counter 0
    on_device = None if name.endswith("cropped") else (N, 0)
    a, b = _play(host, 3, 11, (0, 0)), _play(dev, 3, 11, on_device)
    _assert_same(a, b, name + " train")
    assert len({x.tobytes() for x, _ in b[0]}) == 3
    for net in (host, dev):
        assert net.set_mode(capi.MODE_VALID) == 0
    _assert_same(_play(host, 2, 12, (0, 0)), _play(dev, 2, 12, on_device), name + " valid")
    if on_device is None:
        assert dev.loader_device_letterboxed() in (0, N) and dev.loader_device_decoded() == 0
    _close((host, dev))


# ---- 3. toggling -------------------------------------------------------------------------------------------------------------
def test_toggling_between_batches(tmp_path):
    from bcnn_amd import capi
    lst, _ = _dataset(tmp_path, [(24, 24), (15, 20), (8, 8), (20, 15), (16, 16)], np.random.RandomState(8))
    plain, toggled = _net(tmp_path, CONFIG, capi.MODE_TRAIN, False, "plain"), _net(tmp_path, CONFIG, capi.MODE_TRAIN, True, "tog")
    for net in (plain, toggled):
        assert _set_loader(net, lst, lst) == 0
        net.compile()
    want = _play(plain, 6, 21, (0, 0))
    libc.srand(21)
    got = []
    for k in range(6):
        assert toggled.set_loader_detection_on_device(k % 2 == 0) == 0
        got.append(_next(toggled))
        assert toggled.loader_device_letterboxed() == (N if k % 2 == 0 else 0)
    _assert_same(want, (got, libc.rand()), "toggled")
    # the older switch alone never moves this loader
    assert toggled.set_loader_detection_on_device(False) == 0 and toggled.set_loader_decode_on_device(True) == 0
    _next(toggled)
    assert toggled.loader_device_letterboxed() == 0 and toggled.loader_device_decoded() == 0
    # and the new one does nothing without it
    assert toggled.set_loader_detection_on_device(True) == 0 and toggled.set_loader_on_device(False) == 0
    _next(toggled)
    assert toggled.loader_device_letterboxed() == 0
    _close((plain, toggled))


# ---- 4. PREDICT mode -----------------------------------------------------------------------------------------------------------
def test_predict_mode_leaves_the_labels_alone(tmp_path):
    from bcnn_amd import capi
    lst, _ = _dataset(tmp_path, [(24, 24), (15, 20), (8, 8), (20, 15), (16, 16)], np.random.RandomState(9))
    host, dev = _net(tmp_path, CONFIG, capi.MODE_PREDICT, False, "host"), _net(tmp_path, CONFIG, capi.MODE_PREDICT, True, "dev")
    for net in (host, dev):
        assert _set_loader(net, lst, lst) == 0
        net.compile()
        if net.tensor(1).data:
            net.data(1)[...] = -7.0
    a, b = _play(host, 2, 3, (0, 0)), _play(dev, 2, 3, (N, 0))
    _assert_same(a, b, "predict")
    for _, lab in b[0]:
        assert lab is None or np.all(lab == -7.0)
    _close((host, dev))


# ---- 5. threads ------------------------------------------------------------------------------------------------------------------
def test_batches_do_not_depend_on_the_thread_count(tmp_path):
    from bcnn_amd import capi
    lst, _ = _dataset(tmp_path, [(24, 24), (15, 20), (8, 8), (20, 15), (16, 16)], np.random.RandomState(10))
    runs = []
    for threads in (1, 3, 8):
        net = _net(tmp_path, CONFIG, capi.MODE_TRAIN, True, "t%d" % threads)
        assert net.set_num_threads(threads) == 0
        assert _set_loader(net, lst, lst) == 0
        net.compile()
        runs.append(_play(net, 3, 5, (N, 0)))
        net.close()
    _assert_same(runs[0], runs[1], "3 threads")
    _assert_same(runs[0], runs[2], "8 threads")


def test_a_list_of_failures_gives_up_after_1000(tmp_path):
    from bcnn_amd import capi
    lst = tmp_path / "bad.txt"
    lst.write_text("".join("%s 0 0.5 0.5 0.2 0.2\n" % str(tmp_path / ("none%d.ppm" % k)) for k in range(3)) +
                   "%s 0 0.5\n" % str(tmp_path / "none0.ppm"))
    rands = []
    for device, threads in ((False, 1), (True, 1), (True, 3)):
        net = _net(tmp_path, CONFIG, capi.MODE_TRAIN, device, "bad")
        assert net.set_num_threads(threads) == 0
        assert _set_loader(net, str(lst), str(lst)) == 0
        net.compile()
        libc.srand(13)
        net.L.bcnn_loader_next.restype = C.c_int
        assert net.L.bcnn_loader_next(net.net) == INVALID_DATA
        assert net.loader_device_letterboxed() == 0
        rands.append(libc.rand())
        net.close()
    assert rands[0] == rands[1] == rands[2]      # a skipped entry consumes no draw


# ---- 6. the entry alone ------------------------------------------------------------------------------------------------------------
_host = {}


def _host_fns():
    if not _host:
        from bcnn_amd import _lib, capi
        capi.lib()
        bip = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libbip.so"))
        bip.bip_resize_bilinear.argtypes = [u8p] + [C.c_size_t] * 3 + [u8p] + [C.c_size_t] * 4
        bip.bip_resize_bilinear.restype = C.c_int
        L = C.CDLL(capi.LIB_PATH)
        L.bcnn_convert_img_to_float.argtypes = [u8p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float,
                                                C.c_float, C.POINTER(C.c_float)]
        L.bcnn_convert_img_to_float.restype = None
        _host.update(resize=bip.bip_resize_bilinear, convert=L.bcnn_convert_img_to_float, hip=_lib.load())
    return _host


def _canvas(img, box, W, H):
    """bip_resize_bilinear, memset to 128, paste at (x_off, y_off)"""
    h, w, c = img.shape
    nw, nh, xo, yo = box
    tmp = np.zeros((nh, nw, c), np.uint8)
    assert _host_fns()["resize"](img.ctypes.data_as(u8p), w, h, w * c, tmp.ctypes.data_as(u8p), nw, nh, nw * c, c) == 0
    canvas = np.full((H, W, c), 128, np.uint8)
    canvas[yo:yo + nh, xo:xo + nw] = tmp
    return canvas


def _converted(canvas, swap):
    H, W, c = canvas.shape
    out = np.empty((c, H, W), np.float32)
    _host_fns()["convert"](canvas.ctypes.data_as(u8p), W, H, c, 1 / 127.5, 1 if swap else 0, 127.5, 127.5, 127.5,
                           out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def _case(rs, c, W, H, num):
    """random sources of 1 .. 40 pixels a side; the first boxes pin the ends of every range"""
    pinned = [(1, 1, 0, 0), (W, H, 0, 0), (1, H, W - 1, 0), (W, 1, 0, H - 1), (1, 1, W - 1, H - 1)]
    images, boxes = [], []
    for b in range(num):
        w, h = (1, 1) if b == 0 else (1, 7) if b == 1 else (9, 1) if b == 2 else tuple(rs.randint(1, 41, 2))
        images.append(rs.randint(0, 256, (h, w, c)).astype(np.uint8))
        if b < len(pinned):
            boxes.append(pinned[b])
        else:
            nw, nh = rs.randint(1, W + 1), rs.randint(1, H + 1)
            boxes.append((nw, nh, rs.randint(0, W - nw + 1), rs.randint(0, H - nh + 1)))
    return images, boxes


def _records(rs, num, W, H, flags):
    """records with the stages of `flags`, and tap tables any of which is legal input (index -1 .. extent - 2)"""
    rec = np.zeros((num, 8), np.int32)
    rec[:, 0] = flags
    if flags & 2:
        rec[:, 1], rec[:, 2] = rs.randint(-W, W + 1, num), rs.randint(-H, H + 1, num)
    if flags & 8:
        theta = rs.uniform(-0.4, 0.4, num)
        rec[:, 3], rec[:, 4] = (np.cos(theta) * 65536).astype(np.int32), (np.sin(theta) * 65536).astype(np.int32)
    if flags & 16:
        rec[:, 5] = (rs.uniform(0.7, 1.3, num) * 4096 + 0.5).astype(np.int32)
    rec[:, 6] = rs.randint(-30, 31, num) if flags else 0
    taps = np.zeros((num, W + H, 2), np.int32)
    taps[:, :W, 0] = rs.randint(-1, max(W - 2, 0) + 1, (num, W))
    taps[:, W:, 0] = rs.randint(-1, max(H - 2, 0) + 1, (num, H))
    taps[..., 1] = rs.randint(0, 17, (num, W + H))
    return rec, taps


def _augment_batch(canvases, rec, taps, swap, n):
    """bcnn_hip_augment_batch on dense canvases: the reference of every stage behind the canvas"""
    num, H, W, c = canvases.shape
    dst = torch.full((n, c, H, W), -9.0, device="cuda")
    assert _host_fns()["hip"].bcnn_hip_augment_batch(dst.data_ptr(), n, c, H, W, num, W, H, canvases.ctypes.data, rec.ctypes.data,
                                                     taps.ctypes.data, 1 if swap else 0) == 0
    return dst.cpu().numpy()


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_entry_alone(c):
    from bcnn_amd import ops
    rs = np.random.RandomState(100 + c)
    for W, H in ((19, 13), (16, 16), (5, 3), (64, 9)):      # rows of 19 c bytes end inside a chunk; 16 c and 64 c on it
        n, num = 9, 7
        images, boxes = _case(rs, c, W, H, num)
        canvases = np.stack([_canvas(im, bx, W, H) for im, bx in zip(images, boxes)])
        # identity records: the composition of the issue
        for swap in (False, True):
            dst = torch.full((n, c, H, W), -9.0, device="cuda")
            assert ops.augment_letterbox_batch(dst, images, boxes, swap_to_bgr=swap) == 0
            got = dst.cpu().numpy()
            for b in range(num):
                assert np.array_equal(got[b], _converted(canvases[b], swap)), (W, H, b, swap)
            assert np.all(got[num:] == -9.0)                 # num_samples < n: the other planes keep the sentinel
        # each stage alone, then all together
        for flags in (1, 2, 4, 8, 16, 0, 31):
            rec, taps = _records(rs, num, W, H, flags)
            dst = torch.full((n, c, H, W), -9.0, device="cuda")
            assert ops.augment_letterbox_batch(dst, images, boxes, rec, taps, swap_to_bgr=True) == 0
            got = dst.cpu().numpy()
            assert np.array_equal(got, _augment_batch(canvases, rec, taps, True, n)), (W, H, flags)


def test_entry_refusals():
    from bcnn_amd import ops
    hip = _host_fns()["hip"]
    rs = np.random.RandomState(7)
    W, H, c, n = 12, 10, 3, 4
    images = [rs.randint(0, 256, (6, 8, c)).astype(np.uint8) for _ in range(3)]
    good = [(12, 9, 0, 1), (6, 10, 3, 0), (12, 10, 0, 0)]
    dst = torch.full((n, c, H, W), -9.0, device="cuda")
    assert ops.augment_letterbox_batch(dst, images, good) == 0
    torch.cuda.synchronize()
    dst.fill_(-9.0)

    def refused(boxes=good, records=None, taps=None, num=None, imgs=images):
        assert ops.augment_letterbox_batch(dst, imgs, boxes, records, taps, num_samples=num) == 1
    for bad in ((0, 9, 0, 0), (13, 9, 0, 0), (12, 0, 0, 0), (12, 11, 0, 0), (12, 9, 1, 0), (12, 9, -1, 0), (12, 9, 0, 2),
                (12, 9, 0, -1), (6, 10, 7, 0)):
        refused([bad] + good[1:])
    refused(num=0)
    refused(num=n + 1, imgs=images + images, boxes=good + good)
    scale = np.zeros((3, 8), np.int32)
    scale[1, 0] = 4
    refused(records=scale)                                   # SCALE and no taps
    taps = np.zeros((3, W + H, 2), np.int32)
    taps[1, W - 1, 0] = W - 1
    refused(records=scale, taps=taps)                        # a tap whose neighbour is outside
    taps[1, W - 1, 0] = -2
    refused(records=scale, taps=taps)
    # NULL arguments, extents and channel counts through the raw entry
    arr = (ops.LetterboxImage * 3)(*[ops.LetterboxImage(im.ctypes.data, 8, 6, *bx) for im, bx in zip(images, good)])
    rec = np.zeros((3, 8), np.int32)
    ok = [dst.data_ptr(), n, c, H, W, 3, C.cast(arr, C.c_void_p), rec.ctypes.data, None, 0]
    for at, value in ((0, None), (6, None), (7, None), (1, 0), (2, 0), (2, 5), (3, 0), (4, 0), (5, 0), (5, n + 1)):
        args = list(ok)
        args[at] = value
        assert hip.bcnn_hip_augment_letterbox_batch(*args) == 1, (at, value)
    for field, value in (("pixels", None), ("w", 0), ("h", 0), ("h", -1)):
        arr2 = (ops.LetterboxImage * 3)(*[ops.LetterboxImage(im.ctypes.data, 8, 6, *bx) for im, bx in zip(images, good)])
        setattr(arr2[2], field, value)
        args = list(ok)
        args[6] = C.cast(arr2, C.c_void_p)
        assert hip.bcnn_hip_augment_letterbox_batch(*args) == 1, (field, value)
    # above 2 GiB for the block plus the device part: 8 canvases of 6000 x 6000 x 4 and as many rotated samples are
    # 2.3e9 bytes, while 8 x 6000 x 6000 x 4 alone is in range (no tensor of that size is needed: refused before any write)
    imgs4 = [rs.randint(0, 256, (6, 8, 4)).astype(np.uint8) for _ in range(8)]
    arr8 = (ops.LetterboxImage * 8)(*[ops.LetterboxImage(im.ctypes.data, 8, 6, *good[k % 3]) for k, im in enumerate(imgs4)])
    rec8 = np.zeros((8, 8), np.int32)
    assert 2 * 8 * 6000 * 6000 * 4 > 0x7fffffff >= 8 * 6000 * 6000 * 4
    assert hip.bcnn_hip_augment_letterbox_batch(dst.data_ptr(), 16, 4, 6000, 6000, 8, C.cast(arr8, C.c_void_p),
                                                rec8.ctypes.data, None, 0) == 1
    torch.cuda.synchronize()
    assert torch.all(dst == -9.0).item()
    assert hip.bcnn_hip_augment_letterbox_batch(*ok) == 0    # and the entry still works
    torch.cuda.synchronize()
    assert not torch.any(dst[:3] == -9.0).item() and torch.all(dst[3:] == -9.0).item()


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------------
TRAIN_GRAPH = CONFIG.replace("[conv]\nsrc=input\ndst=c1\nfilters=6\nsize=1\nstride=1\npad=0\nfunction=none\n",
                             "[conv]\nsrc=input\ndst=c0\nfilters=8\nsize=3\nstride=1\npad=1\nfunction=relu\n"
                             "[conv]\nsrc=c0\ndst=c1\nfilters=6\nsize=1\nstride=1\npad=0\nfunction=none\n")


def test_training_from_the_device_loader_equals_training_from_the_host_loader(tmp_path):
    from bcnn_amd import capi
    assert "dst=c0" in TRAIN_GRAPH
    lst, _ = _dataset(tmp_path, [(24, 24), (15, 20), (8, 8), (20, 15), (16, 16)], np.random.RandomState(12))
    results = []
    for device in (False, True):
        net = _net(tmp_path, TRAIN_GRAPH, capi.MODE_TRAIN, device, "train%d" % device)
        assert _set_loader(net, lst, lst) == 0
        net.set_sgd(0.001, 0.9, 5e-4)
        net.compile()
        libc.srand(99)
        costs = []
        for _ in range(4):
            costs.append(np.float32(net.L.bcnn_train_on_batch(net.net)))
            assert net.loader_device_letterboxed() == (N if device else 0)
        weights = []
        for name in ("input_w", "input_b", "c0_w", "c0_b"):
            i = net.index(name)
            assert i >= 2, name
            net.download(i, False)
            weights.append(net.data(i).copy())
        results.append((costs, weights, libc.rand()))
        net.close()
    (ca, wa, ra), (cb, wb, rb_) = results
    assert all(np.isfinite(ca)) and len(set(ca)) == 4, ca       # the net trains: four different costs
    assert ca == cb, (ca, cb)
    for a, b in zip(wa, wb):
        assert np.array_equal(a, b)
    assert ra == rb_
