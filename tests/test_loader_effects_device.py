"""bcnn_set_loader_effects on the device: with the switch on, bcnn_loader_next applies Perlin
distortion and random spotlights, and the three device routes (bcnn_set_loader_on_device, bcnn_set_loader_decode_on_device,
bcnn_set_loader_detection_on_device) give the host path's input tensor, labels and rand() state BIT FOR BIT. The host path
itself is held to the compiled reference in tests/test_augment_effects.py, and once more here through the MNIST loader.
The entry that stages the effects (bcnn_hip_augment_effects_begin) is also driven alone, against libbip's host functions, on
the degenerate sample sizes, on batches where only some samples carry a flag, and through each of its refusals.

The nets come from config files: `max_distortion` has no setter (bcnn_augment_data_with_distortion stores another
member, like the reference's). Shapes: the smallest that run both effects with every other stage, more than one block per
sample, a centre crop, and a width that is no multiple of 4."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ref_bind as rb
from tests.test_data_loader import LIB, _set_loader, _u8, _write_cifar, _write_mnist, libc
from tests.test_loader_device import NET_CONF, TRAIN, VALID, _close, _dev_next, _play, _same, _write_list_files

pytestmark = pytest.mark.gpu

EFFECTS = "max_distortion=0.3\nmax_spots=3\n"


def _conf(w, h, c, n, keys, classes=10):
    text = NET_CONF % keys
    text = text.replace("batch=8", "batch=%d" % n).replace("width=32", "width=%d" % w).replace("height=32", "height=%d" % h)
    return text.replace("channels=3", "channels=%d" % c).replace("output=10", "output=%d" % classes)


def _net(tmp_path, name, text, device=False, effects=True, decode=False, mode=TRAIN):
    from bcnn_amd import capi
    cfg = tmp_path / (name + ".conf")
    cfg.write_text(text)
    net = capi.Net.load_net(str(cfg), None, mode=mode)
    assert net.get_loader_effects() == 0
    assert net.set_loader_effects(effects) == 0 and net.set_loader_on_device(device) == 0
    assert net.set_loader_decode_on_device(decode) == 0
    return net


def _pair(tmp_path, text, **kw):
    """the same net twice: the device path first, then the host path"""
    return [_net(tmp_path, "dev", text, device=True, **kw), _net(tmp_path, "host", text, device=False)]


@pytest.mark.parametrize("side", [28, 24], ids=["native_size", "centre_crop_to_24"])
def test_mnist(tmp_path, side):
    """cropped to 24: the effects are computed on the stored 28 x 28 sample and cropped afterwards"""
    tr = _write_mnist(tmp_path, "train", 21, seed=1)
    te = _write_mnist(tmp_path, "t10k", 12, seed=2)
    nets = _pair(tmp_path, _conf(side, side, 1, 8, EFFECTS + "range_shift_x=5\nrange_shift_y=5\nrotation_range=30\n"))
    for n in nets:
        assert _set_loader(n, 0, tr[0], tr[1], te[0], te[1]) == 0
        n.compile()
    got = _same(nets, [(TRAIN, 3), (VALID, 1)], seed=123)
    assert len({g[0].tobytes() for g in got}) == 4
    _close(nets)


def test_cifar10_with_every_stage(tmp_path):
    tr, te = _write_cifar(tmp_path, "data_batch_1", 13, seed=3), _write_cifar(tmp_path, "test_batch", 9, seed=4)
    keys = EFFECTS + ("range_shift_x=4\nrange_shift_y=2\nmin_scale=0.9\nmax_scale=1.1\nrotation_range=10\nmin_contrast=0.5\n"
                      "max_contrast=1.5\nmin_brightness=-50\nmax_brightness=10\nflip_h=1\n")
    nets = _pair(tmp_path, _conf(32, 32, 3, 6, keys))
    for n in nets:
        assert _set_loader(n, 1, tr, None, te, None) == 0
        n.L.bcnn_augment_data_with_flip.argtypes = [C.c_void_p, C.c_int, C.c_int]
        n.L.bcnn_augment_data_with_flip(n.net, 1, 0)
        n.compile()
    _same(nets, [(TRAIN, 3), (VALID, 1)], seed=77)
    _close(nets)


@pytest.mark.parametrize("decode", [False, True], ids=["host_decoded", "loader_decode_on_device"])
def test_classification_list(tmp_path, decode):
    """30 x 22 x 3 from files of several sizes (PNG, and JPEG where PIL can write them); the missing file's slot shows the
    previous sample with BOTH its own draws and the next ones applied, effects included, on either path"""
    _write_list_files(tmp_path, ((22, 30), (27, 34)), missing_at=(3,))
    keys = EFFECTS + "min_contrast=0.7\nmax_contrast=1.3\nmin_brightness=-10\nmax_brightness=30\nrotation_range=20\nswap_to_bgr=1\n"
    nets = _pair(tmp_path, _conf(30, 22, 3, 4, keys, classes=4), decode=decode)
    for n in nets:
        assert _set_loader(n, 2, str(tmp_path / "c.txt"), None, str(tmp_path / "c.txt"), None) == 0
        n.compile()
    assert nets[0].get_loader_decode_on_device() == int(decode)
    _same(nets, [(TRAIN, 3), (VALID, 1)], seed=31)
    _close(nets)


@pytest.mark.parametrize("channels", [1, 3])
def test_detection_list(tmp_path, channels):
    from bcnn_amd import capi
    from tests.test_detection_loader import CONFIG, N, _set_loader as _set_det
    from tests.test_detection_loader_device import WIDE, _assert_same, _mixed_list, _net as _det_net, _play as _det_play
    text = (CONFIG.replace("input_width=16", "input_width=40").replace("input_height=16", "input_height=24")
            .replace("input_channels=3", "input_channels=%d" % channels)
            .replace("train_detector=1\n", "train_detector=1\nloader_effects=1\nrange_shift_x=4\nrotation_range=20\n" + EFFECTS))
    lst = _mixed_list(tmp_path, np.random.RandomState(4), channels, WIDE)
    host, dev = _det_net(tmp_path, text, capi.MODE_TRAIN, False, "host"), _det_net(tmp_path, text, capi.MODE_TRAIN, True, "dev")
    for net in (host, dev):
        assert net.get_loader_effects() == 1
        assert _set_det(net, lst, lst) == 0
        net.compile()
    a, b = _det_play(host, 3, 11, (0, 0)), _det_play(dev, 3, 11, (N, 0))
    _assert_same(a, b, "train")
    assert len({x.tobytes() for x, _ in b[0]}) == 3
    off = _det_net(tmp_path, text.replace("loader_effects=1\n", ""), capi.MODE_TRAIN, True, "off")
    assert _set_det(off, lst, lst) == 0
    off.compile()
    c = _det_play(off, 1, 11, (N, 0))
    assert np.array_equal(c[0][0][1], b[0][0][1]) and not np.array_equal(c[0][0][0], b[0][0][0])   # same draws, other pixels
    _close((host, dev, off))


def test_switch_on_differs_in_train_and_not_in_valid_and_toggles(tmp_path):
    tr, te = _write_cifar(tmp_path, "data_batch_1", 13, seed=5), _write_cifar(tmp_path, "test_batch", 9, seed=6)
    text = _conf(32, 32, 3, 6, EFFECTS + "range_shift_x=4\nmin_contrast=0.8\nmax_contrast=1.2\n")
    on, off, toggled = (_net(tmp_path, "a", text, device=True), _net(tmp_path, "b", text, device=True, effects=False),
                        _net(tmp_path, "c", text, device=True))
    for n in (on, off, toggled):
        assert _set_loader(n, 1, tr, None, te, None) == 0
        n.compile()
    script = [(TRAIN, 4), (VALID, 1)]
    a, ra = _play(on, script, seed=9)
    b, rb_ = _play(off, script, seed=9)
    assert ra == rb_                                                    # the same number of rand() calls
    for k in range(4):
        assert not np.array_equal(a[k][0], b[k][0]), k                 # TRAIN: the effects show (fails without the feature)
        assert np.array_equal(a[k][1], b[k][1])
    assert np.array_equal(a[4][0], b[4][0])                            # VALID: nothing is drawn or applied
    libc.srand(9)                                                      # effects on, off, off, on; the device switch too
    got = []
    for k in range(4):
        assert toggled.set_loader_effects(k in (0, 3)) == 0 and toggled.set_loader_on_device(k != 2) == 0
        if k != 2:
            got.append(_dev_next(toggled)[0])
        else:
            toggled.L.bcnn_loader_next.argtypes = [C.c_void_p]
            assert toggled.L.bcnn_loader_next(toggled.net) == 0
            got.append(toggled.data(0).copy())
    for k in range(4):
        assert np.array_equal(got[k], (a if k in (0, 3) else b)[k][0]), k
    _close((on, off, toggled))


@pytest.mark.skipif(not rb.available(), reason="oracle/_ref not present")
def test_mnist_through_the_device_path_equals_the_reference(tmp_path):
    from bcnn_amd import capi
    tr = _write_mnist(tmp_path, "train", 21, seed=1)
    text = _conf(28, 28, 1, 8, EFFECTS + "range_shift_x=5\nrange_shift_y=5\nrotation_range=30\n")
    dev = _net(tmp_path, "dev", text, device=True)
    cfg = tmp_path / "ref.conf"
    cfg.write_text(text)
    ref = rb.RefNet(mode=rb.MODE_TRAIN, w=28, h=28, c=1, n=8)
    ref.L.bcnn_load_net.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    ref.L.bcnn_load_net.restype = C.c_int
    assert ref.L.bcnn_load_net(ref.net, str(cfg).encode(), None) == 0
    for n in (dev, ref):
        assert _set_loader(n, 0, tr[0], tr[1], tr[0], tr[1]) == 0
        n.compile()
    assert isinstance(dev, capi.Net)
    _same([dev, ref], [(TRAIN, 3)], seed=123)
    dev.close()
    ref.close()


# ---- the entry alone -----------------------------------------------------------------------------------------------------------
class Effect(C.Structure):
    _fields_ = [("flags", C.c_int32), ("seed", C.c_int32), ("distortion", C.c_float), ("first_spot", C.c_int32),
                ("num_spots", C.c_int32)]


class SpotBox(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("bw", C.c_int32), ("bh", C.c_int32), ("table", C.c_uint32)]


class Spot(C.Structure):
    _fields_ = [("mu_x", C.c_int32), ("mu_y", C.c_int32), ("sigma_x", C.c_float), ("sigma_y", C.c_float)]


DISTORT, SPOTS, RADIUS = 32, 64, 12
fp, ip, u8p, sz = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_size_t


def _bip():
    L = C.CDLL(os.path.join(LIB, "libbip.so"))
    L.bip_perlin_axis.argtypes = [sz, C.c_float, fp, fp, ip]
    L.bip_spot_table.argtypes = [C.POINTER(Spot), sz, sz, C.c_int32, ip, fp]
    L.bip_perlin_distortion_seeded.argtypes = [u8p, sz, sz, sz, sz, u8p, sz, C.c_float, C.c_float, C.c_float, C.c_int32]
    L.bip_add_spotlights.argtypes = [u8p, sz, sz, sz, sz, u8p, sz, C.POINTER(Spot), C.c_uint32]
    return L


def _stage_and_expect(bip, imgs, plan, brightness):
    """plan[b] = (distortion or None, kx, ky, seed, [Spot ...] or None). Builds the arguments of the entry with libbip's
    tabulating functions and the expected float batch with its host functions."""
    num, h, w, c = imgs.shape
    axis = w + h
    fx = (Effect * num)()
    perlin = np.zeros((num, 2, axis), np.float32)
    cells = np.zeros((num, axis), np.int32)
    boxes, tables, want = [], [], []
    for b, (distortion, kx, ky, seed, spots) in enumerate(plan):
        img = np.clip(imgs[b].astype(np.int32) + brightness, 0, 255).astype(np.uint8)
        if distortion is not None:
            fx[b].flags |= DISTORT
            fx[b].seed, fx[b].distortion = seed, distortion
            for off, extent, k in ((0, w, kx), (w, h, ky)):
                bip.bip_perlin_axis(extent, k, perlin[b, 0, off:].ctypes.data_as(fp), perlin[b, 1, off:].ctypes.data_as(fp),
                                    cells[b, off:].ctypes.data_as(ip))
            out = np.zeros_like(img)
            assert bip.bip_perlin_distortion_seeded(_u8(img), w * c, w, h, c, _u8(out), w * c, distortion, kx, ky, seed) == 0
            img = out
        if spots is not None:
            fx[b].flags |= SPOTS
            fx[b].first_spot, fx[b].num_spots = len(boxes), len(spots)
            for s in spots:
                box, val = (C.c_int32 * 4)(), np.zeros((2 * RADIUS + 1) ** 2, np.float32)
                assert bip.bip_spot_table(C.byref(s), w, h, RADIUS, box, val.ctypes.data_as(fp)) == 0
                boxes.append(SpotBox(box[0], box[1], box[2], box[3], sum(len(t) for t in tables)))
                tables.append(val[:box[2] * box[3]].copy())
            if spots:
                arr = (Spot * len(spots))(*spots)
                assert bip.bip_add_spotlights(_u8(img), w * c, w, h, c, _u8(img), w * c, arr, len(spots)) == 0
        want.append((img.astype(np.float32) - np.float32(127.5)) * np.float32(1 / 127.5))
    table = np.concatenate(tables) if tables else np.zeros(1, np.float32)
    spot_arr = (SpotBox * max(len(boxes), 1))(*boxes)
    args = dict(fx=fx, perlin=perlin, cells=cells, spots=spot_arr, num_spots=len(boxes), table=table,
                floats=sum(len(t) for t in tables))
    return args, np.stack(want).transpose(0, 3, 1, 2)


def _begin(L, num, w, h, a, **over):
    a = dict(a, **over)
    ptr = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else C.cast(x, C.c_void_p))
    return L.bcnn_hip_augment_effects_begin(num, w, h, ptr(a["fx"]), ptr(a["perlin"]), ptr(a["cells"]), ptr(a["spots"]),
                                            a["num_spots"], ptr(a["table"]), a["floats"])


def _batch(L, imgs, brightness):
    import torch
    num, h, w, c = imgs.shape
    dst = torch.full((num, c, h, w), 9.0, device="cuda")
    records = np.zeros((num, 8), np.int32)
    records[:, 6] = brightness
    assert L.bcnn_hip_augment_batch(dst.data_ptr(), num, c, h, w, num, w, h, imgs.ctypes.data, records.ctypes.data, None, 0) == 0
    torch.cuda.synchronize()
    return dst.cpu().numpy()


CASES = {
    "1x1": (1, 1, 1), "2x2": (2, 2, 3), "1x5": (1, 5, 1), "5x1x4": (5, 1, 4), "some_flags_33x21": (33, 21, 3),
    "zero_spots_9x7": (9, 7, 2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_entry_with_the_batch_call_matches_the_host_pixel_step(case):
    from bcnn_amd import _lib
    L, bip = _lib.load(), _bip()
    w, h, c = CASES[case]
    rs = np.random.RandomState(len(case))
    num = 5
    imgs = rs.randint(0, 256, (num, h, w, c)).astype(np.uint8)
    corner = [Spot(0, 0, 0.8, 3.5), Spot(w - 1, h - 1, 3.5, 0.8), Spot(w // 2, h // 2, 2.0, 1.1)]
    if case.startswith("some_flags"):      # only some samples carry a flag, and not the same ones
        plan = [(0.3, 0.21, -0.4, 77, None), (None, 0, 0, 0, corner), (None, 0, 0, 0, None), (0.0, 0.5, 0.5, 1, corner[:1]),
                (1.5, -0.5, 0.49, 123456789, corner)]
    elif case.startswith("zero_spots"):    # the stage is on and the count drawn was 0
        plan = [(None, 0, 0, 0, []), (0.2, 0.1, 0.1, 5, []), (None, 0, 0, 0, []), (None, 0, 0, 0, []), (None, 0, 0, 0, [])]
    else:
        plan = [(0.3, 0.21, -0.4, 77 + b, corner if b % 2 else corner[:1]) for b in range(num)]
    args, want = _stage_and_expect(bip, imgs, plan, 10)
    assert _begin(L, num, w, h, args) == 0
    got = _batch(L, imgs, 10)
    assert np.array_equal(got, want), int((got != want).sum())
    plain = (np.clip(imgs.astype(np.int32) + 10, 0, 255).astype(np.float32) - np.float32(127.5)) * np.float32(1 / 127.5)
    assert np.array_equal(_batch(L, imgs, 10), plain.transpose(0, 3, 1, 2))      # consumed: the next batch is plain


def test_refusals_return_1_and_leave_the_next_plain_batch_correct():
    from bcnn_amd import _lib
    L, bip = _lib.load(), _bip()
    w, h, c, num = 9, 7, 3, 2
    imgs = np.random.RandomState(3).randint(0, 256, (num, h, w, c)).astype(np.uint8)
    spots = [Spot(1, 1, 1.0, 1.0), Spot(8, 6, 3.5, 3.5)]
    args, want = _stage_and_expect(bip, imgs, [(0.3, 0.1, 0.2, 9, spots), (None, 0, 0, 0, spots[:1])], 0)
    plain = ((imgs.astype(np.float32) - np.float32(127.5)) * np.float32(1 / 127.5)).transpose(0, 3, 1, 2)

    def edited(field, value, index=0):
        arr = (type(args["spots"][0]) * len(args["spots"]))(*args["spots"]) if field in ("bw", "x0", "table") else None
        if arr is not None:
            setattr(arr[index], field, value)
            return dict(spots=arr)
        fx = (Effect * num)(*args["fx"])
        setattr(fx[index], field, value)
        return dict(fx=fx)

    refusals = [dict(fx=None), dict(perlin=None), dict(cells=None), dict(spots=None), dict(table=None),
                edited("flags", 1), edited("num_spots", 4), edited("first_spot", -1), edited("distortion", float("inf")),
                edited("bw", w + 1), edited("x0", -1), edited("table", args["floats"]), dict(floats=args["floats"] - 1),
                dict(num_spots=-1)]
    for over in refusals:
        assert _begin(L, num, w, h, args, **over) == 1, list(over)
        assert np.array_equal(_batch(L, imgs, 0), plain), list(over)          # nothing was staged
    assert _begin(L, 0, w, h, args) == 1 and _begin(L, num, 0, h, args) == 1
    # counts that do not fit the batch that follows: the batch call refuses, drops what was staged, and the next is plain
    import torch
    dst = torch.zeros((num, c, h, w), device="cuda")
    records = np.zeros((num, 8), np.int32)
    assert _begin(L, num + 1, w, h, dict(args, fx=(Effect * (num + 1))())) == 0
    assert L.bcnn_hip_augment_batch(dst.data_ptr(), num, c, h, w, num, w, h, imgs.ctypes.data, records.ctypes.data, None, 0) == 1
    assert np.array_equal(_batch(L, imgs, 0), plain)
    assert _begin(L, num, w, h, args) == 0
    L.bcnn_hip_augment_effects_cancel()
    assert np.array_equal(_batch(L, imgs, 0), plain)
    assert _begin(L, num, w, h, args) == 0                                      # and the entry still works afterwards
    assert np.array_equal(_batch(L, imgs, 0), want)
