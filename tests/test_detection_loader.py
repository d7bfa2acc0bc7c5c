"""BCNN_LOAD_DETECTION_LIST (bcnn_amd/host/bcnn_data.c: list_detection_next) against the unmodified reference
(bcnn_detection_loader.c) through the public API: the same config file, the same list file and the same libc rand() seed
on both sides, batches and label tensors byte for byte. The images are square or 2:1, for which the reference's integer
aspect ratio is the true one; the 4:3 and 3:4 images of the last test are checked on this build alone, where the ratio is
the float one."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from oracle import ref_bind as rb
from tests import _detect_ref as D

pytestmark = pytest.mark.gpu
libc = C.CDLL(None)
W = H = 16
N = 4
MAX_BOXES = 50

CONFIG = """[net]
input_width=16
input_height=16
input_channels=3
batch_size=4
train_detector=1
flip_h=1
min_contrast=0.8
max_contrast=1.2
min_brightness=-20
max_brightness=20
[conv]
src=input
dst=c1
filters=6
size=1
stride=1
pad=0
function=none
[yolo]
src=c1
dst=yolo
num_anchors=2
num_classes=1
num_coords=4
anchors=3,4,6,5
mask=0
"""


def _write_ppm(path, img):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def _write_png(path, img):
    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xffffffff)
    rows = b"".join(b"\0" + img[y].tobytes() for y in range(img.shape[0]))   # filter type 0 on every row
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", img.shape[1], img.shape[0], 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows)) + chunk(b"IEND", b""))


def _boxes(rs, k):
    return " ".join("%d %.4f %.4f %.4f %.4f" % (rs.randint(2), *rs.uniform(0.1, 0.9, 2), *rs.uniform(0.05, 0.5, 2))
                    for _ in range(k))


def _dataset(tmp, shapes, rs, edge_rows=True):
    """list file over one image per (h, w) of `shapes`; with edge_rows a row of 60 boxes, a malformed row and an
    unreadable path in between. Returns (list path, image paths)."""
    lines, paths = [], []
    for k, (h, w) in enumerate(shapes):
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        p = str(tmp / ("img%d.%s" % (k, "png" if k % 3 == 2 else "ppm")))
        (_write_png if k % 3 == 2 else _write_ppm)(p, img)
        paths.append(p)
        lines.append("%s %s" % (p, _boxes(rs, 1 + k % 3)))
    if edge_rows:
        lines.insert(1, "%s %s" % (paths[0], _boxes(rs, 60)))                    # 60 boxes: 50 are kept
        lines.insert(3, "%s 1 0.5 0.5 0.2 0.2 0 0.3" % paths[1])                 # 1 + 7 fields: skipped
        lines.insert(4, "%s %s" % (str(tmp / "missing.ppm"), _boxes(rs, 2)))     # unreadable: skipped
    lst = tmp / "list.txt"
    lst.write_text("\n".join(lines) + "\n")
    return str(lst), paths


def _nets(tmp, mode):
    from bcnn_amd import capi
    D.need_ref()
    cfg = tmp / "det.cfg"
    cfg.write_text(CONFIG)
    ref = rb.RefNet(mode=mode, w=W, h=H, c=3, n=N)
    ref.L.bcnn_load_net.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    ref.L.bcnn_load_net.restype = C.c_int
    libc.srand(5)
    assert ref.L.bcnn_load_net(ref.net, str(cfg).encode(), None) == 0
    libc.srand(5)
    hip = capi.Net.load_net(str(cfg), None, mode=mode)
    assert hip.get_detector_training() == 1
    return ref, hip


def _set_loader(net, train, test):
    net.L.bcnn_set_data_loader.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
    net.L.bcnn_set_data_loader.restype = C.c_int
    return net.L.bcnn_set_data_loader(net.net, 4, train.encode(), None, test.encode(), None)


def _next(net):
    net.L.bcnn_loader_next.argtypes = [C.c_void_p]
    net.L.bcnn_loader_next.restype = C.c_int
    assert net.L.bcnn_loader_next(net.net) == 0
    return net.data(0).copy(), net.data(1).copy()


def _same_batches(ref, hip, batches, seed):
    outs = []
    for net in (ref, hip):
        libc.srand(seed)
        outs.append([_next(net) for _ in range(batches)])
    for k, ((xa, ya), (xb, yb)) in enumerate(zip(*outs)):
        assert ya.shape == yb.shape == (N, 1, 1, 5 * MAX_BOXES)
        assert np.array_equal(xa, xb), ("input", k)
        assert np.array_equal(ya, yb), ("label", k)
    return outs[1]


def test_batches_and_labels_match_reference(tmp_path):
    rs = np.random.RandomState(21)
    lst, _ = _dataset(tmp_path, [(24, 24), (16, 32), (8, 8), (10, 20), (16, 16)], rs)
    ref, hip = _nets(tmp_path, rb.MODE_TRAIN)
    for net in (ref, hip):
        assert _set_loader(net, lst, lst) == 0
        net.compile()
    got = _same_batches(ref, hip, 5, seed=77)     # 20 samples over 6 readable rows: wraps around, skips two rows each time
    assert len({x.tobytes() for x, _ in got}) == 5
    labels = np.concatenate([y.reshape(N, MAX_BOXES, 5) for _, y in got])
    counts = sorted({int(np.count_nonzero(row[:, 2])) for row in labels})
    assert counts[-1] == MAX_BOXES and counts[0] in (1, 2, 3), counts          # the 60-box row kept 50, and no more
    full = [row for row in labels if np.count_nonzero(row[:, 2]) == MAX_BOXES]
    assert len({r.tobytes() for r in full}) > 1                                  # drawn offsets / flips: no two visits alike
    for net in (ref, hip):
        assert net.L.bcnn_set_mode(net.net, rb.MODE_VALID) == 0
    first = _same_batches(ref, hip, 2, seed=78)
    for net in (ref, hip):                                                       # VALID rewinds: the same samples again
        assert net.L.bcnn_set_mode(net.net, rb.MODE_TRAIN) == 0
        assert net.L.bcnn_set_mode(net.net, rb.MODE_VALID) == 0
    again = _same_batches(ref, hip, 2, seed=79)
    assert np.array_equal(first[0][0], again[0][0])
    ref.close()
    hip.close()


def test_float_aspect_ratio_letterbox(tmp_path):
    """own side only: a 4:3 and a 3:4 image outside TRAIN mode are centred at their true ratio, the canvas around them is
    128 exactly, and the boxes move with the image -- every expression in fp32, as the loader forms it"""
    from bcnn_amd import capi
    rs = np.random.RandomState(3)
    shapes = [(15, 20), (20, 15), (15, 20), (20, 15)]
    lst, _ = _dataset(tmp_path, shapes, rs, edge_rows=False)
    rows = [ln.split(" ")[1:] for ln in open(lst).read().splitlines()]
    cfg = tmp_path / "det.cfg"
    cfg.write_text(CONFIG)
    hip = capi.Net.load_net(str(cfg), None, mode=capi.MODE_VALID)
    assert _set_loader(hip, lst, lst) == 0
    hip.compile()
    x, y = _next(hip)
    f = np.float32
    for b, (h_img, w_img) in enumerate(shapes):
        ratio = f(w_img) / f(h_img)
        nw, nh = (int(f(H) * ratio), H) if ratio < 1 else (W, int(f(W) / ratio))
        assert (nw, nh) == ((12, 16) if w_img < h_img else (16, 12))
        dx, dy = (W - nw) // 2, (H - nh) // 2
        inside = np.zeros((H, W), bool)
        inside[dy:dy + nh, dx:dx + nw] = True
        pix = np.rint(x[b].astype(np.float64) * 127.5 + 127.5)
        assert np.all(pix[:, ~inside] == 128) and len(np.unique(x[b][:, ~inside])) == 1
        assert len(np.unique(pix[:, inside])) > 20                     # the image itself is there
        sx, sy, sdx, sdy = f(nw) / f(W), f(nh) / f(H), f(dx) / f(W), f(dy) / f(H)
        want = np.zeros((MAX_BOXES, 5), np.float32)
        for k in range(len(rows[b]) // 5):
            c, bx, by, bw, bh = rows[b][5 * k:5 * k + 5]
            want[k] = [f(float(bx)) * sx + sdx, f(float(by)) * sy + sdy, f(float(bw)) * sx, f(float(bh)) * sy, int(c)]
        assert np.array_equal(y[b].reshape(MAX_BOXES, 5), want), b
    hip.close()
