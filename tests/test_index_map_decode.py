"""CPU: libbip's class-index mask reader (bip_load_index_map / bip_load_index_map_from_memory). Grey PNG, palette PNG and
PNM P5 / P2 give their indices back, 255 included -- the palette's INDICES, not its colours; every format that holds no
class indices fails with BIP_UNKNOWN_ERROR and a reason on stderr; bip_load_image keeps expanding the palette."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from tests.test_data_loader import LIB

BIP_UNKNOWN_ERROR = 4
W, H = 33, 17


@pytest.fixture(scope="module")
def bip():
    L = C.CDLL(os.path.join(LIB, "libbip.so"))
    i32p, u8pp = C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_uint8))
    L.bip_load_index_map.argtypes = [C.c_char_p, u8pp, i32p, i32p]
    L.bip_load_index_map_from_memory.argtypes = [C.c_char_p, C.c_int, u8pp, i32p, i32p]
    L.bip_load_image.argtypes = [C.c_char_p, u8pp, i32p, i32p, i32p]
    return L


@pytest.fixture(scope="module")
def indices():
    m = np.random.RandomState(5).randint(0, 21, (H, W)).astype(np.uint8)
    m[0, :] = 255            # VOC's void border
    m[:, 0] = 255
    m[3, 3], m[4, 4] = 254, 0
    return m


def _palette():
    """entry i is deliberately not (i, i, i)"""
    rs = np.random.RandomState(9)
    pal = rs.randint(0, 256, (256, 3)).astype(np.uint8)
    pal[np.arange(256) == pal[:, 0], 0] ^= 0x55
    return pal


def _load(bip, path=None, data=None):
    buf, w, h = C.POINTER(C.c_uint8)(), C.c_int32(0), C.c_int32(0)
    if path is not None:
        st = bip.bip_load_index_map(str(path).encode(), C.byref(buf), C.byref(w), C.byref(h))
    else:
        st = bip.bip_load_index_map_from_memory(data, len(data), C.byref(buf), C.byref(w), C.byref(h))
    if st != 0:
        return st, None
    return st, np.ctypeslib.as_array(buf, shape=(h.value, w.value)).copy()


def _write(tmp_path, indices, kind):
    p = tmp_path / ("mask_" + kind)
    if kind == "grey.png":
        Image.fromarray(indices, "L").save(p)
    elif kind == "palette.png":
        im = Image.fromarray(indices, "P")
        im.putpalette(_palette().reshape(-1).tolist())
        im.save(p)
    elif kind == "p5.pgm":
        p.write_bytes(b"P5\n# a comment\n%d %d\n255\n" % (W, H) + indices.tobytes())
    elif kind == "p2.pgm":
        p.write_bytes(b"P2\n%d %d\n255\n" % (W, H) + b"\n".join(b" ".join(b"%d" % v for v in row) for row in indices) + b"\n")
    elif kind == "rgb.png":
        Image.fromarray(np.stack([indices] * 3, -1), "RGB").save(p)
    elif kind == "rgba.png":
        Image.fromarray(np.stack([indices] * 4, -1), "RGBA").save(p)
    elif kind == "la.png":
        Image.fromarray(np.stack([indices] * 2, -1), "LA").save(p)
    elif kind == "mask.jpg":
        Image.fromarray(indices, "L").save(p, format="JPEG")
    elif kind == "mask.bmp":
        Image.fromarray(np.stack([indices] * 3, -1), "RGB").save(p, format="BMP")
    elif kind == "p6.ppm":
        p.write_bytes(b"P6\n%d %d\n255\n" % (W, H) + np.stack([indices] * 3, -1).tobytes())
    return p


@pytest.mark.parametrize("kind", ["grey.png", "palette.png", "p5.pgm", "p2.pgm"])
def test_index_formats_round_trip(bip, indices, tmp_path, kind):
    p = _write(tmp_path, indices, kind)
    st, got = _load(bip, path=p)
    assert st == 0 and np.array_equal(got, indices)
    st, got = _load(bip, data=p.read_bytes())
    assert st == 0 and np.array_equal(got, indices)
    assert (got == 255).any() and (got == 254).any() and (got == 0).any()


@pytest.mark.parametrize("kind", ["rgb.png", "rgba.png", "la.png", "mask.jpg", "mask.bmp", "p6.ppm"])
def test_formats_without_class_indices_fail_with_the_documented_status(bip, indices, tmp_path, capfd, kind):
    p = _write(tmp_path, indices, kind)
    capfd.readouterr()
    st, _ = _load(bip, path=p)
    assert st == BIP_UNKNOWN_ERROR
    err = capfd.readouterr().err
    assert "bip_load_index_map" in err and "class" in err, err       # the line names the reason
    st, _ = _load(bip, data=p.read_bytes())
    assert st == BIP_UNKNOWN_ERROR


def test_missing_and_garbage_files_fail(bip, tmp_path):
    assert _load(bip, path=tmp_path / "nowhere.png")[0] == BIP_UNKNOWN_ERROR
    assert _load(bip, data=b"not an image at all")[0] == BIP_UNKNOWN_ERROR
    assert _load(bip, data=b"\x89PNG\r\n\x1a\n")[0] == BIP_UNKNOWN_ERROR


def test_load_image_still_expands_the_palette(bip, indices, tmp_path):
    p = _write(tmp_path, indices, "palette.png")
    buf, w, h, d = C.POINTER(C.c_uint8)(), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert bip.bip_load_image(str(p).encode(), C.byref(buf), C.byref(w), C.byref(h), C.byref(d)) == 0
    assert (w.value, h.value, d.value) == (W, H, 3)
    got = np.ctypeslib.as_array(buf, shape=(H, W, 3))
    assert np.array_equal(got, _palette()[indices])
    assert not np.array_equal(got[:, :, 0], indices)
