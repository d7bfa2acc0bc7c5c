#!/usr/bin/env python3
"""Writes the JPEG fixtures of tests/golden/jpeg and their MANIFEST (name, width, height, components, sha256 of the pixels
bip_load_image_from_memory decodes). Needs PIL; the tests that read the fixtures do not. The content is seeded, so a
second run with the same PIL writes the same files.

PIL's encoder writes 4:4:4, 4:2:2 and 4:2:0 only. The 4:4:0 and 4:1:1 files are PIL streams whose frame header is
rewritten: a 4:2:2 stream has the blocks of a 4:4:0 one per MCU (Y Y Cb Cr) and a 4:2:0 stream those of a 4:1:1 one
(Y Y Y Y Cb Cr), so a stream encoded at a size with the same NUMBER of MCUs decodes as the other layout once the header's
extent and the luma sampling factors say so. The picture is scrambled; every stage of the decoder runs as for any file.
"""
import ctypes as C
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg")


def content(w, h, seed, contrast=False):
    rs = np.random.RandomState(seed)
    if contrast:      # saturated 3 x 3 patches: the transform overshoots on both sides and the colour conversion with it
        cells = rs.randint(0, 2, ((h + 2) // 3, (w + 2) // 3, 3)) * 255
        return np.kron(cells, np.ones((3, 3, 1)))[:h, :w].astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), (x + y) * 255.0 / max(w + h - 2, 1)], -1)
    return np.clip(base + rs.normal(0, 24, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(w, h, seed, mode="RGB", contrast=False, **kw):
    b = io.BytesIO()
    Image.fromarray(content(w, h, seed, contrast)).convert(mode).save(b, "JPEG", **kw)
    return b.getvalue()


def relayout(data, w, h, luma_hv):
    """the baseline stream `data` with extent w x h and luma sampling byte luma_hv in its frame header"""
    at = data.index(b"\xff\xc0")
    d = bytearray(data)
    d[at + 5:at + 9] = bytes([h >> 8, h & 255, w >> 8, w & 255])
    assert d[at + 10] == 1          # component id 1 = Y
    d[at + 11] = luma_hv
    return bytes(d)


def fixtures():
    q = dict(quality=85)
    yield "y444_8x8.jpg", encode(8, 8, 1, subsampling=0, **q)
    yield "y420_1x1.jpg", encode(1, 1, 2, subsampling=2, **q)
    yield "y420_2x1.jpg", encode(2, 1, 3, subsampling=2, **q)
    yield "grey_13x11.jpg", encode(13, 11, 4, mode="L", **q)
    yield "y420_17x9.jpg", encode(17, 9, 5, subsampling=2, **q)
    yield "y422_16x16.jpg", encode(16, 16, 6, subsampling=1, **q)
    yield "y422_33x18.jpg", encode(33, 18, 7, subsampling=1, **q)
    # 4:4:0 (MCU 8 x 16) from 4:2:2 (MCU 16 x 8): 16x16 has 2 MCUs either way; 33x18 has 5 x 2 = 10, as 80x16 in 4:2:2
    yield "y440_16x16.jpg", relayout(encode(16, 16, 8, subsampling=1, **q), 16, 16, 0x12)
    yield "y440_33x18.jpg", relayout(encode(80, 16, 9, subsampling=1, **q), 33, 18, 0x12)
    # 4:1:1 (MCU 32 x 8) from 4:2:0 (MCU 16 x 16): 16x16 has 1 x 2 = 2 MCUs, as 32x16; 33x18 has 2 x 3 = 6, as 48x32
    yield "y411_16x16.jpg", relayout(encode(32, 16, 10, subsampling=2, **q), 16, 16, 0x41)
    yield "y411_33x18.jpg", relayout(encode(48, 32, 11, subsampling=2, **q), 33, 18, 0x41)
    yield "prog_y420_27x21.jpg", encode(27, 21, 12, subsampling=2, progressive=True, **q)
    yield "prog_grey_19x13.jpg", encode(19, 13, 13, mode="L", progressive=True, **q)
    yield "restart_y420_40x24.jpg", encode(40, 24, 14, subsampling=2, restart_marker_blocks=1, **q)
    yield "q5_contrast_32x24.jpg", encode(32, 24, 15, contrast=True, subsampling=2, quality=5)
    yield "q100_contrast_32x24.jpg", encode(32, 24, 16, contrast=True, subsampling=0, quality=100)
    yield "y420_70x61.jpg", encode(70, 61, 17, subsampling=2, quality=60)


def decode(bip, data):
    src, w, h, c = C.POINTER(C.c_uint8)(), C.c_int32(), C.c_int32(), C.c_int32()
    st = bip.bip_load_image_from_memory(data, len(data), C.byref(src), C.byref(w), C.byref(h), C.byref(c))
    assert st == 0, "bip_load_image_from_memory: %d" % st
    return np.ctypeslib.as_array(src, shape=(h.value, w.value, c.value)).copy()


def main():
    bip = C.CDLL(os.path.join(ROOT, "bcnn_amd", "lib", "libbip.so"))
    os.makedirs(OUT, exist_ok=True)
    lines = []
    for name, data in fixtures():
        px = decode(bip, data)
        assert len(data) < 8192, (name, len(data))
        if "contrast" in name:
            assert px.min() == 0 and px.max() == 255, name      # both clamps fire
        open(os.path.join(OUT, name), "wb").write(data)
        lines.append("%s %d %d %d %s\n" % (name, px.shape[1], px.shape[0], px.shape[2], hashlib.sha256(px.tobytes()).hexdigest()))
        print(lines[-1].strip(), len(data), "bytes")
    open(os.path.join(OUT, "MANIFEST"), "w").writelines(lines)


if __name__ == "__main__":
    sys.exit(main())
