"""The JPEG fixtures of tests/golden/jpeg (written by tools/make_jpeg_fixtures.py) and ctypes bindings of libbip.so's split
decoder: bip_jpeg_frame_info, bip_jpeg_read_coefficients, bip_jpeg_pixels_from_coefficients (include/bip/bip.h)."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "jpeg")
u8p = C.POINTER(C.c_uint8)


class Component(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("h", "v", "width", "height", "pitch", "rows", "blocks_w", "blocks_h", "idct_w",
                                         "idct_h")]


class Info(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("width", "height", "ncomp", "hmax", "vmax", "progressive")] + \
               [("num_coefficients", C.c_size_t), ("comp", Component * 3)]


def manifest():
    """[(name, width, height, components, sha256 of the decoded pixels)]"""
    rows = []
    for line in open(os.path.join(DIR, "MANIFEST")):
        name, w, h, c, digest = line.split()
        rows.append((name, int(w), int(h), int(c), digest))
    return rows


NAMES = [row[0] for row in manifest()]


def read(name):
    return open(os.path.join(DIR, name), "rb").read()


_bip = []


def bip():
    if not _bip:
        from bcnn_amd import capi
        L = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libbip.so"))
        L.bip_jpeg_frame_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(Info)]
        L.bip_jpeg_read_coefficients.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(Info), C.POINTER(C.c_int16)]
        L.bip_jpeg_pixels_from_coefficients.argtypes = [C.POINTER(Info), C.POINTER(C.c_int16), u8p]
        L.bip_load_image_from_memory.argtypes = [C.c_char_p, C.c_int, C.POINTER(u8p), C.POINTER(C.c_int32),
                                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        for fn in (L.bip_jpeg_frame_info, L.bip_jpeg_read_coefficients, L.bip_jpeg_pixels_from_coefficients,
                   L.bip_load_image_from_memory):
            fn.restype = C.c_int
        _bip.append(L)
    return _bip[0]


def host_decode(data):
    """(status, H x W x C uint8 or None) of bip_load_image_from_memory"""
    p, w, h, c = u8p(), C.c_int32(), C.c_int32(), C.c_int32()
    st = bip().bip_load_image_from_memory(data, len(data), C.byref(p), C.byref(w), C.byref(h), C.byref(c))
    if st != 0:
        return st, None
    img = np.ctypeslib.as_array(p, shape=(h.value, w.value, c.value)).copy()
    C.CDLL(None).free(p)
    return 0, img


GUARD = 64  # int16 of canary on either side of a coefficient buffer


def frame_info(data):
    info = Info()
    return bip().bip_jpeg_frame_info(data, len(data), C.byref(info)), info


def read_coefficients(data, info):
    """(status, coefficients as int16 array); asserts that nothing is written outside the num_coefficients asked for"""
    n = info.num_coefficients
    buf = np.full(n + 2 * GUARD, 0x5a5a, np.int16)
    st = bip().bip_jpeg_read_coefficients(data, len(data), C.byref(info),
                                          buf[GUARD:].ctypes.data_as(C.POINTER(C.c_int16)))
    assert (buf[:GUARD] == 0x5a5a).all() and (buf[GUARD + n:] == 0x5a5a).all(), "written outside coeff"
    return st, buf[GUARD:GUARD + n].copy()


def pixels(info, coeff):
    img = np.zeros((info.height, info.width, info.ncomp), np.uint8)
    st = bip().bip_jpeg_pixels_from_coefficients(C.byref(info), coeff.ctypes.data_as(C.POINTER(C.c_int16)),
                                                 img.ctypes.data_as(u8p))
    return st, img
