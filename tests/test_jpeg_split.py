"""libbip.so's JPEG decoder split at the coefficient boundary (bip_jpeg_frame_info, bip_jpeg_read_coefficients, the host
pixel stage bip_jpeg_pixels_from_coefficients) on the fixtures of tests/golden/jpeg: the three calls in a row give
bip_load_image_from_memory's bytes, the reported block counts are read_frame's formulae, everything the one-call decoder
refuses is refused by the new entry points, and the threaded staging routine of libbcnn.so (bcnn_jpeg_read_batch) writes
the same bytes for 1 and 4 threads. No GPU, no PIL."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import _jpeg_fixtures as J

MANIFEST = J.manifest()


def test_manifest_covers_the_shapes_the_stages_can_go_wrong_at():
    names = set(J.NAMES)
    for need in ("y444_8x8", "y420_1x1", "y420_2x1", "grey_13x11", "y420_17x9", "prog_y420_27x21", "prog_grey_19x13",
                 "restart_y420_40x24", "q5_contrast_32x24", "q100_contrast_32x24", "y420_70x61"):
        assert need + ".jpg" in names, need
    for sub in ("y422", "y440", "y411"):
        assert {"%s_16x16.jpg" % sub, "%s_33x18.jpg" % sub} <= names, sub
    assert b"\xff\xdd" in J.read("restart_y420_40x24.jpg")           # a DRI segment: restart markers follow


@pytest.mark.parametrize("name,w,h,c,digest", MANIFEST)
def test_host_decoder_gives_the_recorded_pixels(name, w, h, c, digest):
    st, img = J.host_decode(J.read(name))
    assert st == 0 and img.shape == (h, w, c)
    assert hashlib.sha256(img.tobytes()).hexdigest() == digest
    if "contrast" in name:                                             # both clamps fire
        assert img.min() == 0 and img.max() == 255


@pytest.mark.parametrize("name,w,h,c,digest", MANIFEST)
def test_split_decoder_equals_the_one_call_decoder(name, w, h, c, digest):
    data = J.read(name)
    st, info = J.frame_info(data)
    assert st == 0 and (info.width, info.height, info.ncomp) == (w, h, c)
    st, coeff = J.read_coefficients(data, info)
    assert st == 0
    st, img = J.pixels(info, coeff)
    assert st == 0
    _, want = J.host_decode(data)
    assert np.array_equal(img, want)


SAMPLING = {"y444": (1, 1), "y422": (2, 1), "y420": (2, 2), "y440": (1, 2), "y411": (4, 1), "grey": (1, 1),
            "q5": (2, 2), "q100": (1, 1)}


@pytest.mark.parametrize("name,w,h,c,digest", MANIFEST)
def test_reported_geometry_follows_the_frame_header(name, w, h, c, digest):
    st, info = J.frame_info(J.read(name))
    assert st == 0
    key = name.replace("prog_", "").replace("restart_", "").split("_")[0]
    hmax, vmax = SAMPLING[key]
    assert (info.hmax, info.vmax) == (hmax, vmax)
    assert info.progressive == (1 if name.startswith("prog_") else 0)
    mcus_x, mcus_y = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    total = 0
    for k in range(c):
        p = info.comp[k]
        hk, vk = (hmax, vmax) if k == 0 else (1, 1)
        assert (p.h, p.v) == (hk, vk)
        assert (p.width, p.height) == (-(-w * hk // hmax), -(-h * vk // vmax))
        assert (p.blocks_w, p.blocks_h) == (mcus_x * hk, mcus_y * vk)
        assert (p.pitch, p.rows) == (8 * p.blocks_w, 8 * p.blocks_h)
        if info.progressive:      # only the blocks with content are transformed
            assert (p.idct_w, p.idct_h) == ((p.width + 7) >> 3, (p.height + 7) >> 3)
        else:                     # every block of every whole MCU
            assert (p.idct_w, p.idct_h) == (p.blocks_w, p.blocks_h)
        total += p.blocks_w * p.blocks_h * 64
    assert info.num_coefficients == total
    if name == "prog_y420_27x21.jpg":     # partial coverage: 4 x 3 blocks of luma content in 4 x 4 blocks of whole MCUs
        assert (info.comp[0].idct_w, info.comp[0].idct_h, info.comp[0].blocks_h) == (4, 3, 4)


def _cmyk_stream():
    """a four-component frame: y444_8x8.jpg with a fourth component added to its frame header"""
    data = bytearray(J.read("y444_8x8.jpg"))
    at = data.index(b"\xff\xc0")
    assert data[at + 2:at + 4] == bytes([0, 17]) and data[at + 9] == 3
    data[at + 3] = 20
    data[at + 9] = 4
    data[at + 19:at + 19] = bytes([4, 0x11, 0])
    return bytes(data)


def test_truncated_and_four_component_streams_fail_in_both_entry_points():
    data = J.read("y420_70x61.jpg")
    st, whole = J.frame_info(data)
    assert st == 0
    sos = data.index(b"\xff\xda")
    for cut in (0, 2, 20, sos - 1, sos + 8, (sos + len(data)) // 2, len(data) - 2):
        part = data[:cut]
        assert J.host_decode(part)[0] != 0, cut
        st, info = J.frame_info(part)
        if cut < sos:                                # the frame header is not complete or what follows it is missing
            if st == 0:
                assert J.read_coefficients(part, info)[0] != 0, cut
        else:
            assert st == 0, cut
        if st == 0:
            assert J.read_coefficients(part, info)[0] != 0, cut
        assert J.read_coefficients(part, whole)[0] != 0, cut
    cmyk = _cmyk_stream()
    assert J.host_decode(cmyk)[0] != 0
    st, info = J.frame_info(cmyk)
    assert st != 0
    assert J.read_coefficients(cmyk, whole)[0] != 0
    # an info that is not this buffer's is refused before anything is written
    other = J.frame_info(J.read("y444_8x8.jpg"))[1]
    assert J.read_coefficients(data, other)[0] != 0


def test_threaded_staging_writes_the_same_bytes_for_one_and_four_threads():
    from bcnn_amd import capi
    L = C.CDLL(capi.LIB_PATH)
    L.bcnn_jpeg_read_batch.restype = C.c_int
    names = ["y420_70x61.jpg", "prog_y420_27x21.jpg", "grey_13x11.jpg", "y411_33x18.jpg", "y440_16x16.jpg",
             "restart_y420_40x24.jpg", "prog_grey_19x13.jpg", "y420_1x1.jpg", "q100_contrast_32x24.jpg"]
    datas = [J.read(n) for n in names]
    k = len(datas)
    infos = (J.Info * k)(*[J.frame_info(d)[1] for d in datas])
    offs = np.cumsum([0] + [infos[b].num_coefficients for b in range(k)])
    bufs = (C.c_char_p * k)(*datas)
    lens = (C.c_size_t * k)(*[len(d) for d in datas])

    def run(threads, datas_ptr=bufs, lens_arr=lens):
        block = np.full(int(offs[-1]) + 2 * J.GUARD, 0x5a5a, np.int16)          # a plain heap block with canaries
        base = block[J.GUARD:].ctypes.data
        ptrs = (C.c_void_p * k)(*[base + 2 * int(o) for o in offs[:-1]])
        failed = L.bcnn_jpeg_read_batch(k, datas_ptr, lens_arr, infos, ptrs, threads)
        assert (block[:J.GUARD] == 0x5a5a).all() and (block[-J.GUARD:] == 0x5a5a).all()
        return failed, block

    f1, one = run(1)
    f4, four = run(4)
    f99, many = run(99)                                                          # more threads than images
    assert f1 == f4 == f99 == -1
    assert np.array_equal(one, four) and np.array_equal(one, many)
    for b in range(k):                                                           # and they are the coefficients
        _, want = J.read_coefficients(datas[b], infos[b])
        assert np.array_equal(one[J.GUARD + int(offs[b]):J.GUARD + int(offs[b + 1])], want), names[b]
    # two streams cut short: the lowest failing index is reported, for every thread count
    cut = list(datas)
    cut[6] = cut[6][:len(cut[6]) // 2]
    cut[2] = cut[2][:len(cut[2]) - 40]
    cut_bufs = (C.c_char_p * k)(*cut)
    cut_lens = (C.c_size_t * k)(*[len(d) for d in cut])
    assert run(1, cut_bufs, cut_lens)[0] == 2 and run(4, cut_bufs, cut_lens)[0] == 2
