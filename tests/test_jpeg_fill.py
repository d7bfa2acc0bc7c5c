"""bcnn_fill_tensor_with_jpegs (Net.fill_jpegs): the input tensor of a batch from compressed JPEG buffers. The host only
runs the entropy decoder; inverse DCT, chroma upsampling and colour conversion run on the device (jpeg_pixels.hip) in
front of the existing fill kernel. Every stage is integer arithmetic shared with the host decoder, and the float conversion
is the existing kernel's, so every case compares bit for bit (tolerance 0) with Net.fill_images on the pixels that
bip_load_image_from_memory decodes from the same bytes (tests/test_input_images.py pins that call to the host
composition, tests/test_bip.py the decoder to the reference).

The fixtures (tests/golden/jpeg) are the smallest shapes at which each stage can go wrong: one block; one-sample chroma
rows (1x1, 2x1); odd extents with partial MCUs; every upsampling case (4:2:2, 4:2:0, 4:4:0, 4:1:1) at one MCU and at several
ragged ones; progressive files whose transformed blocks are fewer than their whole MCUs; restart markers; both clamps; and
70x61 (120 transformed blocks: four workgroups of the transform at 32 blocks each, the last one ragged; 549 runs of 8
pixels: three workgroups of the colour kernel, the last one ragged)."""
import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from tests import _jpeg_fixtures as J
from tests.test_input_images import LETTERBOX, MEAN, NORM, STRETCH, device_input, make_net, preset, same_bits

pytestmark = pytest.mark.gpu

W, H = 37, 21

_decoded = {}


def decoded(name):
    """host-decoded pixels of a fixture, decoded once and shared (read-only)"""
    if name not in _decoded:
        st, img = J.host_decode(J.read(name))
        assert st == 0
        img.setflags(write=False)
        _decoded[name] = img
    return _decoded[name]


def reference_fill(names, c, n, fit, swap, mean=MEAN, norm=NORM, plane=(W, H)):
    """the input tensor after Net.fill_images on the host-decoded pixels, entries past len(names) as preset"""
    net = make_net(plane[0], plane[1], c, n)
    preset(net)
    assert net.fill_images([decoded(m) for m in names], fit=fit, norm_coeff=norm, swap_to_bgr=swap, mean=mean) == 0
    got = device_input(net)
    net.close()
    return got


@pytest.mark.parametrize("name,w,h,c,digest", J.manifest())
def test_each_fixture_alone_matches_fill_images_on_host_decoded_pixels(name, w, h, c, digest):
    data = J.read(name)
    net = make_net(W, H, c, 2)
    for fit, swap, mean in ((STRETCH, 1, MEAN), (LETTERBOX, 0, (0.0, 0.0, 0.0))):
        want = reference_fill([name], c, 2, fit, swap, mean)
        before = preset(net)
        assert net.fill_jpegs([data], fit=fit, norm_coeff=NORM, swap_to_bgr=swap, mean=mean) == (0, -1)
        got = device_input(net)
        assert same_bits(got[0], want[0]), (name, fit)
        assert same_bits(got[1], before[1]), (name, fit)
    net.close()


# different sizes and subsamplings, baseline and progressive, restart markers, the several-workgroup image in the middle
MIXED = ["y422_33x18.jpg", "prog_y420_27x21.jpg", "y420_70x61.jpg", "y411_33x18.jpg", "y420_1x1.jpg", "y440_33x18.jpg",
         "restart_y420_40x24.jpg", "q100_contrast_32x24.jpg", "y444_8x8.jpg"]


@pytest.mark.parametrize("fit", [STRETCH, LETTERBOX])
@pytest.mark.parametrize("swap", [0, 1])
def test_mixed_batch_matches_and_leaves_the_entries_past_num_images(fit, swap):
    n = len(MIXED) + 2
    want = reference_fill(MIXED, 3, n, fit, swap)
    net = make_net(W, H, 3, n)
    before = preset(net)
    assert net.fill_jpegs([J.read(m) for m in MIXED], fit=fit, norm_coeff=NORM, swap_to_bgr=swap, mean=MEAN) == (0, -1)
    got = device_input(net)
    net.close()
    for b, name in enumerate(MIXED):
        assert same_bits(got[b], want[b]), name
    assert same_bits(got[len(MIXED):], before[len(MIXED):])


def test_grey_batch_into_a_one_channel_tensor():
    names = ["grey_13x11.jpg", "prog_grey_19x13.jpg"]
    want = reference_fill(names, 1, 3, LETTERBOX, 1)
    net = make_net(W, H, 1, 3)
    before = preset(net)
    assert net.fill_jpegs([J.read(m) for m in names], fit=LETTERBOX, norm_coeff=NORM, swap_to_bgr=1, mean=MEAN) == (0, -1)
    got = device_input(net)
    net.close()
    assert same_bits(got[:2], want[:2]) and same_bits(got[2], before[2])


def test_host_threads_do_not_change_the_tensor():
    want = reference_fill(MIXED, 3, len(MIXED), STRETCH, 0)
    net = make_net(W, H, 3, len(MIXED))
    assert net.set_num_threads(4) == 0
    preset(net)
    assert net.fill_jpegs([J.read(m) for m in MIXED], fit=STRETCH, norm_coeff=NORM, mean=MEAN) == (0, -1)
    got = device_input(net)
    net.close()
    assert same_bits(got, want)


def test_refusals_return_invalid_parameter_and_leave_the_tensor():
    import ctypes as C
    net = make_net(W, H, 3, 3)
    before = preset(net)
    a, b, c = J.read("y420_17x9.jpg"), J.read("y422_16x16.jpg"), J.read("y444_8x8.jpg")
    grey = J.read("grey_13x11.jpg")
    cut = b[:len(b) - 60]                          # the headers are whole, the scan is not
    assert J.frame_info(cut)[0] == 0 and J.host_decode(cut)[0] != 0
    refused = {
        "a truncated stream in the middle": (net.fill_jpegs([a, cut, c]), 1),
        "a stream without a frame header": (net.fill_jpegs([a, c, b[:20]]), 2),
        "a grey stream into three channels": (net.fill_jpegs([grey, a]), 0),
        "more images than the batch": (net.fill_jpegs([a, b, c, a]), -1),
        "no images": (net.fill_jpegs([]), -1),
        "an empty buffer": (net.fill_jpegs([a, b""]), 1),
        "unknown fit": (net.fill_jpegs([a], fit=2), -1),
        "tensor index past the end": (net.fill_jpegs([a], tensor=10000), -1),
        "tensor index below 0": (net.fill_jpegs([a], tensor=-1), -1),
    }
    for what, (result, index) in refused.items():
        assert result == (1, index), (what, result)
    # NULL arguments, straight through the C interface
    k = 2
    keep = [np.frombuffer(a, np.uint8), np.frombuffer(c, np.uint8)]
    ptrs = (C.c_void_p * k)(*[x.ctypes.data for x in keep])
    lens = (C.c_size_t * k)(*[x.size for x in keep])
    failed = C.c_int(7)
    call = net.L.bcnn_fill_tensor_with_jpegs
    assert call(net.net, 0, k, None, lens, STRETCH, NORM, 0, *MEAN, C.byref(failed)) == 1 and failed.value == -1
    assert call(net.net, 0, k, ptrs, None, STRETCH, NORM, 0, *MEAN, C.byref(failed)) == 1 and failed.value == -1
    assert call(net.net, 0, k, (C.c_void_p * k)(keep[0].ctypes.data, None), lens, STRETCH, NORM, 0, *MEAN,
                C.byref(failed)) == 1 and failed.value == 1
    assert call(net.net, 0, k, (C.c_void_p * k)(keep[0].ctypes.data, None), lens, STRETCH, NORM, 0, *MEAN, None) == 1
    t = net.tensor(0)                              # a tensor without a device buffer
    gpu = t.data_gpu
    t.data_gpu = None
    assert call(net.net, 0, k, ptrs, lens, STRETCH, NORM, 0, *MEAN, C.byref(failed)) == 1
    t.data_gpu = gpu
    assert same_bits(device_input(net), before)
    # the same arguments, unbroken, are accepted -- with failed_image NULL as well
    assert call(net.net, 0, k, ptrs, lens, STRETCH, NORM, 0, *MEAN, None) == 0
    assert call(net.net, 0, k, ptrs, lens, STRETCH, NORM, 0, *MEAN, C.byref(failed)) == 0 and failed.value == -1
    net.close()
    # an image whose letterbox extent comes out empty: 70 x 61 into a plane one sample wide, new_h = (61 * 1) / 70 = 0
    flat = make_net(1, 90, 3, 1)
    before = preset(flat)
    wide = J.read("y420_70x61.jpg")
    assert flat.fill_jpegs([wide], fit=LETTERBOX) == (1, 0)
    assert same_bits(device_input(flat), before)
    assert flat.fill_jpegs([wide], fit=STRETCH) == (0, -1)
    flat.close()


def test_back_to_back_calls_with_different_batches_reuse_the_staging_block():
    """the second call stages more than the first and starts while the first one's kernels may still run; it waits for
    the first call's copy only"""
    first, second = ["y420_17x9.jpg", "y444_8x8.jpg"], ["y420_70x61.jpg", "prog_y420_27x21.jpg"]
    want_a = reference_fill(first, 3, 2, LETTERBOX, 1)
    want_b = reference_fill(second, 3, 2, STRETCH, 0)
    net_a, net_b = make_net(W, H, 3, 2), make_net(W, H, 3, 2)
    preset(net_a)
    preset(net_b)
    net_a.sync()
    data_a, data_b = [bytearray(J.read(m)) for m in first], [bytearray(J.read(m)) for m in second]
    assert net_a.fill_jpegs(data_a, fit=LETTERBOX, norm_coeff=NORM, swap_to_bgr=1, mean=MEAN) == (0, -1)
    assert net_b.fill_jpegs(data_b, fit=STRETCH, norm_coeff=NORM, swap_to_bgr=0, mean=MEAN) == (0, -1)
    assert net_a.fill_images([decoded(m) for m in first], fit=LETTERBOX, norm_coeff=NORM, swap_to_bgr=1, mean=MEAN) == 0
    assert net_a.fill_jpegs(data_a, fit=LETTERBOX, norm_coeff=NORM, swap_to_bgr=1, mean=MEAN) == (0, -1)
    got_a, got_b = device_input(net_a), device_input(net_b)
    net_a.close()
    net_b.close()
    assert same_bits(got_a, want_a) and same_bits(got_b, want_b)
