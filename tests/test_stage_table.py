"""GPU: the pinned staging table of runtime.hip (common.h: StageSlot, host_stage, host_stage_extend, stage_upload) through
the C-ABI entry points that stage a batch in it. Every case runs on a host thread of its own: the table is per thread, so
each case starts with empty blocks and the first call allocates, a larger one grows and a smaller one reuses, whatever ran
before in the process. Tensors are at most 2 x 3 x 20 x 24.

  * two slots do not alias: an image batch and its label batch queued back to back, one synchronise;
  * grow, shrink, grow on a slot with no synchronise in between: the second call waits for the first one's copy before it
    frees the block, the third reuses the larger block;
  * a _begin / _run pair with another staging call in between: _run refuses (1), drops the batch and queues nothing;
  * host_stage_extend keeps the batch _begin laid out when staged effects make the block grow.

The yardstick is the host: bcnn_convert_img_to_float on bytes that libbip's host functions made (bip_warp_label_map for
flip and shift, which move bytes and are the same pull-back for a mask and for a channel of an image;
bip_resize_bilinear and the paste for the letterbox; the host JPEG decoder; the host effects), bit for bit."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from tests import _jpeg_fixtures as JF
from tests import _label_cases as LC
from tests.test_detection_loader_device import _canvas, _converted
from tests.test_loader_effects_device import Spot, _begin, _bip, _stage_and_expect

pytestmark = pytest.mark.gpu
SENTINEL = -9.0
W, H = 24, 20            # the destination plane of every case
BIG = "y420_70x61.jpg"   # the larger fixture: 80 x 64 luma samples and two 40 x 32 chroma planes of coefficients


def _on_a_fresh_thread(fn):
    """runs fn on a new host thread (empty staging blocks, device 0, the null stream) and hands its failure on"""
    box = []

    def body():
        try:
            fn()
        except BaseException as e:   # noqa: B036 -- the assertion of the case, raised again below
            box.append(e)
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if box:
        raise box[0]


def _lib():
    from bcnn_amd import _lib
    return _lib.load()


def _dst(n=2, c=3, h=H, w=W):
    return torch.full((n, c, h, w), SENTINEL, dtype=torch.float32, device="cuda")


def _records(w, h, num, first=0):
    """flip and shift records of the loader's own making, one per sample"""
    draws = [dict(flip=True), dict(shift=(2, -1)), dict(flip=True, shift=(-3, 2)), dict()]
    return np.stack([LC.loader_record(w, h, **draws[(first + b) % len(draws)])[0] for b in range(num)])


def _host_images(imgs, recs, w=W, h=H):
    """[num][c][h][w] float32: flip and shift of every channel by bip_warp_label_map onto the canvas byte 128, the centre
    crop to w x h, bcnn_convert_img_to_float"""
    from bcnn_amd import ops
    out = []
    for img, rec in zip(imgs, recs):
        sh, sw, c = img.shape
        moved = np.stack([ops.warp_label_map(img[:, :, k], rec, None, 128) for k in range(c)], axis=2)
        cy, cx = (sh - h) // 2, (sw - w) // 2
        out.append(_converted(np.ascontiguousarray(moved[cy:cy + h, cx:cx + w]), False))
    return np.stack(out)


def _augment_batch(dst, imgs, recs):
    num, sh, sw, c = imgs.shape
    n, _, h, w = dst.shape
    return _lib().bcnn_hip_augment_batch(dst.data_ptr(), n, c, h, w, num, sw, sh, imgs.ctypes.data, recs.ctypes.data, None, 0)


def test_image_slot_and_label_slot_do_not_alias():
    from bcnn_amd import ops

    def case():
        rs = np.random.RandomState(1)
        imgs = rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
        maps = np.stack([LC.label_map(W, H, seed=k) for k in range(2)])
        recs = _records(W, H, 2)
        dst, label = _dst(), _dst(c=1)
        assert _augment_batch(dst, imgs, recs) == 0
        assert ops.augment_label_batch(label, maps, recs, None, 255) == 0     # does not wait for the images' copy
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), _host_images(imgs, recs))
        want = np.stack([ops.warp_label_map(maps[b], recs[b], None, 255) for b in range(2)]).astype(np.float32)
        assert np.array_equal(label.cpu().numpy()[:, 0], want)
    _on_a_fresh_thread(case)


def test_grow_shrink_grow_of_the_augment_slot():
    def case():
        rs = np.random.RandomState(2)
        batches = [rs.randint(0, 256, shape).astype(np.uint8) for shape in ((1, H, W, 3), (2, 36, 40, 3), (1, H, W, 3))]
        recs = [_records(b.shape[2], b.shape[1], b.shape[0], first=k) for k, b in enumerate(batches)]
        dsts = [_dst() for _ in batches]
        for dst, imgs, rec in zip(dsts, batches, recs):                       # 1.5 KB, then 8.7 KB, then 1.5 KB staged
            assert _augment_batch(dst, imgs, rec) == 0
        torch.cuda.synchronize()
        for dst, imgs, rec in zip(dsts, batches, recs):
            got = dst.cpu().numpy()
            assert np.array_equal(got[:len(imgs)], _host_images(imgs, rec)), imgs.shape
            assert np.all(got[len(imgs):] == SENTINEL)
    _on_a_fresh_thread(case)


def test_grow_shrink_grow_of_the_augment_slot_through_the_letterbox():
    """every branch of stage_taps through the ImageDesc the kernel reads: a one-column and a one-row source (the blend
    replicates), an image pasted at x_off > 0 and one at y_off > 0; enlarging and reducing on both axes"""
    from bcnn_amd import ops

    def case():
        rs = np.random.RandomState(3)
        img = lambda w, h: rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        batches = [([img(1, 7)], [(5, H, 9, 0)]),                             # one column; new_w, new_h, x_off, y_off
                   ([img(40, 36), img(36, 40)], [(12, H, 6, 0), (W, 10, 0, 5)]),
                   ([img(9, 1)], [(W, 3, 0, 8)])]                             # one row
        dsts = [_dst() for _ in batches]
        for dst, (images, boxes) in zip(dsts, batches):
            assert ops.augment_letterbox_batch(dst, images, boxes) == 0
        torch.cuda.synchronize()
        for dst, (images, boxes) in zip(dsts, batches):
            got = dst.cpu().numpy()
            for b, (im, box) in enumerate(zip(images, boxes)):
                assert np.array_equal(got[b], _converted(_canvas(im, box, W, H), False)), (im.shape, box)
            assert np.all(got[len(images):] == SENTINEL)
    _on_a_fresh_thread(case)


def test_grow_shrink_grow_of_the_label_slot():
    from bcnn_amd import ops

    def case():
        sizes = [(1, 12, 10), (2, W, H), (1, 12, 10)]                         # num, w, h
        maps = [np.stack([LC.label_map(w, h, seed=10 * k + b) for b in range(num)]) for k, (num, w, h) in enumerate(sizes)]
        recs = [_records(w, h, num, first=k) for k, (num, w, h) in enumerate(sizes)]
        labels = [_dst(c=1, h=h, w=w) for _, w, h in sizes]
        for label, m, rec in zip(labels, maps, recs):
            assert ops.augment_label_batch(label, m, rec, None, 21) == 0
        torch.cuda.synchronize()
        for label, m, rec in zip(labels, maps, recs):
            got = label.cpu().numpy()[:, 0]
            want = np.stack([ops.warp_label_map(m[b], rec[b], None, 21) for b in range(len(m))]).astype(np.float32)
            assert np.array_equal(got[:len(m)], want), m.shape
            assert np.all(got[len(m):] == SENTINEL)
    _on_a_fresh_thread(case)


# ---- the begin / run pairs ---------------------------------------------------------------------------------------------------------
class Frame(C.Structure):
    """bcnn_hip_jpeg_frame (include/bcnn_hip.h)"""
    _fields_ = [(k, C.c_int32) for k in ("width", "height", "ncomp", "hmax", "vmax")] + [("comp", JF.Component * 3)]


def _frame(name):
    """(stream, bip_jpeg_info, bcnn_hip_jpeg_frame, host-decoded pixels) of a fixture"""
    data = JF.read(name)
    st, info = JF.frame_info(data)
    assert st == 0
    f = Frame(info.width, info.height, info.ncomp, info.hmax, info.vmax)
    for k in range(info.ncomp):
        f.comp[k] = info.comp[k]
    st, img = JF.host_decode(data)
    assert st == 0
    return data, info, f, img


def _entropy_decode(data, info, where):
    assert JF.bip().bip_jpeg_read_coefficients(data, len(data), C.byref(info), C.cast(where, C.POINTER(C.c_int16))) == 0


def _fill_images(dst, imgs):
    """bcnn_hip_fill_images, stretch, (px - 127.5) / 127.5"""
    n, c, h, w = dst.shape
    num = len(imgs)
    ptrs = (C.c_void_p * num)(*[im.ctypes.data for im in imgs])
    ws = (C.c_int * num)(*[im.shape[1] for im in imgs])
    hs = (C.c_int * num)(*[im.shape[0] for im in imgs])
    return _lib().bcnn_hip_fill_images(dst.data_ptr(), n, c, h, w, num, C.cast(ptrs, C.c_void_p), C.cast(ws, C.c_void_p),
                                       C.cast(hs, C.c_void_p), None, 0, 1 / 127.5, 0, 127.5, 127.5, 127.5)


def test_a_stale_pending_jpeg_fill_is_refused():
    def case():
        L = _lib()
        data, info, frame, decoded = _frame(BIG)
        dst, other = _dst(n=1), _dst(n=1)
        coeff = (C.c_void_p * 1)()
        run = lambda: L.bcnn_hip_jpeg_stage_run(dst.data_ptr(), 1 / 127.5, 0, 127.5, 127.5, 127.5)
        assert L.bcnn_hip_jpeg_stage_begin(1, 3, H, W, 1, C.byref(frame), 0, C.cast(coeff, C.c_void_p), None) == 0
        _entropy_decode(data, info, coeff[0])
        # one 8 x 8 image stages far fewer bytes than the 15 KB of coefficients: the block is neither freed nor moved,
        # but it is this call's now
        small = np.random.RandomState(4).randint(0, 256, (8, 8, 3)).astype(np.uint8)
        assert _fill_images(other, [small]) == 0
        assert run() == 1                                                      # refused, dropped ...
        torch.cuda.synchronize()
        assert torch.all(dst == SENTINEL).item()                               # ... and nothing was queued
        assert not torch.any(other == SENTINEL).item()
        assert run() == 1                                                      # nothing is pending any more
        # a fresh pair goes through and gives the fill of the host-decoded pixels
        assert L.bcnn_hip_jpeg_stage_begin(1, 3, H, W, 1, C.byref(frame), 0, C.cast(coeff, C.c_void_p), None) == 0
        _entropy_decode(data, info, coeff[0])
        assert run() == 0
        assert _fill_images(other, [decoded]) == 0
        torch.cuda.synchronize()
        assert torch.equal(dst, other) and not torch.any(dst == SENTINEL).item()
    _on_a_fresh_thread(case)


def _jpeg_run(dst, num, records, origins, pixels):
    done = np.ones(num, np.uint8)
    return _lib().bcnn_hip_augment_jpeg_run(dst.data_ptr(), done.ctypes.data, pixels.ctypes.data, records.ctypes.data, None,
                                            origins.ctypes.data, 0)


def test_a_stale_pending_jpeg_training_batch_is_refused():
    def case():
        L = _lib()
        data, info, frame, decoded = _frame(BIG)
        dst, other = _dst(n=1), _dst(n=1, h=8, w=8)
        coeff = (C.c_void_p * 1)()
        records, origins = np.zeros((1, 8), np.int32), np.array([10, 7], np.int32)
        unused = np.zeros((1, H, W, 3), np.uint8)                              # the slot of a sample the caller decoded
        assert L.bcnn_hip_augment_jpeg_begin(1, 3, H, W, 1, C.byref(frame), C.cast(coeff, C.c_void_p)) == 0
        assert coeff[0]
        _entropy_decode(data, info, coeff[0])
        small = np.random.RandomState(5).randint(0, 256, (1, 8, 8, 3)).astype(np.uint8)
        assert _augment_batch(other, small, records) == 0                      # smaller: nothing is freed or moved
        assert _jpeg_run(dst, 1, records, origins, unused) == 1
        torch.cuda.synchronize()
        assert torch.all(dst == SENTINEL).item()
        assert np.array_equal(other.cpu().numpy(), _host_images(small, records, 8, 8))
        assert _jpeg_run(dst, 1, records, origins, unused) == 1                # nothing is pending any more
        # a fresh pair goes through: the 24 x 20 window at (10, 7) of the host-decoded image, converted
        assert L.bcnn_hip_augment_jpeg_begin(1, 3, H, W, 1, C.byref(frame), C.cast(coeff, C.c_void_p)) == 0
        _entropy_decode(data, info, coeff[0])
        assert _jpeg_run(dst, 1, records, origins, unused) == 0
        torch.cuda.synchronize()
        window = np.ascontiguousarray(decoded[7:7 + H, 10:10 + W])
        assert np.array_equal(dst.cpu().numpy()[0], _converted(window, False))
    _on_a_fresh_thread(case)


def test_staged_effects_that_make_the_block_grow_keep_what_begin_laid_out():
    """bcnn_hip_augment_jpeg_run learns of the staged effects after _begin has laid the batch out, and extends the block.
    Sizes, from the layout of bcnn_hip_augment_jpeg_begin / _run (augment.hip) for ONE sample of 24 x 20 x 3 out of
    y422_33x18.jpg (luma 6 x 3 blocks, chroma 3 x 3 each: 36 blocks of 128 bytes):
      records 32 + sums 16 + taps (24 + 20) * 8 = 352 + windows 32 + plane table (3 + 1) * 24 = 96
      + image table (1 + 1) * 96 = 192 + coefficients 4608 + raw samples 1440  =  device_at 6768
    On a fresh thread _begin's host_stage(6768) allocates 6768 + 6768 / 4 = 8460 bytes. The effects blob of one distorted
    sample with one spot whose table covers the sample is
      header 16 + sample 32 + spot 32 + perlin (24 + 20) * 12 = 528 + table 24 * 20 * 4 = 1920  =  2528,
    so _run asks host_stage_extend for 6768 + 2528 = 9296 > 8460: the block is reallocated and the 6768 bytes that hold
    the coefficients are carried over."""
    def case():
        L, bip = _lib(), _bip()
        data, info, frame, decoded = _frame("y422_33x18.jpg")
        assert (info.width, info.height) == (33, 18)
        coeff_bytes = 128 * sum(info.comp[k].blocks_w * info.comp[k].blocks_h for k in range(3))
        device_at = 32 + 16 + (W + H) * 8 + 32 + 4 * 24 + 2 * 96 + coeff_bytes + W * H * 3
        assert coeff_bytes == 4608 and device_at == 6768
        # the sample: the window at (4, -1) of the image, 0 outside it (the crop onto a zeroed buffer)
        origins = np.array([4, -1], np.int32)
        sample = np.zeros((1, H, W, 3), np.uint8)
        sample[0, 1:19, 0:24] = decoded[0:18, 4:28]
        args, want = _stage_and_expect(bip, sample, [(0.3, 0.21, -0.4, 77, [Spot(12, 10, 3.5, 3.5)])], 0)
        fx_bytes = 16 + 32 + 32 + (W + H) * 12 + 4 * args["floats"]
        assert args["floats"] == W * H and device_at + fx_bytes > device_at + device_at // 4
        dst = _dst(n=1)
        coeff = (C.c_void_p * 1)()
        records = np.zeros((1, 8), np.int32)
        assert _begin(L, 1, W, H, args) == 0
        assert L.bcnn_hip_augment_jpeg_begin(1, 3, H, W, 1, C.byref(frame), C.cast(coeff, C.c_void_p)) == 0
        _entropy_decode(data, info, coeff[0])
        assert _jpeg_run(dst, 1, records, origins, sample) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())
    _on_a_fresh_thread(case)
