"""GPU: bcnn_hip_augment_label_batch (bcnn_amd/csrc/augment_label.hip) against libbip's host function
bip_warp_label_map, bit for bit, over the cases of tests/test_label_warp.py (which holds the host function to the numpy
restatement): every stage alone and all at once, shifts beyond the sample, both scale directions, the rotation angles,
the constructed ties, the three fill bytes, the one-sample axis; both kernel forms, read off the dispatch trace; the
planes behind num_samples; every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _label_cases as LC

pytestmark = pytest.mark.gpu
SENTINEL = -7.5


def _trace(on):
    from bcnn_amd import _lib
    L = _lib.load()
    if on:
        L.bcnn_hip_trace_enable(1)
        return None
    n = L.bcnn_hip_trace_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return buf.value.decode().split()


def _batches(w, h):
    """the cases of one size in batches of 3: (names, maps [3][h][w], records [3][8], taps [3][(w + h) * 2])"""
    cases = LC.cases(w, h)
    assert len(cases) % 3 == 0
    for at in range(0, len(cases), 3):
        group = cases[at:at + 3]
        maps = np.stack([LC.label_map(w, h, seed=at + k) for k in range(3)])
        recs = np.stack([np.zeros(8, np.int32) if r is None else r for _, r, _, _ in group])
        taps = np.stack([np.zeros((w + h) * 2, np.int32) if t is None else t for _, _, t, _ in group])
        yield [g[0] for g in group], maps, recs, taps


@pytest.mark.parametrize("w,h", LC.SIZES, ids=["%dx%d" % s for s in LC.SIZES])
def test_device_labels_equal_the_host_warp(w, h):
    from bcnn_amd import ops
    seen = set()
    for names, maps, recs, taps in _batches(w, h):
        for fill in LC.FILLS:
            want = np.stack([ops.warp_label_map(maps[b], recs[b], taps[b], fill) for b in range(3)]).astype(np.float32)
            label = torch.full((3, 1, h, w), SENTINEL, dtype=torch.float32, device="cuda")
            _trace(True)
            assert ops.augment_label_batch(label, maps, recs, taps, fill) == 0
            torch.cuda.synchronize()
            ran = _trace(False)
            got = label.cpu().numpy()[:, 0]
            for b in range(3):
                assert np.array_equal(got[b], want[b]), (names[b], fill, int((got[b] != want[b]).sum()))
            assert ran == ["augment_label:v4" if w % 4 == 0 else "augment_label"], ran
            seen.update(ran)
    assert seen == ({"augment_label:v4"} if w == 16 else {"augment_label"})   # 16 takes the 16-byte stores, 33 cannot


def test_a_misaligned_tensor_takes_the_scalar_form():
    from bcnn_amd import ops
    w, h = 16, 12
    _, maps, recs, taps = next(iter(_batches(w, h)))
    store = torch.full((3 * h * w + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    label = store[1:1 + 3 * h * w].view(3, 1, h, w)            # 4 bytes past a 16-byte boundary
    assert label.data_ptr() % 16 == 4
    _trace(True)
    assert ops.augment_label_batch(label, maps, recs, taps, 255) == 0
    torch.cuda.synchronize()
    assert _trace(False) == ["augment_label"]
    got = store.cpu().numpy()
    want = np.stack([ops.warp_label_map(maps[b], recs[b], taps[b], 255) for b in range(3)]).astype(np.float32)
    assert np.array_equal(got[1:1 + 3 * h * w].reshape(3, h, w), want)
    assert got[0] == SENTINEL and np.all(got[1 + 3 * h * w:] == SENTINEL)


@pytest.mark.parametrize("w,h", [(16, 12), (33, 17)])
def test_planes_behind_num_samples_are_not_written(w, h):
    from bcnn_amd import ops
    names, maps, recs, taps = list(_batches(w, h))[3]          # rotations and all four stages
    label = torch.full((3, 1, h, w), SENTINEL, dtype=torch.float32, device="cuda")
    assert ops.augment_label_batch(label, maps[:2], recs[:2], taps[:2], 21, num_samples=2) == 0
    torch.cuda.synchronize()
    got = label.cpu().numpy()[:, 0]
    for b in range(2):
        assert np.array_equal(got[b], ops.warp_label_map(maps[b], recs[b], taps[b], 21).astype(np.float32)), names[b]
    assert np.all(got[2] == SENTINEL)


def test_identity_records_and_no_taps():
    from bcnn_amd import ops
    w, h = 33, 17
    maps = np.stack([LC.label_map(w, h, seed=k) for k in range(3)])
    label = torch.full((3, 1, h, w), SENTINEL, dtype=torch.float32, device="cuda")
    assert ops.augment_label_batch(label, maps) == 0
    torch.cuda.synchronize()
    assert np.array_equal(label.cpu().numpy()[:, 0], maps.astype(np.float32))


def test_every_refusal_returns_1_and_writes_nothing():
    from bcnn_amd import _lib
    w, h = 16, 12
    L = _lib.load()
    _, maps, recs, taps = list(_batches(w, h))[2]              # scale_half, scale_1.7, rotate_0: two records with SCALE
    assert recs[0][0] & LC.SCALE and recs[1][0] & LC.SCALE
    label = torch.full((3, 1, h, w), SENTINEL, dtype=torch.float32, device="cuda")
    good = dict(label=label.data_ptr(), n=3, h=h, w=w, num=3, maps=maps.ctypes.data, recs=recs.ctypes.data,
                taps=taps.ctypes.data, fill=255)

    def call(**kw):
        a = dict(good, **kw)
        return L.bcnn_hip_augment_label_batch(a["label"], a["n"], a["h"], a["w"], a["num"], a["maps"], a["recs"], a["taps"],
                                              a["fill"])

    bad_taps = []
    for at, value in ((0, w - 1), (2, -2), (2 * w, h - 1), (2 * (w + h) + 2 * w + 2, -5)):   # both samples, both axes
        t = taps.copy()
        t.reshape(-1)[at] = value
        bad_taps.append(t)
    _trace(True)
    for kw in (dict(label=None), dict(maps=None), dict(recs=None), dict(taps=None), dict(n=0), dict(h=0), dict(w=0), dict(h=-3),
               dict(num=0), dict(num=4), dict(num=-1), dict(fill=-1), dict(fill=256), dict(n=2)):
        assert call(**kw) == 1, kw
    for t in bad_taps:
        assert call(taps=t.ctypes.data) == 1
    # a block past 2 GiB: 3 maps of 65536 x 16384 bytes (nothing of that size is read: the sum is refused first)
    assert call(w=65536, h=16384) == 1
    torch.cuda.synchronize()
    assert _trace(False) == []                                 # nothing was queued
    assert np.all(label.cpu().numpy() == SENTINEL)
    assert call() == 0                                         # the same arguments, unbroken, go through
    torch.cuda.synchronize()
    assert not np.any(label.cpu().numpy() == SENTINEL)
