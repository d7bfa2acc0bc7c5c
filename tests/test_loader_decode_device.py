"""Device decoding of the list loaders' JPEG entries (bcnn_set_loader_decode_on_device): with
bcnn_set_loader_on_device and this switch, the host parses headers and entropy-decodes, and the device does inverse DCT,
upsampling, colour conversion, the crop to the net input (a window the geometry kernel reads through), augmentation and
conversion. The bar is np.array_equal on inputs, labels and the next value of rand(), against

  (a) this build's host path (both switches off): same files, same srand() seed -- always;
  (b) the unmodified reference (oracle/_ref) where present, for lists of well-formed, missing and grey files only (it
      aborts on some corrupted entropy streams).

Net inputs are 16 x 16, 17 x 23 (width no multiple of 4) and 13 x 11 x 1; the fixtures of tests/golden/jpeg are larger,
equal, wider-but-shorter and smaller than those, so every branch of the window rule and of the crop-origin draws runs.
bcnn_get_loader_device_decoded tells, batch by batch, that the path ran."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ref_bind as rb
from tests import _jpeg_fixtures as J
from tests import test_loader_device as tld
from tests.test_data_loader import LIB, _augment, _next, _set_loader, _u8, _write_mnist, libc
from tests.test_loader_device import TRAIN, VALID, _close, _play, _same, _trio

pytestmark = pytest.mark.gpu

COLOUR = [row[0] for row in J.manifest() if row[3] == 3]
GREY = [row[0] for row in J.manifest() if row[3] == 1]
SCRIPT = [(TRAIN, 6), (VALID, 2), (TRAIN, 1)]
EVERY_STAGE = dict(flip=(1, 0), shift=(3, 2), scale=(0.8, 1.2), rotation=20.0, color=(-10, 30, 0.7, 1.3))


def _fixture(name):
    return os.path.join(J.DIR, name)


def _png(tmp_path):
    bip = C.CDLL(os.path.join(LIB, "libbip.so"))
    img = np.random.RandomState(8).randint(0, 256, (20, 24, 3)).astype(np.uint8)
    p = str(tmp_path / "host_decoded.png")
    assert bip.bip_write_image(p.encode(), _u8(img), 24, 20, 3, 24 * 3) == 0
    return p


def _corrupted(tmp_path):
    """two copies of y420_70x61.jpg: `header` fails in bip_jpeg_frame_info (its SOF segment is cut after the 6th byte),
    `scan` passes it and fails in bip_jpeg_read_coefficients (the first scan names a component the frame does not have)"""
    data = J.read("y420_70x61.jpg")
    sof, sos = data.index(b"\xff\xc0"), data.index(b"\xff\xda")
    header = data[:sof + 6]
    scan = bytearray(data)
    scan[sos + 5] = 9
    scan = bytes(scan)
    assert J.frame_info(header)[0] != 0 and J.host_decode(header)[0] != 0
    st, info = J.frame_info(scan)
    assert st == 0 and J.read_coefficients(scan, info)[0] != 0 and J.host_decode(scan)[0] != 0
    out = []
    for name, blob in (("bad_header.jpg", header), ("bad_scan.jpg", scan)):
        p = tmp_path / name
        p.write_bytes(blob)
        out.append(str(p))
    return out


def _plain_entries(tmp_path):
    """[(path, components of a well-formed JPEG or 0)]: the 15 colour fixtures with the two grey ones, a PNG and a
    missing path in between"""
    col = [(_fixture(n), 3) for n in COLOUR]
    grey = [(_fixture(n), 1) for n in GREY]
    return col[:4] + grey[:1] + col[4:7] + [(_png(tmp_path), 0)] + col[7:11] + [(str(tmp_path / "missing.jpg"), 0)] + \
        col[11:13] + grey[1:] + col[13:]


def _failing_entries(tmp_path):
    """the same files with the two corrupted streams (A: header, B: scan) first in the list, directly after a
    device-decoded sample, twice in a row inside a batch and across two batches of 4, and first in a batch whose
    predecessor ended on a device-decoded sample"""
    plain = _plain_entries(tmp_path)
    col = [e for e in plain if e[1] == 3]
    rest = [e for e in plain if e[1] != 3]
    a, b = [(p, 0) for p in _corrupted(tmp_path)]
    return [a, col[0], col[1], b,              # first in the list; after a device-decoded sample; last in its batch
            a, col[2], col[3], col[4],         # ... and the next batch starts on a failure; ends on a device sample
            b, a, col[5], col[6],              # first in a batch behind a device-decoded sample; twice in a row
            rest[0], col[7], rest[1], b,       # grey, colour, PNG, failure behind a host-decoded sample
            col[8], rest[2], col[9], col[10],  # a missing file in the middle
            col[11], col[12], rest[3], col[13],
            col[14]]


def _write_lists(tmp_path, entries):
    rs = np.random.RandomState(4)
    (tmp_path / "c.txt").write_text("".join("%s %d\n" % (p, k % 4) for k, (p, _) in enumerate(entries)))
    (tmp_path / "r.txt").write_text("".join("%s %.3f %.3f %.3f\n" % (p, *rs.uniform(-1, 1, 3)) for p, _ in entries))


def _expected_counts(entries, script, batch, channels):
    """device-decoded samples per batch: the train stream goes on where it was, the test stream restarts with the mode"""
    out, train_at = [], 0
    for mode, batches in script:
        at = train_at if mode == TRAIN else 0
        for _ in range(batches):
            out.append(sum(entries[(at + k) % len(entries)][1] == channels for k in range(batch)))
            at += batch
        if mode == TRAIN:
            train_at = at
    return out


def _nets(w, h, c, n, classes, with_ref=True):
    """_trio with the decode switch on the first net as well"""
    nets = _trio(w, h, c, n, classes, with_ref=with_ref)
    assert nets[0].set_loader_decode_on_device(True) == 0 and nets[0].get_loader_decode_on_device() == 1
    assert nets[1].get_loader_decode_on_device() == 0
    return nets


def _load(nets, tmp_path, kind=2, **augment):
    path = str(tmp_path / ("c.txt" if kind == 2 else "r.txt"))
    for n in nets:
        assert _set_loader(n, kind, path, None, path, None) == 0
        _augment(n, **augment)
        n.compile()


@pytest.fixture
def counters(monkeypatch):
    """what bcnn_get_loader_device_decoded said after every batch that _play ran, per net"""
    seen = {}
    dev_next, host_next = tld._dev_next, tld._next

    def counted(fn):
        def run(net):
            out = fn(net)
            if hasattr(net, "loader_device_decoded"):
                seen.setdefault(id(net), []).append(net.loader_device_decoded())
            return out
        return run
    monkeypatch.setattr(tld, "_dev_next", counted(dev_next))
    monkeypatch.setattr(tld, "_next", counted(host_next))
    return seen


@pytest.mark.parametrize("kind,classes", [(2, 4), (3, 3)], ids=["classification", "regression"])
def test_every_fixture(tmp_path, counters, kind, classes):
    entries = _plain_entries(tmp_path)
    assert len(COLOUR) == 15 and len(GREY) == 2 and len(entries) == 19
    _write_lists(tmp_path, entries)
    nets = _nets(16, 16, 3, 4, classes)
    _load(nets, tmp_path, kind, **EVERY_STAGE)
    got = _same(nets, SCRIPT, seed=31)
    want = _expected_counts(entries, SCRIPT, 4, 3)
    assert counters[id(nets[0])] == want and 4 in want and min(want) < 4
    assert counters[id(nets[1])] == [0] * len(want)
    assert len({x.tobytes() for x, _ in got[:6]}) == 6
    _close(nets)


def test_input_width_that_is_no_multiple_of_4(tmp_path, counters):
    """17 x 23 x 3: the scalar head and tail of the stores run, and most fixtures are shorter than the input"""
    entries = _plain_entries(tmp_path)
    _write_lists(tmp_path, entries)
    nets = _nets(17, 23, 3, 3, 4)
    _load(nets, tmp_path, 2, **EVERY_STAGE)
    script = [(TRAIN, 6), (VALID, 2)]
    _same(nets, script, seed=57)
    assert counters[id(nets[0])] == _expected_counts(entries, script, 3, 3)
    _close(nets)


def test_grey_net(tmp_path, counters):
    """13 x 11 x 1: equal extents (no draw), a larger progressive file, and a colour file as the channel mismatch"""
    entries = [(_fixture("grey_13x11.jpg"), 1), (_fixture("prog_grey_19x13.jpg"), 1), (_fixture("y444_8x8.jpg"), 3)]
    _write_lists(tmp_path, entries)
    nets = _nets(13, 11, 1, 2, 4)
    _load(nets, tmp_path, 2, shift=(2, 2), rotation=15.0, color=(-10, 30, 0.7, 1.3))
    script = [(TRAIN, 4), (VALID, 2)]
    _same(nets, script, seed=5)
    want = _expected_counts(entries, script, 2, 1)
    assert counters[id(nets[0])] == want and set(want) == {1, 2}
    _close(nets)


def test_flip_for_real(tmp_path, counters):
    """the flip only happens on a net whose config sets flip_h (bcnn_data.c's header): the window sits below it. The same
    config swaps the planes to B G R."""
    from bcnn_amd import capi
    entries = _plain_entries(tmp_path)
    _write_lists(tmp_path, entries)
    conf = tld.NET_CONF.replace("batch=8", "batch=4").replace("width=32", "width=16").replace("height=32", "height=16")
    keys = "flip_h=1\nswap_to_bgr=1\nrange_shift_x=3\nrange_shift_y=2\nrotation_range=20\n"
    nets = []
    for extra in ("loader_on_device=1\nloader_decode_on_device=1\n", ""):
        cfg = tmp_path / ("net%d.conf" % len(nets))
        cfg.write_text(conf % (keys + extra))
        nets.append(capi.Net.load_net(str(cfg), None, mode=capi.MODE_TRAIN))
    assert [(n.get_loader_on_device(), n.get_loader_decode_on_device()) for n in nets] == [(1, 1), (0, 0)]
    _load(nets, tmp_path, 2, flip=(1, 0))
    _same(nets, [(TRAIN, 5), (VALID, 1)], seed=3)
    assert counters[id(nets[0])] == _expected_counts(entries, [(TRAIN, 5), (VALID, 1)], 4, 3)
    _close(nets)


def test_failures_in_every_position(tmp_path, counters):
    """own host path only. A failed entry shows the previous sample augmented again; where that sample was decoded on the
    device, the loader rebuilds it on the host from the bytes and crop origin it kept."""
    entries = _failing_entries(tmp_path)
    assert len(entries) == 25
    _write_lists(tmp_path, entries)
    for kind, classes in ((2, 4), (3, 3)):
        nets = _nets(16, 16, 3, 4, classes, with_ref=False)
        _load(nets, tmp_path, kind, **EVERY_STAGE)
        _same(nets, SCRIPT, seed=19)
        assert counters.pop(id(nets[0])) == _expected_counts(entries, SCRIPT, 4, 3)
        _close(nets)


def test_toggling_between_batches(tmp_path):
    """(both off) -> (loader_on_device) -> (both on) -> (both on) ... on one net: the batches of a net that never toggled"""
    _write_lists(tmp_path, _failing_entries(tmp_path))
    toggled, host = _nets(16, 16, 3, 4, 4, with_ref=False)
    _load([toggled, host], tmp_path, 2, **EVERY_STAGE)
    cycle = ((False, False), (True, False), (True, True), (True, True))
    script = [(TRAIN, 9), (VALID, 3), (TRAIN, 3)]
    libc.srand(11)
    got, k = [], 0
    for mode, batches in script:
        toggled.L.bcnn_set_mode(toggled.net, mode)
        for _ in range(batches):
            on, decode = cycle[k % len(cycle)]
            assert toggled.set_loader_on_device(on) == 0 and toggled.set_loader_decode_on_device(decode) == 0
            got.append(tld._dev_next(toggled) if on else _next(toggled))
            assert (toggled.loader_device_decoded() > 0) == decode, k
            k += 1
    after = libc.rand()
    want, after_host = _play(host, script, seed=11)
    assert after == after_host
    for k, ((xa, ya), (xb, yb)) in enumerate(zip(got, want)):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb), k
    _close([toggled, host])


def test_thread_count_does_not_matter(tmp_path):
    _write_lists(tmp_path, _failing_entries(tmp_path))
    one, three = _nets(16, 16, 3, 4, 4, with_ref=False)
    assert three.set_loader_on_device(True) == 0 and three.set_loader_decode_on_device(True) == 0
    assert one.set_num_threads(1) == 0 and three.set_num_threads(3) == 0
    _load([one, three], tmp_path, 2, **EVERY_STAGE)
    a, ra = _play(one, SCRIPT, seed=23)
    b, rb_ = _play(three, SCRIPT, seed=23)
    assert ra == rb_
    for k, ((xa, ya), (xb, yb)) in enumerate(zip(a, b)):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb), k
    _close([one, three])


def test_host_copy_of_the_input_is_left_alone(tmp_path):
    _write_lists(tmp_path, _plain_entries(tmp_path))
    dev, host = _nets(16, 16, 3, 4, 4, with_ref=False)
    _load([dev, host], tmp_path, 2, **EVERY_STAGE)
    dev.data(0)[...] = 7.25
    libc.srand(5)
    dev.L.bcnn_loader_next.argtypes = [C.c_void_p]
    assert dev.L.bcnn_loader_next(dev.net) == 0 and dev.loader_device_decoded() == 4
    assert np.all(dev.data(0) == 7.25)                     # not written, and not uploaded over the device's batch
    libc.srand(5)
    want, labels = _next(host)
    assert np.array_equal(dev.data(1), labels)
    dev.download(0, False)
    assert np.array_equal(dev.data(0), want)
    _close([dev, host])


def test_switch_without_loader_on_device(tmp_path, counters):
    _write_lists(tmp_path, _plain_entries(tmp_path))
    alone, host = _nets(16, 16, 3, 4, 4, with_ref=False)
    assert alone.set_loader_on_device(False) == 0 and alone.get_loader_decode_on_device() == 1
    _load([alone, host], tmp_path, 2, **EVERY_STAGE)
    _same([alone, host], SCRIPT, seed=31)
    assert counters[id(alone)] == [0] * 9
    _close([alone, host])


def test_switch_on_an_mnist_loader(tmp_path, counters):
    tr = _write_mnist(tmp_path, "train", 37, seed=1)
    nets = _nets(28, 28, 1, 16, 10, with_ref=False)
    for n in nets:
        assert _set_loader(n, 0, tr[0], tr[1], tr[0], tr[1]) == 0
        _augment(n, shift=(5, 5), rotation=30.0)
        n.compile()
    _same(nets, [(TRAIN, 3), (VALID, 1)], seed=123)
    assert counters[id(nets[0])] == [0] * 4
    _close(nets)


def test_switch_on_a_detection_list_loader(tmp_path):
    """stage_begin refuses the detection list, so the batch is the host's whatever the two switches say"""
    from bcnn_amd import capi
    from tests.test_detection_loader import CONFIG
    from tests.test_detection_loader import _set_loader as set_detection_loader
    rs = np.random.RandomState(2)
    lst = tmp_path / "det.txt"
    lst.write_text("".join("%s %d %.4f %.4f %.4f %.4f\n" % (_fixture(n), rs.randint(2), *rs.uniform(0.2, 0.8, 2),
                                                          *rs.uniform(0.1, 0.4, 2)) for n in COLOUR[:6]))
    nets = []
    for extra in ("loader_on_device=1\nloader_decode_on_device=1\n", ""):
        cfg = tmp_path / ("det%d.cfg" % len(nets))
        cfg.write_text(CONFIG.replace("train_detector=1\n", "train_detector=1\n" + extra))
        net = capi.Net.load_net(str(cfg), None, mode=capi.MODE_TRAIN)
        assert set_detection_loader(net, str(lst), str(lst)) == 0
        net.compile()
        nets.append(net)
    assert nets[0].get_loader_on_device() == 1 and nets[0].get_loader_decode_on_device() == 1
    runs = []
    for net in nets:
        libc.srand(9)
        batches = []
        for _ in range(3):
            batches.append(_next(net))
            assert net.loader_device_decoded() == 0
        runs.append((batches, libc.rand()))
    assert runs[0][1] == runs[1][1]
    for (xa, ya), (xb, yb) in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
    _close(nets)
