"""CPU checks of the entry points behind bcnn_set_loader_decode_on_device: the three public
functions are declared exactly once in include/bcnn/bcnn.h and exported by the built libbcnn.so; the C-ABI entry points
behind them are declared once in include/bcnn_hip.h, defined once in bcnn_amd/csrc/augment.hip, listed in _lib.SIGNATURES
and exported by libbcnn_hip.so; capi.Net has the three methods; the setter's statuses; the [net] key sets the flag; the
counter of a fresh net is 0. bcnn_hip_augment_batch keeps its 12 arguments (tests/test_loader_device_abi.py pins them)."""
import ctypes as C
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CABI = {"bcnn_hip_augment_jpeg_begin": 7, "bcnn_hip_augment_jpeg_run": 7, "bcnn_hip_augment_jpeg_cancel": 0}


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def _fresh_net(mode):
    """a net without layers needs no device"""
    from bcnn_amd import capi
    net = capi.Net.__new__(capi.Net)
    net.L, net.net = capi.lib(), C.c_void_p()
    assert net.L.bcnn_init_net(C.byref(net.net), mode) == 0
    net.L.bcnn_set_log_context(net.net, None, 4)
    return net


def test_public_functions_are_declared_once_and_exported():
    from bcnn_amd import capi
    text = _no_comments(open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read())
    assert len(re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_set_loader_decode_on_device\s*\(\s*bcnn_net\s*\*\s*net\s*,\s*int\s+on"
                          r"\s*\)\s*;", text)) == 1
    assert len(re.findall(r"BCNN_API\s+int\s+bcnn_get_loader_decode_on_device\s*\(\s*const\s+bcnn_net\s*\*\s*net\s*\)\s*;",
                          text)) == 1
    assert len(re.findall(r"BCNN_API\s+int\s+bcnn_get_loader_device_decoded\s*\(\s*const\s+bcnn_net\s*\*\s*net\s*\)\s*;",
                          text)) == 1
    names = ("bcnn_set_loader_decode_on_device", "bcnn_get_loader_decode_on_device", "bcnn_get_loader_device_decoded")
    assert os.path.exists(capi.LIB_PATH), "run __graft_entry__.build() first"
    lib = C.CDLL(capi.LIB_PATH)
    for name in names:
        assert len(re.findall(r"\b%s\b" % name, text)) == 1, name
        assert hasattr(lib, name), name
    for method in ("set_loader_decode_on_device", "get_loader_decode_on_device", "loader_device_decoded"):
        assert callable(getattr(capi.Net, method)), method


def test_cabi_entry_points_are_declared_once_and_defined_once():
    from bcnn_amd import _lib
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    sources = {os.path.basename(p): _no_comments(open(p).read())
               for p in glob.glob(os.path.join(ROOT, "bcnn_amd", "csrc", "*.hip"))}
    lib = C.CDLL(_lib.LIB_PATH)
    for name, nargs in CABI.items():
        assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1, name
        defined = [fn for fn, text in sources.items()
                   for _ in re.findall(r"^[A-Za-z_][\w \*]*\b%s\s*\([^;{]*\)\s*\{" % name, text, flags=re.M)]
        assert defined == ["augment.hip"], (name, defined)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert name in _lib.declared_symbols()
        assert hasattr(lib, name), name
    # the siblings they stand beside are where and what they were
    assert len(_lib.SIGNATURES["bcnn_hip_augment_batch"][1]) == 12
    assert len(_lib.SIGNATURES["bcnn_hip_jpeg_stage_begin"][1]) == 9
    host = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libbcnn.so"))
    assert hasattr(host, "bcnn_jpeg_read_batch") and hasattr(host, "bcnn_jpeg_read_batch_each")


def test_setter_statuses_without_a_device():
    from bcnn_amd import capi
    L = capi.lib()
    assert L.bcnn_set_loader_decode_on_device(None, 1) == 1   # BCNN_INVALID_PARAMETER
    assert L.bcnn_get_loader_decode_on_device(None) == 0
    assert L.bcnn_get_loader_device_decoded(None) == 0
    net = _fresh_net(capi.MODE_TRAIN)
    assert net.get_loader_decode_on_device() == 0             # off by default
    assert net.loader_device_decoded() == 0                   # fresh net
    assert net.set_loader_decode_on_device(True) == 0 and net.get_loader_decode_on_device() == 1   # no loader: accepted
    assert net.set_loader_decode_on_device(False) == 0 and net.get_loader_decode_on_device() == 0
    assert L.bcnn_set_loader_decode_on_device(net.net, 7) == 0 and net.get_loader_decode_on_device() == 1
    assert net.get_loader_on_device() == 0                    # the other switch is its own
    assert net.loader_device_decoded() == 0


def _flag_after_load(tmp_path, text, mode):
    p = tmp_path / "c.conf"
    p.write_text(text)
    net = _fresh_net(mode)
    assert net.get_loader_decode_on_device() == 0
    assert net.L.bcnn_load_net(net.net, str(p).encode(), None) == 0
    return net.get_loader_decode_on_device(), net.get_loader_on_device()


def test_net_key_sets_the_flag(tmp_path):
    """a config of a [net] section alone builds no layer and so needs no device; both dialects read the section through
    the same function"""
    from bcnn_amd import capi
    keys = "batch=2\nwidth=4\nheight=4\nchannels=1\n"
    for mode in (capi.MODE_TRAIN, capi.MODE_PREDICT):
        for head in ("[net]\n", "[network]\n"):
            assert _flag_after_load(tmp_path, head + keys + "loader_decode_on_device=1\n", mode) == (1, 0)
            assert _flag_after_load(tmp_path, head + "loader_decode_on_device = 1\nloader_on_device=1\n" + keys, mode) == (1, 1)
            assert _flag_after_load(tmp_path, head + keys + "loader_decode_on_device=0\n", mode) == (0, 0)
            assert _flag_after_load(tmp_path, head + keys + "loader_on_device=1\n", mode) == (0, 1)
            assert _flag_after_load(tmp_path, head + keys, mode) == (0, 0)


def test_per_image_staging_reports_every_status_for_any_thread_count():
    """bcnn_jpeg_read_batch_each on a plain heap block: a status per image, images without a destination skipped, the
    same bytes for 1, 3 and more threads than images; bcnn_jpeg_read_batch still reports the lowest failure only"""
    import numpy as np
    from bcnn_amd import capi
    from tests import _jpeg_fixtures as J
    L = C.CDLL(capi.LIB_PATH)
    L.bcnn_jpeg_read_batch_each.restype = L.bcnn_jpeg_read_batch.restype = C.c_int
    names = ["y420_70x61.jpg", "prog_y420_27x21.jpg", "grey_13x11.jpg", "y411_33x18.jpg", "y420_1x1.jpg",
             "restart_y420_40x24.jpg"]
    datas = [J.read(n) for n in names]
    k = len(datas)
    infos = (J.Info * k)(*[J.frame_info(d)[1] for d in datas])
    datas[1] = datas[1][:len(datas[1]) // 2]                 # cut short: fails
    datas[5] = datas[5][:len(datas[5]) - 30]                 # fails too
    skipped = 3                                              # no destination: not touched, status kept
    offs = np.cumsum([0] + [infos[b].num_coefficients for b in range(k)])
    bufs = (C.c_char_p * k)(*datas)
    lens = (C.c_size_t * k)(*[len(d) for d in datas])

    def run(threads):
        block = np.full(int(offs[-1]) + 2 * J.GUARD, 0x5a5a, np.int16)
        base = block[J.GUARD:].ctypes.data
        ptrs = (C.c_void_p * k)(*[None if b == skipped else base + 2 * int(offs[b]) for b in range(k)])
        status = (C.c_int * k)(*([-7] * k))
        assert L.bcnn_jpeg_read_batch_each(k, bufs, lens, infos, ptrs, threads, status) == 0
        assert (block[:J.GUARD] == 0x5a5a).all() and (block[-J.GUARD:] == 0x5a5a).all()
        return list(status), block

    s1, one = run(1)
    s3, three = run(3)
    s99, many = run(99)
    assert s1 == s3 == s99 == [1, 0, 1, -7, 1, 0]
    assert np.array_equal(one, three) and np.array_equal(one, many)
    assert (one[J.GUARD + int(offs[skipped]):J.GUARD + int(offs[skipped + 1])] == 0x5a5a).all()
    for b in (0, 2, 4):
        _, want = J.read_coefficients(datas[b], infos[b])
        assert np.array_equal(one[J.GUARD + int(offs[b]):J.GUARD + int(offs[b + 1])], want), names[b]
    assert L.bcnn_jpeg_read_batch_each(k, bufs, lens, infos, None, 1, None) == -2   # nowhere to report to
