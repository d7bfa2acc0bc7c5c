"""CPU checks of the entry points behind bcnn_set_loader_detection_on_device: the three public
functions are declared exactly once in include/bcnn/bcnn.h and exported by the built libbcnn.so; the C-ABI entry behind
them is declared once in include/bcnn_hip.h, defined once in bcnn_amd/csrc/augment.hip, listed in _lib.SIGNATURES and
exported by libbcnn_hip.so; capi.Net has the three methods and ops.py the wrapper; the setter's statuses; the [net] key
sets the flag in both config dialects; the counter of a fresh net is 0. The switches that were there keep their own
flags."""
import ctypes as C
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "bcnn_hip_augment_letterbox_batch"


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
    assert len(re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_set_loader_detection_on_device\s*\(\s*bcnn_net\s*\*\s*net\s*,"
                          r"\s*int\s+on\s*\)\s*;", text)) == 1
    assert len(re.findall(r"BCNN_API\s+int\s+bcnn_get_loader_detection_on_device\s*\(\s*const\s+bcnn_net\s*\*\s*net\s*\)\s*;",
                          text)) == 1
    assert len(re.findall(r"BCNN_API\s+int\s+bcnn_get_loader_device_letterboxed\s*\(\s*const\s+bcnn_net\s*\*\s*net\s*\)\s*;",
                          text)) == 1
    names = ("bcnn_set_loader_detection_on_device", "bcnn_get_loader_detection_on_device",
             "bcnn_get_loader_device_letterboxed")
    assert os.path.exists(capi.LIB_PATH), "run __graft_entry__.build() first"
    lib = C.CDLL(capi.LIB_PATH)
    for name in names:
        assert len(re.findall(r"\b%s\b" % name, text)) == 1, name
        assert hasattr(lib, name), name
    for method in ("set_loader_detection_on_device", "get_loader_detection_on_device", "loader_device_letterboxed"):
        assert callable(getattr(capi.Net, method)), method


def test_cabi_entry_is_declared_once_and_defined_once():
    from bcnn_amd import _lib, ops
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    sources = {os.path.basename(p): _no_comments(open(p).read())
               for p in glob.glob(os.path.join(ROOT, "bcnn_amd", "csrc", "*.hip"))}
    assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % ENTRY, header)) == 1
    assert len(re.findall(r"typedef\s+struct\s+bcnn_hip_letterbox_image\s*\{", header)) == 1
    fields = re.search(r"typedef\s+struct\s+bcnn_hip_letterbox_image\s*\{(.*?)\}\s*bcnn_hip_letterbox_image\s*;", header, re.S)
    assert re.sub(r"\s+", " ", fields.group(1)).strip() == ("const uint8_t *pixels; int32_t w, h; int32_t new_w, new_h; "
                                                            "int32_t x_off, y_off;")
    defined = [fn for fn, text in sources.items()
               for _ in re.findall(r"^[A-Za-z_][\w \*]*\b%s\s*\([^;{]*\)\s*\{" % ENTRY, text, flags=re.M)]
    assert defined == ["augment.hip"], defined
    assert len(re.findall(r"\baugment_letterbox_kernel\b[^;{]*\{", sources["augment.hip"])) == 1   # one kernel, templated
    assert len(_lib.SIGNATURES[ENTRY][1]) == 10
    assert ENTRY in _lib.declared_symbols()
    assert hasattr(C.CDLL(_lib.LIB_PATH), ENTRY)
    assert callable(ops.augment_letterbox_batch)
    assert C.sizeof(ops.LetterboxImage) == 32                     # a pointer and six int32
    # the siblings it stands beside are what they were
    assert len(_lib.SIGNATURES["bcnn_hip_augment_batch"][1]) == 12
    assert len(_lib.SIGNATURES["bcnn_hip_augment_jpeg_run"][1]) == 7


def test_setter_statuses_without_a_device():
    from bcnn_amd import capi
    L = capi.lib()
    assert L.bcnn_set_loader_detection_on_device(None, 1) == 1   # BCNN_INVALID_PARAMETER
    assert L.bcnn_get_loader_detection_on_device(None) == 0
    assert L.bcnn_get_loader_device_letterboxed(None) == 0
    net = _fresh_net(capi.MODE_TRAIN)
    assert net.get_loader_detection_on_device() == 0             # off by default
    assert net.loader_device_letterboxed() == 0                  # fresh net
    assert net.set_loader_detection_on_device(True) == 0 and net.get_loader_detection_on_device() == 1   # no loader: accepted
    assert net.set_loader_detection_on_device(False) == 0 and net.get_loader_detection_on_device() == 0
    assert L.bcnn_set_loader_detection_on_device(net.net, 7) == 0 and net.get_loader_detection_on_device() == 1
    assert L.bcnn_set_loader_detection_on_device(net.net, -3) == 0 and net.get_loader_detection_on_device() == 1
    assert net.get_loader_on_device() == 0 and net.get_loader_decode_on_device() == 0   # the other switches are their own
    assert net.loader_device_letterboxed() == 0 and net.loader_device_decoded() == 0


def _flags_after_load(tmp_path, text, mode):
    p = tmp_path / "c.conf"
    p.write_text(text)
    net = _fresh_net(mode)
    assert net.get_loader_detection_on_device() == 0
    assert net.L.bcnn_load_net(net.net, str(p).encode(), None) == 0
    return net.get_loader_detection_on_device(), net.get_loader_on_device(), net.get_loader_decode_on_device()


def test_net_key_sets_the_flag(tmp_path):
    """a config of a [net] section alone builds no layer and so needs no device; the INI dialect ([net] with input_width)
    and the Darknet one ([net] / [network] with width) read the section through the same function"""
    from bcnn_amd import capi
    ini = "batch_size=2\ninput_width=4\ninput_height=4\ninput_channels=1\n"
    darknet = "batch=2\nwidth=4\nheight=4\nchannels=1\n"
    for mode in (capi.MODE_TRAIN, capi.MODE_PREDICT):
        for head, keys in (("[net]\n", ini), ("[net]\n", darknet), ("[network]\n", darknet)):
            assert _flags_after_load(tmp_path, head + keys + "loader_detection_on_device=1\n", mode) == (1, 0, 0)
            assert _flags_after_load(tmp_path, head + "loader_detection_on_device = 1\nloader_on_device=1\n" + keys,
                                     mode) == (1, 1, 0)
            assert _flags_after_load(tmp_path, head + keys + "loader_detection_on_device=5\n", mode) == (1, 0, 0)
            assert _flags_after_load(tmp_path, head + keys + "loader_detection_on_device=0\n", mode) == (0, 0, 0)
            assert _flags_after_load(tmp_path, head + keys + "loader_decode_on_device=1\nloader_on_device=1\n", mode) == (0, 1, 1)
            assert _flags_after_load(tmp_path, head + keys, mode) == (0, 0, 0)
