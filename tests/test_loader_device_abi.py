"""CPU checks of the device loader path's entry points (bcnn_set_loader_on_device): the two public
functions are declared exactly once in include/bcnn/bcnn.h and exported by the built libbcnn.so; the C-ABI entry point
behind them is declared once in include/bcnn_hip.h, defined once in bcnn_amd/csrc/augment.hip, listed in _lib.SIGNATURES,
exported by libbcnn_hip.so and named in both build files; capi.Net has the two methods; the [net] key sets the flag; the
resize sampling rule still has one definition, which augment.hip and the loader include."""
import ctypes as C
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def test_public_functions_are_declared_once_and_exported():
    from bcnn_amd import capi
    text = _no_comments(open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read())
    assert len(re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_set_loader_on_device\s*\(\s*bcnn_net\s*\*\s*net\s*,\s*int\s+on\s*\)\s*;",
                          text)) == 1
    assert len(re.findall(r"BCNN_API\s+int\s+bcnn_get_loader_on_device\s*\(\s*const\s+bcnn_net\s*\*\s*net\s*\)\s*;", text)) == 1
    for name in ("bcnn_set_loader_on_device", "bcnn_get_loader_on_device"):
        assert len(re.findall(r"\b%s\b" % name, text)) == 1, name
    assert os.path.exists(capi.LIB_PATH), "run __graft_entry__.build() first"
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "bcnn_set_loader_on_device") and hasattr(lib, "bcnn_get_loader_on_device")
    assert callable(getattr(capi.Net, "set_loader_on_device")) and callable(getattr(capi.Net, "get_loader_on_device"))


def test_cabi_entry_point_is_declared_once_and_defined_once():
    from bcnn_amd import _lib
    name = "bcnn_hip_augment_batch"
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    sources = {os.path.basename(p): _no_comments(open(p).read())
               for p in glob.glob(os.path.join(ROOT, "bcnn_amd", "csrc", "*.hip"))}
    assert len(sources) > 20
    assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1
    assert len(re.findall(r"typedef\s+struct\s+bcnn_hip_augment_record\s*\{[^}]*\}\s*bcnn_hip_augment_record\s*;", header)) == 1
    defined = [fn for fn, text in sources.items()
               for _ in re.findall(r"^[A-Za-z_][\w \*]*\b%s\s*\([^;{]*\)\s*\{" % name, text, flags=re.M)]
    assert defined == ["augment.hip"], defined
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 12
    assert name in _lib.declared_symbols()
    assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    for build_file in (os.path.join("bcnn_amd", "csrc", "Makefile"), "CMakeLists.txt"):
        text = open(os.path.join(ROOT, build_file)).read()
        assert "augment.hip" in text or "${CSRC}/*.hip" in text, build_file


def _flag_after_load(tmp_path, text, mode):
    from bcnn_amd import capi
    p = tmp_path / "c.conf"
    p.write_text(text)
    net = capi.Net.__new__(capi.Net)
    net.L, net.net = capi.lib(), C.c_void_p()
    assert net.L.bcnn_init_net(C.byref(net.net), mode) == 0
    net.L.bcnn_set_log_context(net.net, None, 4)
    assert net.get_loader_on_device() == 0                 # off by default
    assert net.L.bcnn_load_net(net.net, str(p).encode(), None) == 0
    return net.get_loader_on_device()


def test_net_key_sets_the_flag(tmp_path):
    """a config of a [net] section alone builds no layer and so needs no device; both dialects read the section through
    the same function (the Darknet dialect, which a *.weights model selects, is loaded in tests/test_loader_device.py)"""
    from bcnn_amd import capi
    keys = "batch=2\nwidth=4\nheight=4\nchannels=1\n"
    for mode in (capi.MODE_TRAIN, capi.MODE_PREDICT):
        for head in ("[net]\n", "[network]\n"):
            assert _flag_after_load(tmp_path, head + keys + "loader_on_device=1\n", mode) == 1
            assert _flag_after_load(tmp_path, head + "loader_on_device = 1\n" + keys, mode) == 1
            assert _flag_after_load(tmp_path, head + keys + "loader_on_device=0\n", mode) == 0
            assert _flag_after_load(tmp_path, head + keys, mode) == 0


def test_setter_statuses_without_a_device():
    from bcnn_amd import capi
    L = capi.lib()
    assert L.bcnn_set_loader_on_device(None, 1) == 1       # BCNN_INVALID_PARAMETER
    net = capi.Net.__new__(capi.Net)
    net.L, net.net = L, C.c_void_p()
    assert L.bcnn_init_net(C.byref(net.net), capi.MODE_TRAIN) == 0
    assert net.set_loader_on_device(True) == 0 and net.get_loader_on_device() == 1   # no loader yet: accepted
    assert net.set_loader_on_device(False) == 0 and net.get_loader_on_device() == 0
    assert net.set_loader_on_device(7) == 0 and net.get_loader_on_device() == 1


def test_resize_sampling_rule_still_has_one_definition():
    """bip_min.c (the host resize), image_fill.hip, and now the loader (which tabulates the taps of the scale stage) and
    augment.hip (whose kernel blends with them) include the same header; no file of the tree restates the rule"""
    host, csrc = os.path.join(ROOT, "bcnn_amd", "host"), os.path.join(ROOT, "bcnn_amd", "csrc")
    files = glob.glob(os.path.join(host, "*.[ch]")) + glob.glob(os.path.join(csrc, "*.hip")) + \
        glob.glob(os.path.join(csrc, "*.h"))
    taps = [os.path.basename(p) for p in files
            if re.search(r"\bvoid\s+\w*resize_tap\s*\([^;{]*\)\s*\{", _no_comments(open(p).read()))]
    blends = [os.path.basename(p) for p in files
              if re.search(r"\b\w*resize_blend\s*\([^;{]*\)\s*\{", _no_comments(open(p).read()))]
    assert taps == ["bip_resize_tap.h"] and blends == ["bip_resize_tap.h"], (taps, blends)
    aug = open(os.path.join(csrc, "augment.hip")).read()
    assert "bip_resize_blend(" in _no_comments(aug)        # it resizes ...
    for user in (os.path.join(csrc, "augment.hip"), os.path.join(host, "bcnn_data.c")):
        assert re.search(r'#include\s+"[./a-z]*bip_resize_tap\.h"', open(user).read()), user   # ... by the shared rule
