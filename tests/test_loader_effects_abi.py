"""CPU checks of the entry points of the loader's effects switch (bcnn_set_loader_effects): the two
public functions are declared exactly once in include/bcnn/bcnn.h and exported by the built libbcnn.so; the C-ABI entry
that stages the effects of the next batch and its cancel are declared once in include/bcnn_hip.h, defined once in
bcnn_amd/csrc/augment.hip, listed in _lib.SIGNATURES and exported by libbcnn_hip.so; the batch entry keeps its 12 arguments
and the record its eight members; capi.Net has the two methods; the [net] key sets the flag in both dialects; the
per-pixel rule of the two effects has one definition, which libbip and augment.hip include."""
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
    assert len(re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_set_loader_effects\s*\(\s*bcnn_net\s*\*\s*net\s*,\s*int\s+on\s*\)\s*;",
                          text)) == 1
    assert len(re.findall(r"BCNN_API\s+int\s+bcnn_get_loader_effects\s*\(\s*const\s+bcnn_net\s*\*\s*net\s*\)\s*;", text)) == 1
    for name in ("bcnn_set_loader_effects", "bcnn_get_loader_effects"):
        assert len(re.findall(r"\b%s\b" % name, text)) == 1, name
    assert os.path.exists(capi.LIB_PATH), "run __graft_entry__.build() first"
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "bcnn_set_loader_effects") and hasattr(lib, "bcnn_get_loader_effects")
    assert callable(getattr(capi.Net, "set_loader_effects")) and callable(getattr(capi.Net, "get_loader_effects"))
    bip = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libbip.so"))
    bip_h = _no_comments(open(os.path.join(ROOT, "include", "bip", "bip.h")).read())
    for name in ("bip_image_perlin_distortion", "bip_add_random_spotlights", "bip_perlin_distortion_seeded",
                 "bip_add_spotlights", "bip_perlin_axis", "bip_spot_table", "bip_apply_spot_table"):
        assert hasattr(bip, name), name
        assert len(re.findall(r"\b%s\s*\(" % name, bip_h)) == 1, name


def test_cabi_entry_points_are_declared_once_and_defined_once():
    from bcnn_amd import _lib
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    sources = {os.path.basename(p): _no_comments(open(p).read())
               for p in glob.glob(os.path.join(ROOT, "bcnn_amd", "csrc", "*.hip"))}
    assert len(sources) > 20
    for name, nargs in (("bcnn_hip_augment_effects_begin", 10), ("bcnn_hip_augment_effects_cancel", 0)):
        assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1, name
        defined = [fn for fn, text in sources.items()
                   for _ in re.findall(r"^[A-Za-z_][\w \*]*\b%s\s*\([^;{]*\)\s*\{" % name, text, flags=re.M)]
        assert defined == ["augment.hip"], (name, defined)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert name in _lib.declared_symbols()
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    for struct in ("bcnn_hip_augment_effect", "bcnn_hip_augment_spot"):
        assert len(re.findall(r"typedef\s+struct\s+%s\s*\{[^}]*\}\s*%s\s*;" % (struct, struct), header)) == 1
    flags = dict(re.findall(r"#define\s+(BCNN_HIP_AUG_\w+)\s+(\d+)", header))
    assert flags["BCNN_HIP_AUG_DISTORT"] == "32" and flags["BCNN_HIP_AUG_SPOTS"] == "64"
    assert len(set(flags.values())) == len(flags) == 7                 # seven distinct bits


def test_existing_batch_entries_keep_their_shape():
    from bcnn_amd import _lib
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    assert len(_lib.SIGNATURES["bcnn_hip_augment_batch"][1]) == 12
    decl = re.search(r"\bbcnn_hip_augment_batch\s*\(([^;{]*)\)\s*;", header).group(1)
    assert len(decl.split(",")) == 12
    assert len(_lib.SIGNATURES["bcnn_hip_augment_jpeg_run"][1]) == 7
    assert len(_lib.SIGNATURES["bcnn_hip_augment_letterbox_batch"][1]) == 10
    record = re.search(r"typedef\s+struct\s+bcnn_hip_augment_record\s*\{([^}]*)\}", header).group(1)
    members = re.findall(r"\b(\w+)\s*[,;]", record)
    assert members == ["flags", "x_ul", "y_ul", "ca", "sa", "gain", "brightness", "reserved"], members
    assert "int32_t" in record and "float" not in record               # 8 x 4 bytes, as before


def _flag_after_load(tmp_path, text, mode):
    from bcnn_amd import capi
    p = tmp_path / "c.conf"
    p.write_text(text)
    net = capi.Net.__new__(capi.Net)
    net.L, net.net = capi.lib(), C.c_void_p()
    assert net.L.bcnn_init_net(C.byref(net.net), mode) == 0
    net.L.bcnn_set_log_context(net.net, None, 4)
    assert net.get_loader_effects() == 0                   # off by default
    assert net.L.bcnn_load_net(net.net, str(p).encode(), None) == 0
    return net.get_loader_effects(), net.get_loader_on_device()


def test_net_key_sets_the_flag(tmp_path):
    """a config of a [net] section alone builds no layer and so needs no device; both dialects read the section through
    the function that reads loader_on_device, of which the switch is independent"""
    from bcnn_amd import capi
    keys = "batch=2\nwidth=4\nheight=4\nchannels=1\nmax_distortion=0.3\nmax_spots=3\n"
    for mode in (capi.MODE_TRAIN, capi.MODE_PREDICT):
        for head in ("[net]\n", "[network]\n"):
            assert _flag_after_load(tmp_path, head + keys + "loader_effects=1\n", mode) == (1, 0)
            assert _flag_after_load(tmp_path, head + "loader_effects = 1\n" + keys, mode) == (1, 0)
            assert _flag_after_load(tmp_path, head + keys + "loader_effects=1\nloader_on_device=1\n", mode) == (1, 1)
            assert _flag_after_load(tmp_path, head + keys + "loader_effects=0\nloader_on_device=1\n", mode) == (0, 1)
            assert _flag_after_load(tmp_path, head + keys, mode) == (0, 0)
    source = _no_comments(open(os.path.join(ROOT, "bcnn_amd", "host", "bcnn_config.c")).read())
    body = re.search(r"static\s+void\s+net_set_param\s*\([^)]*\)\s*\{(.*?)\n\}", source, flags=re.S).group(1)
    assert '"loader_on_device"' in body and '"loader_effects"' in body


def test_setter_statuses_without_a_device():
    from bcnn_amd import capi
    L = capi.lib()
    assert L.bcnn_set_loader_effects(None, 1) == 1         # BCNN_INVALID_PARAMETER
    assert L.bcnn_get_loader_effects(None) == 0
    net = capi.Net.__new__(capi.Net)
    net.L, net.net = L, C.c_void_p()
    assert L.bcnn_init_net(C.byref(net.net), capi.MODE_TRAIN) == 0
    assert net.get_loader_effects() == 0
    assert net.set_loader_effects(True) == 0 and net.get_loader_effects() == 1     # no loader yet: accepted
    assert net.get_loader_on_device() == 0                                         # and no other switch moves
    assert net.set_loader_effects(False) == 0 and net.get_loader_effects() == 0
    assert L.bcnn_set_loader_effects(net.net, 7) == 0 and net.get_loader_effects() == 1


def test_effect_arithmetic_has_one_definition():
    """bip_effects.c (the host functions) and augment.hip (the convert kernel of a batch with effects) include the same
    header; no other file of the tree restates the lattice hash, the position map, the blend or the spot's sum"""
    host, csrc = os.path.join(ROOT, "bcnn_amd", "host"), os.path.join(ROOT, "bcnn_amd", "csrc")
    files = glob.glob(os.path.join(host, "*.[ch]")) + glob.glob(os.path.join(csrc, "*.hip")) + \
        glob.glob(os.path.join(csrc, "*.h"))
    for rule in ("bip_perlin_lattice", "bip_perlin_noise", "bip_distort_map", "bip_distort_blend", "bip_spot_exponent",
                 "bip_spot_add"):
        owners = [os.path.basename(p) for p in files
                  if re.search(r"^[A-Za-z_][\w \*]*\b%s\s*\([^;{]*\)\s*\{" % rule, _no_comments(open(p).read()), flags=re.M)]
        assert owners == ["bip_effects.h"], (rule, owners)
    for user in (os.path.join(csrc, "augment.hip"), os.path.join(host, "bip_effects.c")):
        assert re.search(r'#include\s+"[./a-z]*bip_effects\.h"', open(user).read()), user
    kernel = _no_comments(open(os.path.join(csrc, "augment.hip")).read())
    for rule in ("bip_perlin_noise(", "bip_distort_map(", "bip_distort_blend(", "bip_spot_add("):
        assert rule in kernel, rule
    for build_file in (os.path.join("bcnn_amd", "csrc", "Makefile"), "CMakeLists.txt"):
        text = open(os.path.join(ROOT, build_file)).read()
        assert "-ffp-contract=off" in text and "bip_effects.h" in text, build_file
