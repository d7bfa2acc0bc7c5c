"""CPU checks of the batched input fill's entry points: bcnn_fill_tensor_with_images and the bcnn_image_fit enum are
declared exactly once in include/bcnn/bcnn.h and the function is exported by the built libbcnn.so; the C-ABI entry point
behind it is declared once in include/bcnn_hip.h, defined once in bcnn_amd/csrc/image_fill.hip, listed in _lib.SIGNATURES
and exported by libbcnn_hip.so; the resize sampling rule has one definition, which both users include."""
import ctypes
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def test_public_function_and_enum_are_declared_once_and_exported():
    from bcnn_amd import capi
    text = _no_comments(open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read())
    assert len(re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_fill_tensor_with_images\s*\(", text)) == 1
    assert len(re.findall(r"\bbcnn_fill_tensor_with_images\b", text)) == 1
    enums = re.findall(r"typedef\s+enum\s*\{([^}]*)\}\s*bcnn_image_fit\s*;", text)
    assert len(enums) == 1 and len(re.findall(r"\bbcnn_image_fit\b", text)) == 2   # the typedef and the parameter
    assert re.sub(r"\s", "", enums[0]) == "BCNN_IMAGE_FIT_STRETCH=0,BCNN_IMAGE_FIT_LETTERBOX=1"
    assert os.path.exists(capi.LIB_PATH), "run __graft_entry__.build() first"
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "bcnn_fill_tensor_with_images")
    assert (capi.IMAGE_FIT_STRETCH, capi.IMAGE_FIT_LETTERBOX) == (0, 1)
    assert callable(getattr(capi.Net, "fill_images"))


def test_cabi_entry_point_is_declared_once_and_defined_once():
    from bcnn_amd import _lib
    name = "bcnn_hip_fill_images"
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    sources = {os.path.basename(p): _no_comments(open(p).read())
               for p in glob.glob(os.path.join(ROOT, "bcnn_amd", "csrc", "*.hip"))}
    assert len(sources) > 20
    assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1
    defined = [fn for fn, text in sources.items()
               for _ in re.findall(r"^[A-Za-z_][\w \*]*\b%s\s*\([^;{]*\)\s*\{" % name, text, flags=re.M)]
    assert defined == ["image_fill.hip"], defined
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 16
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    for build_file in (os.path.join("bcnn_amd", "csrc", "Makefile"), "CMakeLists.txt"):
        text = open(os.path.join(ROOT, build_file)).read()
        assert "image_fill.hip" in text or "${CSRC}/*.hip" in text, build_file


def test_resize_sampling_rule_has_one_definition():
    """bip_min.c (the host resize) and image_fill.hip (the tap tables of the kernel) include the same header; no other
    file of the tree defines the rule"""
    host, csrc = os.path.join(ROOT, "bcnn_amd", "host"), os.path.join(ROOT, "bcnn_amd", "csrc")
    files = glob.glob(os.path.join(host, "*.[ch]")) + glob.glob(os.path.join(csrc, "*.hip")) + \
        glob.glob(os.path.join(csrc, "*.h"))
    defs = [os.path.basename(p) for p in files
            if re.search(r"\bvoid\s+\w*resize_tap\s*\([^;{]*\)\s*\{", _no_comments(open(p).read()))]
    assert defs == ["bip_resize_tap.h"], defs
    for user in (os.path.join(host, "bip_min.c"), os.path.join(csrc, "image_fill.hip")):
        assert re.search(r'#include\s+"[./a-z]*bip_resize_tap\.h"', open(user).read()), user
