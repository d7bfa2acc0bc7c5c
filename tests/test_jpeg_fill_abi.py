"""CPU checks of the JPEG input path's entry points: bcnn_fill_tensor_with_jpegs is declared exactly once in
include/bcnn/bcnn.h and exported by libbcnn.so; the three C-ABI entry points behind it are declared once in
include/bcnn_hip.h, defined once in bcnn_amd/csrc/jpeg_pixels.hip, listed in _lib.SIGNATURES and exported by
libbcnn_hip.so, which still does not depend on libbip.so; the split decoder's entry points are declared once in
include/bip/bip.h and exported by libbip.so; the decoder's pixel arithmetic has one definition, which both users include."""
import ctypes
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CABI = {"bcnn_hip_jpeg_stage_begin": 9, "bcnn_hip_jpeg_stage_run": 6, "bcnn_hip_jpeg_stage_cancel": 0}
BIP = ("bip_jpeg_frame_info", "bip_jpeg_read_coefficients", "bip_jpeg_pixels_from_coefficients")
ARITHMETIC = ("bip_jpeg_idct8", "bip_jpeg_sar", "bip_jpeg_idct_column", "bip_jpeg_idct_row", "bip_jpeg_up_sample",
              "bip_jpeg_up_source_rows", "bip_jpeg_ycc_to_rgb", "bip_jpeg_clamp255")


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_public_function_is_declared_once_and_exported():
    from bcnn_amd import capi
    text = _no_comments(_read("include", "bcnn", "bcnn.h"))
    assert len(re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_fill_tensor_with_jpegs\s*\(", text)) == 1
    assert len(re.findall(r"\bbcnn_fill_tensor_with_jpegs\b", text)) == 1
    decl = re.search(r"bcnn_fill_tensor_with_jpegs\s*\(([^;]*)\)\s*;", text).group(1)
    params = [re.sub(r"\s+", " ", p).strip() for p in decl.split(",")]
    assert len(params) == 12 and params[3] == "const uint8_t *const *buffers" and params[4] == "const size_t *lengths"
    assert params[6:] == ["float norm_coeff", "int swap_to_bgr", "float mean_r", "float mean_g", "float mean_b",
                          "int *failed_image"]
    assert os.path.exists(capi.LIB_PATH), "run __graft_entry__.build() first"
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "bcnn_fill_tensor_with_jpegs")
    assert callable(getattr(capi.Net, "fill_jpegs"))


def test_cabi_entry_points_are_declared_once_and_defined_once():
    from bcnn_amd import _lib
    header = _no_comments(_read("include", "bcnn_hip.h"))
    sources = {os.path.basename(p): _no_comments(open(p).read())
               for p in glob.glob(os.path.join(ROOT, "bcnn_amd", "csrc", "*.hip"))}
    assert len(sources) > 20
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in CABI.items():
        assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1, name
        defined = [fn for fn, text in sources.items()
                   for _ in re.findall(r"^[A-Za-z_][\w \*]*\b%s\s*\([^;{]*\)\s*\{" % name, text, flags=re.M)]
        assert defined == ["jpeg_pixels.hip"], (name, defined)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), name
    for build_file in (os.path.join("bcnn_amd", "csrc", "Makefile"), "CMakeLists.txt"):
        text = _read(build_file)
        assert "jpeg_pixels.hip" in text or "${CSRC}/*.hip" in text, build_file
    for build_file in (os.path.join("bcnn_amd", "host", "Makefile"), "CMakeLists.txt"):
        assert "bcnn_input_jpeg.c" in _read(build_file), build_file
    # the kernels library does not link the image library: the coefficients come through the caller
    needed = subprocess.run(["readelf", "-d", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "libbip" not in needed


def test_split_decoder_is_declared_once_and_exported():
    from bcnn_amd import capi
    header = _no_comments(_read("include", "bip", "bip.h"))
    lib = ctypes.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libbip.so"))
    for name in BIP:
        assert len(re.findall(r"\bbip_status\s+%s\s*\([^;{]*\)\s*;" % name, header)) == 1, name
        assert hasattr(lib, name), name
    jpeg = _no_comments(_read("bcnn_amd", "host", "bip_jpeg.c"))
    # the one-call decoder is the two calls and the host pixel stage
    body = jpeg[jpeg.index("uint8_t *bip_decode_jpeg("):]
    for name in BIP:
        assert name + "(" in body, name


def test_pixel_arithmetic_has_one_definition_and_both_users_include_it():
    host, csrc = os.path.join(ROOT, "bcnn_amd", "host"), os.path.join(ROOT, "bcnn_amd", "csrc")
    files = glob.glob(os.path.join(host, "*.[ch]")) + glob.glob(os.path.join(csrc, "*.hip")) + \
        glob.glob(os.path.join(csrc, "*.h"))
    texts = {os.path.basename(p): _no_comments(open(p).read()) for p in files}
    for fn in ARITHMETIC:
        defs = [name for name, text in texts.items() if re.search(r"\b%s\s*\([^;{]*\)\s*\{" % fn, text)]
        assert defs == ["bip_jpeg_pixels.h"], (fn, defs)
    # the transform's and the colour conversion's constants appear nowhere else
    for constant in ("0.5411961", "1.847759065", "1.40200", "0.34414"):
        assert [name for name, text in texts.items() if constant in text] == ["bip_jpeg_pixels.h"], constant
    for user in (os.path.join(host, "bip_jpeg.c"), os.path.join(csrc, "jpeg_pixels.hip")):
        assert re.search(r'#include\s+"[./a-z]*bip_jpeg_pixels\.h"', open(user).read()), user
    header = texts["bip_jpeg_pixels.h"]
    assert "__host__ __device__" in header and "__HIPCC__" in header
