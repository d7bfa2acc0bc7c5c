"""CPU checks of the batched-detection entry points: the two public functions are declared in include/bcnn/bcnn.h and
exported by the built libbcnn.so; the C-ABI entry points behind them are declared once in include/bcnn_hip.h, defined
once in bcnn_amd/csrc, and exported by libbcnn_hip.so."""
import ctypes
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ["bcnn_yolo_get_detections_batch", "bcnn_free_detections"]
CABI = ["bcnn_hip_yolo_nms_capacity", "bcnn_hip_yolo_detect_result_words", "bcnn_hip_yolo_detect_batch"]


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def test_public_functions_are_declared_and_exported():
    from bcnn_amd import capi
    text = _no_comments(open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read())
    for name in PUBLIC:
        assert len(re.findall(r"BCNN_API\s+[A-Za-z_ \*]+?\b%s\s*\(" % name, text)) == 1, name
    assert os.path.exists(capi.LIB_PATH), "run __graft_entry__.build() first"
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in PUBLIC:
        assert hasattr(raw, name), name
    assert hasattr(raw, "bcnn_yolo_detections_batch_worker")   # the same call with its capacities as arguments


def test_cabi_entry_points_are_declared_once_and_defined_once():
    from bcnn_amd import _lib
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    sources = {os.path.basename(p): _no_comments(open(p).read())
               for p in glob.glob(os.path.join(ROOT, "bcnn_amd", "csrc", "*.hip"))}
    assert len(sources) > 20
    for name in CABI:
        assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1, name
        defined = [fn for fn, text in sources.items() for _ in re.findall(r"^[A-Za-z_][\w \*]*\b%s\s*\([^;{]*\)\s*\{" % name,
                                                                          text, flags=re.M)]
        assert defined == ["detect.hip"], (name, defined)
        assert name in _lib.SIGNATURES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in CABI:
        assert hasattr(raw, name), name


def test_nms_capacity_is_a_power_of_two_of_a_few_thousand():
    from bcnn_amd import _lib
    cap = _lib.load().bcnn_hip_yolo_nms_capacity()
    assert cap >= 2048 and cap & (cap - 1) == 0
    assert _lib.load().bcnn_hip_yolo_detect_result_words(3, 5, 4) == 3 + 3 * 5 * (1 + 6 + 4)
