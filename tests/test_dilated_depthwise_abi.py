"""CPU checks of the dilated depthwise node's entry points: the public header declares the builder and
the layer-type constant behind the enumerator list (BCNN_LAYER_POOL2D + 6), libbcnn.so exports the builder, libbcnn_hip.so
the four C-ABI functions, bcnn_amd._lib / ops / capi expose the new names, the builder refuses bad parameters before it
touches a device, and the two shape queries are pure host functions."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"bcnn_hip_dilated_depthwise_workspace_size": 8, "bcnn_hip_dilated_depthwise_forward": 13,
           "bcnn_hip_dilated_depthwise_backward": 19, "bcnn_hip_dilated_depthwise_path": 9}
# the shapes of tests/test_dilated_depthwise.py: (n, c, h, w, k, s, p, d)
GPU_CASES = [
    (2, 3, 7, 9, 3, 1, 2, 2), (1, 4, 5, 5, 3, 1, 7, 7), (2, 5, 33, 33, 3, 1, 6, 6), (2, 3, 9, 9, 3, 1, 1, 3),
    (1, 2, 6, 6, 3, 1, 5, 2), (2, 6, 11, 10, 3, 2, 2, 2), (1, 3, 12, 13, 3, 2, 3, 3), (1, 2, 9, 9, 3, 3, 4, 4),
    (2, 4, 8, 8, 2, 1, 1, 2), (1, 3, 10, 10, 5, 1, 4, 2), (2, 17, 6, 6, 1, 1, 0, 3), (3, 70, 4, 4, 3, 1, 2, 2),
    (9, 3, 5, 5, 3, 1, 2, 2), (1, 2, 150, 260, 3, 1, 2, 2), (1, 1, 131, 257, 3, 1, 4, 4),
    (1, 1, 96, 128, 3, 1, 2, 2), (1, 1, 97, 128, 3, 1, 2, 2), (1, 1, 100, 120, 3, 1, 6, 2),
    (1, 1, 82, 151, 3, 1, 40, 40), (1, 1, 82, 152, 3, 1, 40, 40),
    (2, 5, 14, 14, 3, 1, 1, 1), (2, 3, 9, 11, 3, 2, 1, 1), (1, 70, 7, 7, 3, 1, 1, 1),
]


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def test_header_declares_the_builder_and_the_constant():
    public = _no_comments(open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read())
    decl = re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_add_dilated_depthwise_conv_layer\s*\(([^;{]*)\)\s*;", public)
    assert len(decl) == 1
    assert re.sub(r"\s+", " ", decl[0]).strip() == (
        "bcnn_net *net, int size, int stride, int pad, int dilation, bcnn_filler_type init, bcnn_activation activation, "
        "const char *src_id, const char *dst_id")
    value = re.findall(r"#define\s+BCNN_LAYER_DILATED_DEPTHWISE_CONV2D\s+(.*)", public)
    assert len(value) == 1
    assert re.sub(r"\s+", "", value[0]) == "((bcnn_layer_type)(BCNN_LAYER_POOL2D+6))"
    # the enumerator list is untouched: it still ends with BCNN_LAYER_POOL2D, at 17
    body = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*bcnn_layer_type\s*;", public).group(1)
    names = [t.strip() for t in body.split(",") if t.strip()]
    assert names[-1] == "BCNN_LAYER_POOL2D" and len(names) == 18


def test_entry_points_are_declared_listed_and_exported():
    from bcnn_amd import _lib, capi
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    hip = C.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1, name
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols(), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(hip, name), name
    assert hasattr(C.CDLL(capi.LIB_PATH), "bcnn_add_dilated_depthwise_conv_layer")


def test_python_names():
    from bcnn_amd import capi, ops
    for name in ("dilated_depthwise_workspace_size", "dilated_depthwise_forward", "dilated_depthwise_backward",
                 "dilated_depthwise_path", "dilated_conv_out_hw"):
        assert callable(getattr(ops, name)), name
    assert callable(capi.Net.dilated_depthwise)
    assert capi.LAYER_DILATED_DEPTHWISE_CONV2D == capi.LAYER_POOL2D + 6 == 23
    assert capi.lib().bcnn_add_dilated_depthwise_conv_layer.argtypes is not None   # the ctypes signature is set


def test_builder_refuses_invalid_parameters_without_a_device():
    """the builder checks its parameters before it allocates anything; the net's first node reads the input shape"""
    from bcnn_amd import capi
    L = capi.lib()
    net = C.c_void_p()
    assert L.bcnn_init_net(C.byref(net), capi.MODE_TRAIN) == 0   # host allocations only
    # the net is not ended: bcnn_end_net synchronises the device, and this test runs without one
    L.bcnn_set_log_context(net, None, capi.LOG_SILENT)
    L.bcnn_set_input_shape(net, 8, 6, 6, 2)
    bad = [(0, 1, 2, 2, capi.ACT_NONE), (-1, 1, 2, 2, capi.ACT_NONE), (3, 0, 2, 2, capi.ACT_NONE),
           (3, 1, -1, 2, capi.ACT_NONE), (3, 1, 2, 0, capi.ACT_NONE), (3, 1, 2, -3, capi.ACT_NONE),
           (3, 1, 0, 4, capi.ACT_NONE),      # 6 rows - 4 * 2 - 1 < 0
           (3, 1, 2, 2, capi.ACT_PRELU), (3, 1, 2, 2, capi.ACT_HARD_SWISH), (3, 1, 2, 2, capi.ACT_SWISH),
           (3, 1, 2, 2, capi.ACT_MISH)]
    for k, s, p, d, act in bad:
        st = L.bcnn_add_dilated_depthwise_conv_layer(net, k, s, p, d, capi.FILLER_XAVIER, act, b"input", b"dd")
        assert st == 1, (k, s, p, d, act)   # BCNN_INVALID_PARAMETER
        assert L.bcnn_get_num_nodes(net) == 0


def test_shape_queries_are_pure_and_need_no_device():
    from bcnn_amd import ops
    for case in GPU_CASES:
        n, c, h, w, k, s, p, d = case
        for backward in (False, True):
            path = ops.dilated_depthwise_path(*case, backward=backward)
            assert 0 <= path < len(ops.DILATED_DEPTHWISE_PATHS), (case, backward)
            assert path == ops.dilated_depthwise_path(*case, backward=backward)
            if k != 3 or s != 1:
                assert path == 0, case
        size = ops.dilated_depthwise_workspace_size(*case)
        assert size > 0 and size == ops.dilated_depthwise_workspace_size(*case)
        assert size % (n * c * (k * k + 1)) == 0, case   # k k tap sums and the bias sum per (plane, band)
        if ops.dilated_depthwise_path(*case, backward=True) != 2:
            assert size == n * c * (k * k + 1), case
    # a shape the workers refuse: the path query says so instead of ending the process
    assert ops.dilated_depthwise_path(1, 1, 4, 4, 3, 1, 0, 2) == -1      # 4 + 0 - 2 * 2 - 1 < 0
    assert ops.dilated_depthwise_path(0, 1, 4, 4, 3, 1, 2, 2) == -1
