"""CPU checks of the group-norm node's entry points: the public header declares the builder and the
layer-type constant behind the enumerator list (BCNN_LAYER_POOL2D + 2), libbcnn_hip.so exports the three C-ABI functions and
libbcnn.so the builder, bcnn_amd.ops / bcnn_amd.capi expose the new names, and the path rule is a function of the shape."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bcnn_hip_group_norm_forward", "bcnn_hip_group_norm_backward", "bcnn_hip_group_norm_path")


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def test_header_declares_the_builder_and_the_constant():
    public = _no_comments(open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read())
    decl = re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_add_groupnorm_layer\s*\(([^;{]*)\)\s*;", public)
    assert len(decl) == 1
    assert re.sub(r"\s+", " ", decl[0]).strip() == ("bcnn_net *net, int num_groups, float eps, const char *src_id, "
                                                    "const char *dst_id")
    value = re.findall(r"#define\s+BCNN_LAYER_GROUPNORM\s+(.*)", public)
    assert len(value) == 1
    assert re.sub(r"\s+", "", value[0]) == "((bcnn_layer_type)(BCNN_LAYER_POOL2D+2))"
    # the enumerator list is untouched: it still ends with BCNN_LAYER_POOL2D, at 17
    body = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*bcnn_layer_type\s*;", public).group(1)
    names = [t.strip() for t in body.split(",") if t.strip()]
    assert names[-1] == "BCNN_LAYER_POOL2D" and len(names) == 18


def test_entry_points_are_declared_listed_and_exported():
    from bcnn_amd import _lib, capi
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    hip = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1, name
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols(), name
        assert hasattr(hip, name), name
    assert len(_lib.SIGNATURES["bcnn_hip_group_norm_forward"][1]) == 11
    assert len(_lib.SIGNATURES["bcnn_hip_group_norm_backward"][1]) == 13
    assert hasattr(C.CDLL(capi.LIB_PATH), "bcnn_add_groupnorm_layer")


def test_python_names():
    from bcnn_amd import capi, ops
    assert callable(ops.group_norm_forward) and callable(ops.group_norm_backward) and callable(ops.group_norm_path)
    assert callable(capi.Net.groupnorm)
    assert capi.LAYER_GROUPNORM == capi.LAYER_POOL2D + 2 == 19
    assert ops.GROUP_NORM_PATHS == ("lanes", "resident", "split")


def test_path_is_a_function_of_the_row_length():
    """host code only: rows of up to 1024 floats go to lane groups, rows that fit the LDS stage (one for the forward, two
    for the backward) to a resident workgroup, the rest is split; the batch does not enter"""
    from bcnn_amd import ops
    for n in (1, 64):
        assert ops.group_norm_path(n, 72, 49, 72) == 0 and ops.group_norm_path(n, 72, 49, 72, True) == 0
        assert ops.group_norm_path(n, 1024, 1, 1) == 0 and ops.group_norm_path(n, 1025, 1, 1) == 1
        assert ops.group_norm_path(n, 512, 196, 32) == 1 and ops.group_norm_path(n, 512, 196, 32, True) == 1
        assert ops.group_norm_path(n, 16128, 1, 1) == 1 and ops.group_norm_path(n, 16129, 1, 1) == 2
        assert ops.group_norm_path(n, 8064, 1, 1, True) == 1 and ops.group_norm_path(n, 8065, 1, 1, True) == 2
        assert ops.group_norm_path(n, 256, 3136, 32) == 2 and ops.group_norm_path(n, 256, 3136, 1, True) == 2
    assert ops.group_norm_path(2, 6, 9, 4) == -1 and ops.group_norm_path(2, 6, 9, 0) == -1


def test_builder_refuses_invalid_groups_without_a_device():
    """the builder checks its parameters before it allocates anything; the net's first node reads the input shape"""
    from bcnn_amd import capi
    L = capi.lib()
    net = C.c_void_p()
    assert L.bcnn_init_net(C.byref(net), capi.MODE_TRAIN) == 0   # host allocations only
    # the net is not ended: bcnn_end_net synchronises the device, and this test runs without one
    L.bcnn_set_log_context(net, None, capi.LOG_SILENT)
    L.bcnn_set_input_shape(net, 8, 6, 6, 2)
    for groups in (0, -1, 4, 5, 7, 12):
        assert L.bcnn_add_groupnorm_layer(net, groups, 0.0, b"input", b"gn") == 1, groups   # BCNN_INVALID_PARAMETER
        assert L.bcnn_get_num_nodes(net) == 0
