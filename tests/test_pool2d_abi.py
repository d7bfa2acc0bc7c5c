"""CPU checks of the pool2d node's entry points: libbcnn_hip.so exports the three C-ABI functions and
libbcnn.so the builder; the layer type is appended behind BCNN_LAYER_COST; bcnn_hip_pool2d_out_extent gives the shape
torch's CPU pooling returns; the builder refuses every invalid parameter set before it touches the device and leaves the
net as it was; the refused parameter sets have extent 0."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests._pool2d_cases import TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bcnn_hip_pool2d_out_extent", "bcnn_hip_pool2d_forward", "bcnn_hip_pool2d_backward")


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def test_entry_points_are_declared_listed_and_exported():
    from bcnn_amd import _lib, capi, ops
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    hip = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1, name
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols(), name
        assert hasattr(hip, name), name
    fields = re.search(r"typedef\s+struct\s+bcnn_hip_pool2d_desc\s*\{(.*?)\}\s*bcnn_hip_pool2d_desc\s*;", header, re.S)
    assert re.sub(r"\s+", " ", fields.group(1)).strip() == "int kind; int size, stride, pad; int ceil_mode; int count_include_pad;"
    assert C.sizeof(ops.Pool2dDesc) == 24                          # the six parameters
    public = _no_comments(open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read())
    assert len(re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_add_pool2d_layer\s*\(", public)) == 1
    assert hasattr(C.CDLL(capi.LIB_PATH), "bcnn_add_pool2d_layer")
    assert callable(capi.Net.pool2d) and callable(ops.pool2d_forward) and callable(ops.pool2d_backward)
    # no existing enumerator changed value: the new type is the last one, right behind BCNN_LAYER_COST
    body = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*bcnn_layer_type\s*;", public).group(1)
    names = [t.strip() for t in body.split(",") if t.strip()]
    assert names[-2:] == ["BCNN_LAYER_COST", "BCNN_LAYER_POOL2D"] and names.index("BCNN_LAYER_COST") == 16


@pytest.mark.parametrize("case", TABLE, ids=lambda c: "%s-%dx%d-k%ds%dp%d-%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "ceil" if c[6] else "floor"))
def test_out_extent_is_torchs(case):
    from bcnn_amd import ops
    kind, h, w, size, stride, pad, ceil, expected = case
    x = torch.zeros(1, 1, h, w)
    if kind == "max":
        ref = F.max_pool2d(x, size, stride, pad, ceil_mode=bool(ceil))
    else:
        ref = F.avg_pool2d(x, size, stride, pad, ceil_mode=bool(ceil))
    got = ops.pool2d_out_hw(kind, h, w, size, stride, pad, bool(ceil))
    assert got == tuple(ref.shape[2:])
    if expected is not None:
        assert got == expected


INVALID = [  # size, stride, pad on an 8 x 6 (w x h) input
    (0, 1, 0), (-1, 1, 0), (2, 0, 0), (2, -1, 0), (3, 1, -1), (3, 1, 2), (2, 2, 2), (4, 1, 3),
    (9, 1, 0),    # in + 2 pad < size on both axes
    (7, 1, 0),    # ... on the height only (6 < 7)
    (11, 1, 1),   # 8 + 2 < 11
]


def test_refused_parameter_sets_have_extent_zero():
    from bcnn_amd import ops
    for size, stride, pad in INVALID:
        oh, ow = ops.pool2d_out_hw("max", 6, 8, size, stride, pad)
        assert oh == 0 or ow == 0, (size, stride, pad)
    assert ops.pool2d_out_hw(7, 6, 8, 2, 2, 0) == (0, 0)           # unknown kind
    assert ops.pool2d_out_hw("avg", 0, 8, 2, 2, 0)[0] == 0          # empty input


def test_builder_refuses_invalid_parameters_without_a_device():
    """the builder checks its parameters before it allocates anything, so the refusals need no device; a net's first
    node reads the input shape bcnn_set_input_shape left"""
    from bcnn_amd import capi
    L = capi.lib()
    net = C.c_void_p()
    if L.bcnn_init_net(C.byref(net), capi.MODE_TRAIN) != 0:
        pytest.skip("no net can be built without a device")
    # the net is not ended: bcnn_end_net synchronises the device, and this test runs without one
    L.bcnn_set_log_context(net, None, capi.LOG_SILENT)
    L.bcnn_set_input_shape(net, 8, 6, 3, 2)
    assert L.bcnn_get_num_nodes(net) == 0
    for kind in (capi.POOL2D_MAX, capi.POOL2D_AVG):
        for size, stride, pad in INVALID:
            for ceil in (0, 1):
                st = L.bcnn_add_pool2d_layer(net, kind, size, stride, pad, ceil, 1, b"input", b"pool")
                assert st == 1, (kind, size, stride, pad, ceil)      # BCNN_INVALID_PARAMETER
                assert L.bcnn_get_num_nodes(net) == 0
    assert L.bcnn_add_pool2d_layer(net, 2, 2, 2, 0, 0, 1, b"input", b"pool") == 1   # unknown kind
    assert L.bcnn_get_num_nodes(net) == 0
