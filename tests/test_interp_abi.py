"""CPU checks of the bilinear interpolation node's entry points: the public header declares the
builder and the layer-type constant behind the enumerator list (BCNN_LAYER_POOL2D + 4), libbcnn.so exports the builder,
libbcnn_hip.so the three C-ABI functions, bcnn_amd._lib / ops / capi expose the new names, the builder refuses every
malformed extent form before it adds anything, and the config loader refuses malformed sections and hands every key of
both section names to the builder (read off the builder's refusal line). The one test that builds the two sections from
a file is marked gpu: a builder that succeeds allocates its output tensor on the device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bcnn_hip_interp_forward", "bcnn_hip_interp_backward", "bcnn_hip_interp_axis_taps")


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def test_header_declares_the_builder_and_the_constant():
    public = _no_comments(open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read())
    decl = re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_add_interp_layer\s*\(([^;{]*)\)\s*;", public)
    assert len(decl) == 1
    assert re.sub(r"\s+", " ", decl[0]).strip() == (
        "bcnn_net *net, int out_w, int out_h, int scale, int zoom, int align_corners, const char *src_id, "
        "const char *dst_id")
    value = re.findall(r"#define\s+BCNN_LAYER_INTERP\s+(.*)", public)
    assert len(value) == 1
    assert re.sub(r"\s+", "", value[0]) == "((bcnn_layer_type)(BCNN_LAYER_POOL2D+4))"
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
    assert len(_lib.SIGNATURES["bcnn_hip_interp_forward"][1]) == 7
    assert len(_lib.SIGNATURES["bcnn_hip_interp_backward"][1]) == 8
    assert len(_lib.SIGNATURES["bcnn_hip_interp_axis_taps"][1]) == 6
    assert re.search(r"typedef\s+struct\s+bcnn_hip_interp_desc\s*\{\s*int\s+out_h\s*,\s*out_w\s*;\s*int\s+align_corners\s*;\s*\}",
                     header)
    assert hasattr(C.CDLL(capi.LIB_PATH), "bcnn_add_interp_layer")


def test_python_names():
    from bcnn_amd import capi, ops
    for name in ("interp_out_hw", "interp_forward", "interp_backward", "interp_axis_taps"):
        assert callable(getattr(ops, name)), name
    assert callable(capi.Net.interp)
    assert capi.LAYER_INTERP == capi.LAYER_POOL2D + 4 == 21
    assert ops.interp_out_hw(65, 65, zoom=8) == (513, 513)
    assert ops.interp_out_hw(33, 33, scale=4) == (132, 132)
    assert ops.interp_out_hw(9, 12, out_h=4, out_w=5) == (4, 5)
    assert ops.interp_out_hw(9, 12) == (0, 0) and ops.interp_out_hw(9, 12, scale=2, zoom=2) == (0, 0)


def _bare_net(w=8, h=6, c=3, n=2):
    from bcnn_amd import capi
    L = capi.lib()
    net = C.c_void_p()
    assert L.bcnn_init_net(C.byref(net), capi.MODE_TRAIN) == 0   # host allocations only
    # the net is not ended: bcnn_end_net synchronises the device, and these tests run without one
    L.bcnn_set_log_context(net, None, capi.LOG_SILENT)
    L.bcnn_set_input_shape(net, w, h, c, n)
    return L, net


def test_builder_refuses_malformed_forms_without_a_device():
    """the builder checks its parameters before it adds anything; the net's first node reads the input shape"""
    L, net = _bare_net()
    bad = [(0, 0, 0, 0, b"input"),      # no form (scale = 0 together with zoom = 0, no extents)
           (0, 0, 2, 2, b"input"),      # two forms
           (16, 12, 2, 0, b"input"), (16, 12, 0, 3, b"input"), (16, 12, 2, 3, b"input"),
           (0, 12, 0, 0, b"input"), (16, 0, 0, 0, b"input"),     # half a fixed form
           (-16, 12, 0, 0, b"input"), (16, -12, 0, 0, b"input"), (-1, -1, 0, 0, b"input"),   # non-positive extents
           (0, 0, -2, 0, b"input"), (0, 0, 0, -1, b"input"), (0, 0, -1, 2, b"input"),
           (0, 0, 2, 0, b"nowhere"), (16, 12, 0, 0, b"nowhere")]   # an unknown source name
    for out_w, out_h, scale, zoom, src in bad:
        for align_corners in (0, 1):
            st = L.bcnn_add_interp_layer(net, out_w, out_h, scale, zoom, align_corners, src, b"up")
            assert st == 1, (out_w, out_h, scale, zoom, src)   # BCNN_INVALID_PARAMETER
            assert L.bcnn_get_num_nodes(net) == 0


SECTION = """
[net]
input_width=8
input_height=6
input_channels=3
batch_size=2

[%s]
%s
src=input
dst=up
"""
# section name, keys, (out_h, out_w) of a 6 x 8 input
SECTIONS = [("interp", "scale=2", (12, 16)), ("bilinear", "stride=3", (18, 24)), ("interp", "zoom=4\nalign_corners=1", (21, 29)),
            ("bilinear", "out_w=5\nout_h=4", (4, 5)), ("interp", "scale=2\nalign_corners=0\nactivation=linear", (12, 16))]
REFUSED = [("interp", "scale=2\nactivation=relu"), ("bilinear", "zoom=2\nactivation=relu"), ("interp", "align_corners=1"),
           ("interp", "scale=2\nzoom=2"), ("bilinear", "out_w=5"), ("interp", "scale=2\nstride=2")]


@pytest.mark.gpu   # a builder that succeeds allocates the output tensor on the device; everything else here runs without one
@pytest.mark.parametrize("name,keys,want", SECTIONS)
def test_config_sections_build_the_node(tmp_path, name, keys, want):
    from bcnn_amd import capi
    cfg = tmp_path / "interp.cfg"
    cfg.write_text(SECTION % (name, keys))
    net = capi.Net.load_net(str(cfg), None, mode=capi.MODE_TRAIN)
    assert net.num_nodes == 1 and net.node_type(0) == capi.LAYER_INTERP
    assert net.shape(net.index("up")) == (2, 3) + want
    net.close()


# every key of a section, read back on the host: two forms at once are refused by the builder, whose log line names what
# it was handed. (section, keys, the values the line must carry: scale, zoom, out_w, out_h, align_corners)
PARSED = [("interp", "scale=2\nzoom=3\nout_w=5\nout_h=4\nalign_corners=1", (2, 3, 5, 4, 1)),
          ("bilinear", "stride=3\nzoom=2", (3, 2, 0, 0, 0)),
          ("bilinear", "zoom=7\nout_h=9\nout_w=11\nalign_corners=0", (0, 7, 11, 9, 0)),
          ("interp", "scale=4\nout_w=6\nout_h=8\nalign_corners=1\nactivation=linear", (4, 0, 6, 8, 1))]


@pytest.mark.parametrize("name,keys,want", PARSED)
def test_config_sections_hand_every_key_to_the_builder(tmp_path, capfd, name, keys, want):
    from bcnn_amd import capi
    L, net = _bare_net(1, 1, 1, 1)
    L.bcnn_set_log_context(net, None, 2)   # BCNN_LOG_ERROR: the refusal goes to stderr
    cfg = tmp_path / "interp.cfg"
    cfg.write_text(SECTION % (name, keys))
    capfd.readouterr()
    assert L.bcnn_load_net(net, str(cfg).encode(), None) == 1   # BCNN_INVALID_PARAMETER
    assert L.bcnn_get_num_nodes(net) == 0
    err = capfd.readouterr().err
    line = "Interp layer up: exactly one of scale (%d), zoom (%d) and out_w x out_h (%d x %d) must be given (align_corners %d)"
    assert line % want in err, err


@pytest.mark.parametrize("name,keys", REFUSED)
def test_config_sections_are_refused(tmp_path, name, keys):
    """refused before anything is added, so no device is touched"""
    L, net = _bare_net(1, 1, 1, 1)
    cfg = tmp_path / "interp.cfg"
    cfg.write_text(SECTION % (name, keys))
    assert L.bcnn_load_net(net, str(cfg).encode(), None) == 1   # BCNN_INVALID_PARAMETER
    assert L.bcnn_get_num_nodes(net) == 0
