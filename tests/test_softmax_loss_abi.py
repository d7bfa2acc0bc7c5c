"""The entry points of the softmax-loss node. CPU: the public header declares the builder, the
two readers, the bcnn_loss_norm enum and the layer-type constant behind the enumerator list (BCNN_LAYER_POOL2D + 5);
libbcnn.so and libbcnn_hip.so export them; bcnn_amd._lib / ops / capi expose the names with the right signatures; the
refusals that need no net (the first-node position, from the builder and from both INI section names; a normalize value
that is none of the three names). gpu (a net is built, so tensors are allocated): every other refusal of the builder, with
nothing added and the label tensor untouched, and every INI key of both section names, read off the builder's log line."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"bcnn_hip_softmax_loss_forward": 8, "bcnn_hip_softmax_loss_backward": 9, "bcnn_hip_softmax_loss_confusion": 7,
           "bcnn_hip_softmax_loss_c_reg": 0}
INVALID = 1   # BCNN_INVALID_PARAMETER


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def _flat(text):
    return re.sub(r"\s+", " ", text).strip()


def test_header_declares_the_builder_the_readers_and_the_constants():
    public = _no_comments(open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read())
    decl = re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_add_softmax_loss_layer\s*\(([^;{]*)\)\s*;", public)
    assert len(decl) == 1
    assert _flat(decl[0]) == ("bcnn_net *net, int ignore_label, bcnn_loss_norm norm, float scale, const char *src_id, "
                              "const char *label_id, const char *dst_id")
    decl = re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_get_softmax_loss_stats\s*\(([^;{]*)\)\s*;", public)
    assert len(decl) == 1 and _flat(decl[0]) == "bcnn_net *net, int node, bcnn_softmax_loss_stats *out"
    decl = re.findall(r"BCNN_API\s+bcnn_status\s+bcnn_get_confusion_matrix\s*\(([^;{]*)\)\s*;", public)
    assert len(decl) == 1 and _flat(decl[0]) == "bcnn_net *net, int node, int64_t *counts"
    value = re.findall(r"#define\s+BCNN_LAYER_SOFTMAX_LOSS\s+(.*)", public)
    assert len(value) == 1 and re.sub(r"\s+", "", value[0]) == "((bcnn_layer_type)(BCNN_LAYER_POOL2D+5))"
    body = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*bcnn_layer_type\s*;", public).group(1)
    names = [t.strip() for t in body.split(",") if t.strip()]
    assert names[-1] == "BCNN_LAYER_POOL2D" and len(names) == 18   # the enumerator list is untouched
    norm = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*bcnn_loss_norm\s*;", public).group(1)
    assert [t.strip() for t in norm.split(",")] == ["BCNN_LOSS_NORM_NONE", "BCNN_LOSS_NORM_VALID",
                                                   "BCNN_LOSS_NORM_VALID_PER_IMAGE"]   # 0, 1, 2
    stats = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*bcnn_softmax_loss_stats\s*;", public).group(1)
    assert _flat(stats) == "float loss; int64_t valid, ignored, out_of_range, correct;"


def test_entry_points_are_declared_listed_and_exported():
    from bcnn_amd import _lib, capi
    header = _no_comments(open(os.path.join(ROOT, "include", "bcnn_hip.h")).read())
    hip = C.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        assert len(re.findall(r"\b%s\s*\([^;{]*\)\s*;" % name, header)) == 1, name
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols(), name
        assert hasattr(hip, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["bcnn_hip_softmax_loss_c_reg"][0] is C.c_int
    rec = re.search(r"typedef\s+struct\s+bcnn_hip_softmax_loss_record\s*\{([^}]*)\}", header).group(1)
    assert _flat(rec) == "float loss; float grad_factor; int valid, ignored, out_of_range, correct;"
    desc = re.search(r"typedef\s+struct\s+bcnn_hip_softmax_loss_desc\s*\{([^}]*)\}", header).group(1)
    assert _flat(desc) == "int ignore_label; int norm; float scale;"
    host = C.CDLL(capi.LIB_PATH)
    for name in ("bcnn_add_softmax_loss_layer", "bcnn_get_softmax_loss_stats", "bcnn_get_confusion_matrix"):
        assert hasattr(host, name), name


def test_python_names_and_structures():
    from bcnn_amd import capi, ops
    for name in ("softmax_loss_forward", "softmax_loss_backward", "softmax_loss_confusion", "softmax_loss_c_reg",
                 "softmax_loss_record", "softmax_loss_read_record"):
        assert callable(getattr(ops, name)), name
    for name in ("softmax_loss", "softmax_loss_stats", "confusion_matrix"):
        assert callable(getattr(capi.Net, name)), name
    assert capi.LAYER_SOFTMAX_LOSS == capi.LAYER_POOL2D + 5 == 22
    assert (capi.LOSS_NORM_NONE, capi.LOSS_NORM_VALID, capi.LOSS_NORM_VALID_PER_IMAGE) == (0, 1, 2)
    assert capi.LOSS_NORMS == ops.LOSS_NORMS == {"none": 0, "valid": 1, "valid_per_image": 2}
    assert C.sizeof(ops.SoftmaxLossRecord) == 24 and C.sizeof(ops.SoftmaxLossDesc) == 12
    assert C.sizeof(capi.SoftmaxLossStats) == 40 and capi.SoftmaxLossStats.valid.offset == 8
    assert ops.softmax_loss_c_reg() >= 21   # VOC's classes stay in registers (host code: no device needed)
    L = capi.lib()
    i, f, cp, vp = C.c_int, C.c_float, C.c_char_p, C.c_void_p
    assert L.bcnn_add_softmax_loss_layer.argtypes == [vp, i, i, f, cp, cp, cp]
    assert L.bcnn_get_softmax_loss_stats.argtypes == [vp, i, C.POINTER(capi.SoftmaxLossStats)]
    assert L.bcnn_get_confusion_matrix.argtypes == [vp, i, C.POINTER(C.c_int64)]


def _bare_net(w=8, h=6, c=3, n=2, level=None):
    from bcnn_amd import capi
    L = capi.lib()
    net = C.c_void_p()
    assert L.bcnn_init_net(C.byref(net), capi.MODE_TRAIN) == 0   # host allocations only
    # the net is not ended: bcnn_end_net synchronises the device, and the CPU tests run without one
    L.bcnn_set_log_context(net, None, capi.LOG_SILENT if level is None else level)
    L.bcnn_set_input_shape(net, w, h, c, n)
    return L, net


def test_builder_refuses_the_first_node_position_without_a_device(capfd):
    L, net = _bare_net(level=2)
    capfd.readouterr()
    for norm in (0, 1, 2):
        assert L.bcnn_add_softmax_loss_layer(net, 255, norm, 1.0, b"input", b"label", b"loss") == INVALID
    assert L.bcnn_get_num_nodes(net) == 0
    assert "Softmax-loss layer can't be the first layer of the network" in capfd.readouterr().err
    out = __import__("bcnn_amd").capi.SoftmaxLossStats(loss=3.0, valid=7)
    assert L.bcnn_get_softmax_loss_stats(net, 0, C.byref(out)) == INVALID and out.loss == 0.0 and out.valid == 0
    assert L.bcnn_get_confusion_matrix(net, 0, None) == INVALID


SECTION = """
[net]
input_width=8
input_height=6
input_channels=3
batch_size=2

%s
[%s]
%s
src=%s
dst=loss
"""
CONV = """[conv]
filters=4
size=1
stride=1
pad=0
activation=linear
src=input
dst=c1
"""


@pytest.mark.parametrize("name", ["softmax_loss", "softmaxwithloss"])
def test_config_sections_reach_the_builder_and_refuse_a_bad_normalize_without_a_device(tmp_path, capfd, name):
    """as the first section both names are refused: by the builder (the first-node position) when the keys parse, and by
    the loader before it (no silent fallback) when normalize= is none of the three names"""
    for keys, line in (("ignore_label=255\nnormalize=valid\nscale=0.5", "can't be the first layer of the network"),
                       ("normalize=batch", "Softmax-loss layer loss: normalize must be none, valid or valid_per_image"),
                       ("normalize=VALID", "normalize must be none, valid or valid_per_image")):
        L, net = _bare_net(level=2)
        cfg = tmp_path / "loss.cfg"
        cfg.write_text(SECTION % ("", name, keys, "input"))
        capfd.readouterr()
        assert L.bcnn_load_net(net, str(cfg).encode(), None) == INVALID
        assert L.bcnn_get_num_nodes(net) == 0
        assert line in capfd.readouterr().err


# ---- with a net (device allocations) ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_builder_refusals_leave_the_net_as_it_was(capfd):
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=8, h=6, c=3, n=2)
    net.conv(4, 1, 1, 0, src="input", dst="c1")
    L, h = net.L, net.net
    L.bcnn_set_log_context(h, None, 2)
    tensors = lambda: (L.bcnn_get_num_nodes(h), net.index("loss"), net.shape(1), bool(net.tensor(1).data))
    before = tensors()
    assert before == (1, -1, (0, 0, 0, 0), False)
    bad = [((255, 0, 1.0, b"nowhere"), "invalid input node name nowhere"),
           ((255, 3, 1.0, b"c1"), "unknown normaliser 3"), ((255, -1, 1.0, b"c1"), "unknown normaliser -1"),
           ((1 << 24, 2, 1.0, b"c1"), "is not below 2^24"), (((1 << 24) + 5, 0, 1.0, b"c1"), "is not below 2^24")]
    for (ignore, norm, scale, src), line in bad:
        capfd.readouterr()
        assert L.bcnn_add_softmax_loss_layer(h, ignore, norm, scale, src, b"label", b"loss") == INVALID, line
        assert line in capfd.readouterr().err
        assert tensors() == before
    # the largest ignore label a float holds as an index is accepted, and so is "nothing ignored"
    assert L.bcnn_add_softmax_loss_layer(h, (1 << 24) - 1, 2, 1.0, b"c1", b"label", b"loss") == 0
    assert L.bcnn_add_softmax_loss_layer(h, -7, 0, 2.0, b"c1", b"label", b"loss2") == 0   # the same label map: shared
    assert L.bcnn_get_num_nodes(h) == 3 and net.shape(1) == (2, 1, 6, 8) and net.shape(net.index("loss")) == (2, 4, 6, 8)
    assert net.node_type(1) == capi.LAYER_SOFTMAX_LOSS and net.node_src(1, 1) == 1
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("other", ["cost", "yolo"])
def test_builder_refuses_a_label_tensor_another_node_shaped(capfd, other):
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_TRAIN, w=8, h=6, c=3, n=2)
    if other == "cost":
        net.conv(4, 1, 1, 0, src="input", dst="c1")
        net.cost("c1", "label", "cost")                  # a dense [2][4][6][8] label
    else:
        assert net.set_detector_training(True) == 0
        net.conv(21, 1, 1, 0, src="input", dst="c1")    # 3 anchors x (2 classes + 4 + 1)
        net.yolo(3, 2, [0, 1, 2], [1.0] * 6, "c1", "det")
    shape = net.shape(1)
    assert shape != (2, 1, 6, 8) and net.tensor(1).data
    net.L.bcnn_set_log_context(net.net, None, 2)
    capfd.readouterr()
    assert net.L.bcnn_add_softmax_loss_layer(net.net, 255, 2, 1.0, b"c1", b"label", b"loss") == INVALID
    assert "the label tensor is already %d x %d x %d x %d" % shape in capfd.readouterr().err
    assert net.L.bcnn_get_num_nodes(net.net) == 2 and net.shape(1) == shape and net.index("loss") == -1
    net.close()


# section name, keys, what the builder's log line must say: ignore, norm, scale
KEYS = [("softmax_loss", "", (-1, "valid_per_image", "1")),
        ("softmaxwithloss", "", (-1, "valid_per_image", "1")),
        ("softmax_loss", "ignore_label=255", (255, "valid_per_image", "1")),
        ("softmaxwithloss", "ignore_label=7\nnormalize=none\nscale=0.25", (7, "none", "0.25")),
        ("softmax_loss", "normalize=valid\nscale=3", (-1, "valid", "3")),
        ("softmaxwithloss", "normalize=valid_per_image\nignore_label=-1\nscale=1.5", (-1, "valid_per_image", "1.5"))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,keys,want", KEYS)
def test_config_sections_hand_every_key_to_the_builder(tmp_path, capfd, name, keys, want):
    from bcnn_amd import capi
    L, net = _bare_net(level=0)   # BCNN_LOG_INFO: the builder's line goes to stderr
    cfg = tmp_path / "loss.cfg"
    cfg.write_text(SECTION % (CONV, name, keys, "c1"))
    capfd.readouterr()
    assert L.bcnn_load_net(net, str(cfg).encode(), None) == 0
    io = capfd.readouterr()
    assert "ignore %d norm %s scale %s\n" % want in io.err + io.out, io.err + io.out
    assert L.bcnn_get_num_nodes(net) == 2 and L.bcnn_get_node_type(net, 1) == capi.LAYER_SOFTMAX_LOSS
    t = L.bcnn_peek_tensor(net, 1).contents
    assert (t.n, t.c, t.h, t.w) == (2, 1, 6, 8)
    L.bcnn_end_net(C.byref(net))


@pytest.mark.gpu
def test_config_refuses_a_bad_normalize_behind_a_conv(tmp_path):
    L, net = _bare_net()
    cfg = tmp_path / "loss.cfg"
    cfg.write_text(SECTION % (CONV, "softmax_loss", "normalize=mean", "c1"))
    assert L.bcnn_load_net(net, str(cfg).encode(), None) == INVALID
    assert L.bcnn_get_num_nodes(net) == 1   # the convolution in front of it was built; the loss section added nothing
    L.bcnn_end_net(C.byref(net))
