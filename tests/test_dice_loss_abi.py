"""The dice-loss node's interface without a device: exports, struct layouts, the layer type, the host-only path and
workspace functions with their refusals, and the config sections up to the builder's first check."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


def _fields(text, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}" % name, text).group(1), flags=re.S)
    return [w.strip(" *") for decl in body.split(";") for w in re.sub(r"^\s*(const\s+)?(float|int)\b", "", decl.strip()).split(",") if w.strip()]


def test_exports_struct_layouts_and_the_layer_type():
    from bcnn_amd import _lib, capi, ops
    header = open(os.path.join(ROOT, "include", "bcnn_hip.h")).read()
    public = open(os.path.join(ROOT, "include", "bcnn", "bcnn.h")).read()
    hip, host = C.CDLL(_lib.LIB_PATH), C.CDLL(capi.LIB_PATH)
    for name in ("forward", "backward", "workspace_size", "path"):
        assert hasattr(hip, "bcnn_hip_dice_loss_" + name) and "bcnn_hip_dice_loss_" + name in _lib.SIGNATURES
    for name in ("bcnn_add_dice_loss_layer", "bcnn_get_dice_loss_stats", "bcnn_get_dice_loss_sums"):
        assert hasattr(host, name) and len(re.findall(r"BCNN_API\s+bcnn_status\s+%s\s*\(" % name, public)) == 1
    for struct, cls, size in (("BcnnDiceLossFwdArgs", _lib.DiceLossFwdArgs, 72), ("BcnnDiceLossBwdArgs", _lib.DiceLossBwdArgs, 64),
                              ("bcnn_hip_dice_loss_record", ops.DiceLossRecord, 32)):
        assert _fields(header, struct) == [k for k, _ in cls._fields_] and C.sizeof(cls) == size, struct
    stats = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*bcnn_dice_loss_stats\s*;", public).group(1)
    assert re.findall(r"\b(loss|ce|dice|valid|ignored|out_of_range|correct)\b", stats) == [k for k, _ in capi.DiceLossStats._fields_]
    define = re.search(r"#define\s+BCNN_LAYER_DICE_LOSS\s+\(\(bcnn_layer_type\)\(BCNN_LAYER_POOL2D \+ (\d+)\)\)", public)
    assert capi.LAYER_DICE_LOSS == capi.LAYER_POOL2D + int(define.group(1)) == capi.LAYER_POOL2D + 13 == 30
    for name in ("dice_loss_forward", "dice_loss_backward", "dice_loss_path"):
        assert callable(getattr(ops, name))
    for name in ("dice_loss", "dice_loss_stats", "dice_loss_sums"):
        assert callable(getattr(capi.Net, name))


@pytest.mark.parametrize("aligned", [True, False])
def test_path_is_a_function_of_the_class_count_and_hw_alone(aligned):
    from bcnn_amd import ops
    assert ops.softmax_loss_c_reg() == 32
    assert [ops.dice_loss_path(2, c, 64, aligned) for c in (1, 32, 33)] == [0, 0, 1]
    assert [ops.dice_loss_path(2, c, 1, aligned) for c in (1, 33)] == [1, 1], "hw == 1: rows, then the sums from p"


def test_refusals_at_their_limits():
    from bcnn_amd import ops
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (-1, 3, 4)):
        assert ops.dice_loss_path(*shape) == -1 and ops.dice_loss_workspace_size(*shape) == 0, shape
    assert ops.dice_loss_path(1, 1, 2 ** 31 - 1) == 0 and ops.dice_loss_path(1, 2, 2 ** 30) == -1      # 2^31 - 1 | 2^31 elements
    assert ops.dice_loss_path(2 ** 15, 2 ** 4, 2 ** 12 - 1) == 0 and ops.dice_loss_path(2 ** 15, 2 ** 4, 2 ** 12) == -1
    assert ops.dice_loss_workspace_size(3, 5, 7, "batch") == 8 + 8 * 5 and ops.dice_loss_workspace_size(3, 5, 7, "image") == 8 + 8 * 15
    assert ops.dice_loss_workspace_size(3, 5, 7, 2) == 0 and ops.dice_loss_workspace_size(3, 5, 7, -1) == 0   # an unknown reduce


def _bare_net():
    """host allocations only. Not ended: bcnn_end_net synchronises the device, and these tests run without one"""
    from bcnn_amd import capi
    L, net = capi.lib(), C.c_void_p()
    assert L.bcnn_init_net(C.byref(net), capi.MODE_TRAIN) == 0
    L.bcnn_set_log_context(net, None, 2)
    L.bcnn_set_input_shape(net, 8, 6, 3, 2)
    return L, net


def test_builder_refusals_at_their_limits(capfd):
    """each refused argument at its limit and one step inside it; an accepted set reaches the first-node refusal"""
    L, net = _bare_net()
    add = lambda ignore, cw, dw, smooth, reduce: L.bcnn_add_dice_loss_layer(net, ignore, cw, dw, smooth, 1, reduce, b"input", b"label", b"x")
    nan, inf, fmax = float("nan"), float("inf"), 3.4028234663852886e38
    for args, line in (((1 << 24, 0.4, 0.6, 1e-5, 0), "is not below 2^24"), ((255, 0.4, 0.6, -1e-45, 0), "negative or not finite"),
                       ((255, 0.4, 0.6, inf, 0), "negative or not finite"), ((255, 0.4, 0.6, nan, 0), "negative or not finite"),
                       ((255, 0.4, 0.6, 1e-5, 2), "unknown reduce 2"), ((255, 0.4, 0.6, 1e-5, -1), "unknown reduce -1"),
                       ((255, nan, 0.6, 1e-5, 0), "a weight is not finite"), ((255, 0.4, inf, 1e-5, 0), "a weight is not finite"),
                       (((1 << 24) - 1, 0.4, 0.6, 0.0, 1), "can't be the first layer"), ((-1, -fmax, fmax, fmax, 0), "can't be the first layer")):
        capfd.readouterr()
        assert add(*args) == INVALID and L.bcnn_get_num_nodes(net) == 0
        assert line in capfd.readouterr().err, args
    assert L.bcnn_get_dice_loss_groups(net, 0) == -1


SECTION = "[net]\ninput_width=8\ninput_height=6\ninput_channels=3\nbatch_size=2\n\n[%s]\n%ssrc=input\ndst=loss\n"


@pytest.mark.parametrize("name", ["dice_loss", "softmax_dice_loss"])
def test_config_sections_reach_the_builder_and_refuse_a_bad_reduce(tmp_path, capfd, name):
    from bcnn_amd import capi
    """the builder checks its own arguments first and names them when it refuses the first-node position: the defaults and
    every key can be read without a device"""
    first = "Dice-loss layer (ignore %s) can't be the first layer of the network"
    for keys, line in (("", first % "-1 ce 0.4 dice 0.6 smooth 1e-05 squared reduce batch"),
                       ("ignore_label=7\nce_weight=0.5\ndice_weight=0.25\nsmooth=1\nsquared=0\nreduce=image\n",
                        first % "7 ce 0.5 dice 0.25 smooth 1 plain reduce image"),
                       ("reduce=mean\n", "Dice-loss layer loss: reduce must be batch or image")):
        L, net = _bare_net()
        cfg = tmp_path / "loss.cfg"
        cfg.write_text(SECTION % (name, keys))
        capfd.readouterr()
        assert L.bcnn_load_net(net, str(cfg).encode(), None) == INVALID and L.bcnn_get_num_nodes(net) == 0
        assert line in capfd.readouterr().err
        out = capi.DiceLossStats(loss=3.0, valid=7)
        assert L.bcnn_get_dice_loss_stats(net, 0, C.byref(out)) == INVALID and out.loss == 0.0 and out.valid == 0
        assert L.bcnn_get_dice_loss_sums(net, 0, None) == INVALID
