"""The window-attention C ABI without a device: exports of both libraries, struct sizes, the node-type constant, and
ops.window_attention_check at each limit and one step past it."""
import ctypes as C

import pytest


def test_exports_struct_sizes_and_the_node_type():
    from bcnn_amd import _lib, capi
    hip, host = _lib.load(), capi.lib()
    for name in ("bcnn_hip_window_attention_forward", "bcnn_hip_window_attention_backward", "bcnn_hip_window_attention_check"):
        assert hasattr(hip, name), name
    assert hasattr(host, "bcnn_add_window_attention_layer")
    # 5 / 9 pointers, 8 ints, a float (and 3 ints): as the C compiler lays BcnnWindowAttnFwdArgs / BwdArgs out
    assert C.sizeof(_lib.WindowAttnFwdArgs) == 5 * 8 + 8 * 4 + 4 + 4 and C.sizeof(_lib.WindowAttnBwdArgs) == 9 * 8 + 8 * 4 + 4 + 3 * 4
    assert capi.LAYER_WINDOW_ATTENTION == capi.LAYER_POOL2D + 9 == 26


# (n, heads, d, c, h, w, window, shift) -> the refusal
@pytest.mark.parametrize("shape,want", [
    ((1, 1, 1, 1, 1, 1, 1, 0), "ok"), ((2, 3, 64, 64, 16, 8, 8, 7), "ok"), ((1, 1, 32, 32, 7, 7, 7, 6), "ok"),
    ((1, 65535, 1, 1, 1, 1, 1, 0), "ok"), ((1, 65536, 1, 1, 1, 1, 1, 0), "extent"),   # heads is a grid dimension
    ((0, 1, 1, 1, 1, 1, 1, 0), "extent"), ((1, 0, 1, 1, 1, 1, 1, 0), "extent"), ((1, 1, 1, 1, 0, 1, 1, 0), "extent"),
    ((1, 1, 1, 1, 1, 1, 0, 0), "window"), ((1, 1, 1, 1, 9, 9, 9, 0), "window"),
    ((1, 1, 1, 1, 9, 8, 8, 0), "ragged_map"), ((1, 1, 1, 1, 8, 9, 8, 0), "ragged_map"),
    ((1, 1, 1, 1, 8, 8, 8, 8), "shift"), ((1, 1, 1, 1, 8, 8, 8, -1), "shift"),
    ((1, 1, 65, 64, 8, 8, 8, 0), "head_dim"), ((1, 1, 64, 65, 8, 8, 8, 0), "head_dim"), ((1, 1, 0, 1, 8, 8, 8, 0), "head_dim"),
    ((1, 1, 64, 1, 4096, 8192, 8, 0), "too_large"), ((1, 1, 64, 1, 4096, 8184, 8, 0), "ok")], ids=str)
def test_check_at_each_limit(shape, want):
    from bcnn_amd import ops
    assert ops.WINDOW_ATTENTION_REFUSALS[ops.window_attention_check(*shape)] == want
