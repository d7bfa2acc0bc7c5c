"""CPU checks of the channel-norm entry points: exports, struct sizes, the constant, the path rule."""
import ctypes as C

import pytest


def test_exports_struct_sizes_and_the_constant():
    from bcnn_amd import _lib, capi, ops
    hip = C.CDLL(_lib.LIB_PATH)
    for name in ("bcnn_hip_channel_norm_forward", "bcnn_hip_channel_norm_backward", "bcnn_hip_channel_norm_path"):
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(hip, name), name
    assert C.sizeof(_lib.ChannelNormFwdArgs) == 64 and C.sizeof(_lib.ChannelNormBwdArgs) == 80
    assert hasattr(C.CDLL(capi.LIB_PATH), "bcnn_add_channel_norm_layer") and callable(capi.Net.channelnorm)
    assert capi.LAYER_CHANNEL_NORM == capi.LAYER_POOL2D + 8 == 25
    assert ops.CHANNEL_NORM_PATHS == ("column", "resident", "stream")


@pytest.mark.parametrize("c,forward,backward", [(1, 0, 0), (8, 0, 0), (9, 0, 2), (16, 0, 2), (17, 1, 2), (238, 1, 2), (239, 2, 2),
                                                (768, 2, 2)])
def test_path_is_a_function_of_the_channel_count(c, forward, backward):
    """host code only: column to C = 16 forward / 8 backward, resident forward to 238, else stream; N and H*W do not enter"""
    from bcnn_amd import ops
    for n, hw in ((1, 1), (32, 49), (2, 3136)):
        assert ops.channel_norm_path(n, c, hw) == forward and ops.channel_norm_path(n, c, hw, True) == backward
    assert ops.channel_norm_path(1, 0, 4) == -1 and ops.channel_norm_path(1, 4, 0) == -1
