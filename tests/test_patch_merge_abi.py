"""CPU checks of the patch-merging, residual and GELU entry points: exports, constants, the path rule."""
import ctypes as C

import pytest


def test_exports_and_constants():
    from bcnn_amd import _lib, capi, ops
    hip, host = C.CDLL(_lib.LIB_PATH), C.CDLL(capi.LIB_PATH)
    for name in ("bcnn_hip_patch_merge_forward", "bcnn_hip_patch_merge_backward", "bcnn_hip_patch_merge_path"):
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(hip, name), name
    assert hasattr(host, "bcnn_add_patch_merging_layer") and hasattr(host, "bcnn_add_residual_layer")
    assert callable(capi.Net.patch_merging) and callable(capi.Net.residual)
    assert capi.LAYER_PATCH_MERGING == capi.LAYER_POOL2D + 10 == 27 and capi.LAYER_RESIDUAL == capi.LAYER_POOL2D + 11 == 28
    assert capi.ACT_GELU == capi.ACT_MISH + 1 == ops.ACT_ALL["gelu"] == 15 and "gelu" not in ops.ACT
    assert ops.PATCH_MERGE_PATHS == ("column", "split", "stream")


@pytest.mark.parametrize("c,path", [(1, 0), (3, 0), (8, 0), (9, 1), (96, 1), (256, 1), (257, 2), (512, 2)])
def test_path_is_a_function_of_the_channel_count(c, path):
    """host code only: column to C = 8, split to 256, else stream; N, H and W enter through the refusals alone"""
    from bcnn_amd import ops
    for n, h, w in ((1, 2, 2), (32, 14, 14), (2, 56, 56)):
        assert ops.patch_merge_path(n, c, h, w) == path
    assert ops.patch_merge_path(1, c, 3, 2) == ops.patch_merge_path(1, c, 2, 3) == ops.patch_merge_path(0, c, 2, 2) == -1
    assert ops.patch_merge_limits() == (8, 256)
