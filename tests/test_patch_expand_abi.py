"""CPU checks of the patch-expanding entry points: exports, signatures, constants, the path rule and
its refusals."""
import ctypes as C
import os
import re

import pytest


def test_exports_signatures_and_constants():
    from bcnn_amd import _lib, capi, ops
    hip, host = C.CDLL(_lib.LIB_PATH), C.CDLL(capi.LIB_PATH)
    for name in ("bcnn_hip_patch_expand_forward", "bcnn_hip_patch_expand_backward", "bcnn_hip_patch_expand_path"):
        assert name in _lib.SIGNATURES and name in _lib.declared_symbols() and hasattr(hip, name), name
    assert _lib.SIGNATURES["bcnn_hip_patch_expand_forward"] == _lib.SIGNATURES["bcnn_hip_patch_expand_backward"] == (None, [C.c_void_p])
    assert _lib.SIGNATURES["bcnn_hip_patch_expand_path"] == (C.c_int, [C.c_int] * 5)
    # the argument structs field for field, as the header declares them
    assert [k for k, _ in _lib.PatchExpandFwdArgs._fields_] == "x scales b y mean rstd n c_in h w block order eps".split()
    assert [k for k, _ in _lib.PatchExpandBwdArgs._fields_] == \
        "x scales mean rstd dy dx dscales db n c_in h w block order overwrite".split()
    assert C.sizeof(_lib.PatchExpandFwdArgs) == 6 * 8 + 7 * 4 + 4 and C.sizeof(_lib.PatchExpandBwdArgs) == 8 * 8 + 7 * 4 + 4
    assert hasattr(host, "bcnn_add_patch_expanding_layer") and callable(capi.Net.patch_expanding)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bcnn", "bcnn.h")).read()
    offset = int(re.search(r"#define BCNN_LAYER_PATCH_EXPANDING \(\(bcnn_layer_type\)\(BCNN_LAYER_POOL2D \+ (\d+)\)\)", header).group(1))
    assert capi.LAYER_PATCH_EXPANDING == capi.LAYER_POOL2D + offset == 29
    assert ops.PATCH_EXPAND_PATHS == ("column", "split", "stream") and ops.PATCH_EXPAND_ORDERS == dict(blocks=0, channels=1)
    assert (capi.PATCH_EXPAND_BLOCKS, capi.PATCH_EXPAND_CHANNELS) == (0, 1)


@pytest.mark.parametrize("block,limits", [(2, (8, 512)), (4, (8, 256))])
def test_path_is_a_function_of_channels_and_block(block, limits):
    """host code only: N, H and W enter through the refusals alone"""
    from bcnn_amd import ops
    assert ops.patch_expand_limits(block) == limits
    pp = block * block
    for c, path in ((1, 0), (limits[0], 0), (limits[0] + 1, 1), (96, 1), (limits[1], 1), (limits[1] + 1, 2), (2048, 2)):
        for n, h, w in ((1, 1, 1), (32, 28, 28), (2, 5, 13)):
            assert ops.patch_expand_path(n, c * pp, h, w, block) == path, (c, n, h, w)


@pytest.mark.parametrize("n,c_in,h,w,block", [
    (0, 16, 2, 2, 2), (1, 0, 2, 2, 2), (1, 16, 0, 2, 2), (1, 16, 2, 0, 4), (1, -16, 2, 2, 2),     # an extent below 1
    (1, 16, 2, 2, 1), (1, 9, 2, 2, 3), (1, 64, 2, 2, 8), (1, 16, 2, 2, 0),                        # a block other than 2 or 4
    (1, 6, 2, 2, 2), (1, 24, 2, 2, 4), (1, 3, 2, 2, 2),                                           # no multiple of block^2
    (1, 4, 1 << 15, 1 << 14, 2), (2, 16, 1 << 13, 1 << 13, 4), (1 << 16, 1 << 15, 1, 1, 2)])      # 2^31 elements or more
def test_path_refuses(n, c_in, h, w, block):
    from bcnn_amd import ops
    assert ops.patch_expand_path(n, c_in, h, w, block) == -1
