"""The forward and the data-gradient ladders kConvFwdFamilies / kConvDxFamilies (bcnn_amd/csrc/conv.hip), row by row and
host-chosen sub-branch by sub-branch: which family takes a layer (dispatch trace) and what it computes -- EXACTLY, on small
integers, as tests/test_conv_dw_ladder.py does for the weight gradient (same data, same float64 reference, same precondition:
the convolutions of the absolute values stay below 2^24, or 2^24 / 64 where an F(2x2,3x3) family can take the shape; asserted
on the reference alone, before the comparison).

What the cases are aimed at: the stride-parity classes of the two data-gradient GEMMs (classes that own no tap when the stride
is above the kernel size, classes of different sizes in one launch, where the largest needs a column tile more than the first,
input rows and columns behind the last window, and the 64 classes of a stride of 8), the chunks of the few-channel col2im data gradient, the three tiles of the register-staged kernel, the fused epilogue of every forward family
(bias indexed g * Mg + m, a bias of exactly 1.0f that is not added -- here always the last filter of every group, which lies in
the ragged last row block wherever there is one -- and the cheap activations), and the ragged edges of the window, stem and
direct kernels.

Activations in the fused forward epilogue: NONE, RELU, ABS, CLAMP and PRELU with dyadic slopes of both signs are exact; LRELU is
one fp32 product 0.1f * x, the correctly rounded float64 product; RAMP is x * (x > 0) + 0.1f * x, which the compiler may contract
into one fma: exactly the two float32 candidates (one rounding or two) are accepted. The backward side has NONE, RELU and PRELU
with positive dyadic slopes (the node takes act' from y, as the reference does: with a negative slope that is not the derivative
autograd computes); its y is the reference's, so that a data-gradient case does not depend on the forward kernels.

The expected names are written out per case; `_port_fwd` / `_port_dx` are a port of the shape rules at kCUs = 256 that the cases are
checked against without a GPU (test_the_cases_agree_with_the_port_of_the_shape_rules). The trace assertion is the check."""
import functools
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_conv_dispatch_table import DX_FAMILIES, FWD_FAMILIES
from tests.test_conv_dw_ladder import (LIMIT, NONE, PRELU, RELU, SENTINEL, _assert_exact, _float_case, _integers, _out_hw,
                                       _reference, _trace_start, _trace_stop, _workspace)

gpu = pytest.mark.gpu
DEV = "cuda:0"
RAMP, LRELU, ABS, CLAMP = 3, 5, 6, 7
A3 = (NONE, RELU, PRELU)
ALL = (NONE, RELU, PRELU, RAMP, LRELU, ABS, CLAMP)
GUARD = 4096
KCUS = 256
TILES = ["conv_igemm_tile:32x128", "conv_igemm_tile:64x128", "conv_igemm_tile:128x128"]
# every name a forward launcher writes (families and host-chosen sub-branches; pack:self is tests/test_conv_dispatch_table.py's)
FWD_NAMES = set(FWD_FAMILIES) | set(TILES) | {"conv_fwd_window_kernel:tm1", "conv_fwd_window_kernel:tm2",
                                              "conv_fwd_direct_kernel:tm1", "conv_fwd_direct_kernel:tm2",
                                              "wino_fused:halfblocks", "wino_tail_fixup"}
# ... and a data-gradient launcher: the unfused F(2x2,3x3) form runs its 16 GEMMs on the forward LDS-DMA kernel; the class
# loops add conv_dx_classes:<launches> (_pick)
DX_NAMES = set(DX_FAMILIES) | set(TILES) | {"conv_igemm_dma_kernel:fwd", "conv_igemm_dma_kernel:dx+bnsums",
                                            "wino_fused:halfblocks", "wino_tail_fixup"}
SUB_BRANCHES = set(TILES) | {"conv_fwd_window_kernel:tm1", "conv_fwd_window_kernel:tm2", "conv_fwd_direct_kernel:tm1",
                             "conv_fwd_direct_kernel:tm2", "wino_fused:halfblocks", "conv_dx_classes:1", "conv_dx_classes:3",
                             "conv_dx_classes:4"}


def _pick(trace, names):
    return {k for k in trace if k in names or k.startswith("conv_dx_classes:")}


# ---- the expected names, by family ----------------------------------------------------------------------------------------
def WINDOW(tm):
    return {"conv_fwd_window_kernel", "conv_fwd_window_kernel:tm%d" % tm}


def DIRECT(tm):
    return {"conv_fwd_direct_kernel", "conv_fwd_direct_kernel:tm%d" % tm}


def FUSED_F(*more):
    return {"wino_fused_kernel:fwd"} | set(more)


def IGEMM_F(tile):
    return {"conv_igemm_kernel:fwd", "conv_igemm_tile:" + tile}


STEM = {"conv_fwd_stem_kernel"}
W43_F, W43_D = {"wino43b_kernel:fwd"}, {"wino43b_kernel:dx"}
UNFUSED_F = {"wino_unfused:fwd", "conv_igemm_dma_kernel:fwd"}
LARGE_F, LARGE_D = {"conv_large_gemm_kernel:fwd"}, {"conv_large_gemm_kernel:dx"}
DMA_F = {"conv_igemm_dma_kernel:fwd"}
SMALLC_F = {"conv_small_c:fwd", "conv_igemm_dma_kernel:fwd"}   # ends in the LDS-DMA launcher
FUSED_D = {"wino_fused_kernel:dx"}
UNFUSED_D = {"wino_unfused:dx", "conv_igemm_dma_kernel:fwd"}
SMALLC_D = {"conv_small_c:dx", "conv_igemm_tile:32x128"}       # col = W^T dy has K <= 32 rows


def _classes(launches):
    return set() if launches is None else {"conv_dx_classes:%d" % launches}


def DMA_D(launches):  # None: pointwise, no classes
    return {"conv_igemm_dma_kernel:dx"} | _classes(launches)


def IGEMM_D(tile, launches):
    return {"conv_igemm_kernel:dx", "conv_igemm_tile:" + tile} | _classes(launches)


# (n, c, h, w, f, k, stride, pad, groups), the activations of the forward runs, the forward names, the data-gradient names
# (None: that direction is not run). The shapes of a 3x3 / s1 / p1 layer's F(2x2,3x3) rows are tests/test_conv_dw_ladder.py's.
CASES = [
    # window row: 3x3 / s1, Cg <= 3, Mg <= 64, W % 4 == 0; strips of four output rows
    ((2, 3, 10, 16, 32, 3, 1, 1, 1), ALL, WINDOW(1), SMALLC_D),                 # OH = 10: a strip of 2
    ((1, 2, 7, 12, 40, 3, 1, 0, 1), A3, WINDOW(2), SMALLC_D),                   # ragged Mg, pad 0, a strip of 1
    ((2, 6, 9, 20, 64, 3, 1, 4, 2), A3, WINDOW(1), IGEMM_D("32x128", 1)),       # two groups, pad 4, Cg = 3
    ((1, 1, 5, 8, 8, 3, 1, 2, 1), A3, WINDOW(1), IGEMM_D("32x128", 1)),         # Cg = 1
    # stem row: 7x7 / s2; strips of eight output rows
    ((2, 3, 30, 32, 64, 7, 2, 3, 1), ALL, STEM, IGEMM_D("32x128", 1)),          # OH = 15: a strip of 7
    ((1, 2, 19, 20, 24, 7, 2, 0, 1), A3, STEM, IGEMM_D("32x128", 1)),
    ((2, 6, 21, 24, 64, 7, 2, 2, 2), A3, STEM, IGEMM_D("32x128", 1)),
    # direct row: K = 9, 18, 27 and 25 at both tm; tiles of 32 pixels, at least four per workgroup
    ((2, 1, 9, 11, 8, 3, 2, 1, 1), ALL, DIRECT(1), IGEMM_D("32x128", 1)),
    ((1, 2, 13, 13, 40, 3, 3, 3, 1), A3, DIRECT(2), SMALLC_D),                  # stride 3, pad 3 > k / 2
    ((2, 3, 17, 18, 33, 3, 1, 0, 1), A3, DIRECT(2), SMALLC_D),                  # W % 4 != 0
    ((1, 1, 21, 20, 8, 5, 1, 0, 1), A3, DIRECT(1), IGEMM_D("32x128", 1)),
    ((3, 2, 11, 11, 64, 5, 2, 2, 2), A3, DIRECT(1), IGEMM_D("32x128", 1)),      # 5x5 on one channel per group
    ((1, 3, 6, 7, 16, 3, 1, 0, 1), A3, DIRECT(1), IGEMM_D("32x128", 1)),        # total_q = 20 < 32
    ((1, 2, 13, 5, 48, 3, 1, 0, 1), A3, DIRECT(2), SMALLC_D),                   # total_q = 33
    ((1, 3, 8, 8, 16, 3, 4, 0, 1), A3, DIRECT(1), IGEMM_D("32x128", 4)),        # stride above the kernel size
    # fused F(2x2,3x3): T * ceil(M / 64) >= 8192
    ((32, 64, 32, 32, 64, 3, 1, 1, 1), ALL, FUSED_F(), FUSED_D),                # the smallest whole-units shape
    ((57, 72, 15, 17, 96, 3, 1, 1, 1), (NONE, PRELU), FUSED_F(), FUSED_D),      # odd plane, ragged M: the tiles hang over
    ((36, 64, 32, 32, 128, 3, 1, 1, 1), (RELU,), FUSED_F("wino_fused:halfblocks"), FUSED_D),  # 288 blocks: rem = 32
    # unfused F(2x2,3x3)
    ((2, 128, 14, 14, 128, 3, 1, 1, 1), ALL, UNFUSED_F, UNFUSED_D),
    ((3, 130, 13, 15, 128, 3, 1, 1, 1), A3, UNFUSED_F, UNFUSED_D),
    ((3, 128, 13, 15, 130, 3, 1, 1, 1), A3, UNFUSED_F, UNFUSED_D),
    # large row (tests/test_conv_large_kernel.py owns it)
    ((2, 3, 23, 23, 16, 11, 4, 0, 1), A3, LARGE_F, LARGE_D),
    # LDS-DMA row: Mg > 32, Cg >= 8
    ((4, 64, 14, 14, 128, 1, 1, 0, 1), A3, DMA_F, DMA_D(None)),
    ((4, 34, 14, 14, 130, 1, 1, 0, 1), ALL, DMA_F, DMA_D(None)),                # ragged rows and reduction
    ((4, 32, 12, 12, 72, 3, 2, 1, 2), A3, DMA_F, IGEMM_D("32x128", 1)),         # two groups, stride 2
    ((5, 16, 8, 8, 33, 5, 1, 2, 1), A3, DMA_F, IGEMM_D("32x128", 1)),           # Mg = 33: the lower edge
    ((2, 8, 9, 7, 66, 3, 1, 0, 1), A3, DMA_F, IGEMM_D("32x128", 1)),            # J = 8: the lower edge
    ((3, 24, 10, 10, 40, 7, 3, 3, 1), A3, DMA_F, IGEMM_D("32x128", 3)),         # 49 taps, stride 3
    # few-channel row: Cg < 8, Mg > 32, K >= 64
    ((2, 3, 16, 16, 64, 5, 1, 2, 1), ALL, SMALLC_F, IGEMM_D("32x128", 1)),
    ((2, 3, 30, 30, 40, 7, 2, 3, 1), A3, SMALLC_F, IGEMM_D("32x128", 1)),       # W % 4 != 0 keeps it off the stem row
    ((1, 7, 12, 12, 34, 5, 1, 2, 1), A3, SMALLC_F, IGEMM_D("32x128", 1)),
    ((2, 4, 9, 9, 33, 4, 1, 0, 1), A3, SMALLC_F, IGEMM_D("32x128", 1)),         # K = 64: the lower edge
    # register-staged row and its three tiles
    ((2, 16, 8, 8, 16, 1, 1, 0, 1), ALL, IGEMM_F("32x128"), IGEMM_D("32x128", None)),
    ((2, 4, 9, 9, 40, 1, 1, 0, 1), A3, IGEMM_F("64x128"), IGEMM_D("32x128", None)),
    ((2, 4, 9, 9, 130, 1, 1, 0, 1), ALL, IGEMM_F("64x128"), IGEMM_D("32x128", None)),   # M > 64, four big tiles: three row tiles
    ((2, 4, 128, 128, 130, 1, 1, 0, 1), A3, IGEMM_F("128x128"), IGEMM_D("32x128", None)),  # 2 * 256 big tiles
    ((2, 12, 11, 11, 20, 3, 2, 0, 2), A3, IGEMM_F("32x128"), IGEMM_D("32x128", 1)),     # two groups
    ((1, 4, 5, 5, 6, 3, 1, 1, 1), A3, IGEMM_F("32x128"), IGEMM_D("32x128", 1)),
    # D1: the stride-parity classes of the LDS-DMA data gradient (Cg > 32, Mg >= 8), four per launch
    ((2, 34, 9, 11, 16, 3, 2, 1, 1), A3, IGEMM_F("32x128"), DMA_D(1)),          # odd planes: classes of 5x6, 5x5, 4x6, 4x5
    ((2, 34, 11, 11, 16, 3, 2, 1, 1), None, None, DMA_D(1)),                    # 50, 60, 60 and 72 columns: one and two 64-column tiles
    ((2, 40, 10, 7, 8, 3, 2, 0, 1), A3, IGEMM_F("32x128"), DMA_D(1)),           # the last input row is behind the last window
    ((2, 40, 10, 8, 8, 3, 2, 0, 1), None, None, DMA_D(1)),                      # ... and the last column too
    ((2, 36, 13, 11, 16, 5, 3, 2, 1), A3, IGEMM_F("32x128"), DMA_D(3)),         # nine classes
    ((2, 36, 11, 10, 16, 2, 3, 0, 1), A3, IGEMM_F("32x128"), DMA_D(3)),         # stride 3, k = 2: five classes own no tap
    ((2, 36, 12, 10, 16, 2, 3, 0, 1), None, None, DMA_D(3)),                    # ... a row and two columns behind the last window
    ((1, 40, 13, 14, 8, 3, 4, 1, 1), A3, IGEMM_F("32x128"), DMA_D(4)),          # 16 classes, 7 of them own no tap
    ((1, 40, 14, 14, 8, 3, 4, 1, 1), None, None, DMA_D(4)),                     # ... a remainder in both directions
    ((1, 40, 17, 18, 8, 3, 8, 1, 1), A3, IGEMM_F("32x128"), DMA_D(16)),         # stride 8: 64 classes, 55 of them own no tap
    ((4, 72, 12, 12, 32, 3, 2, 1, 2), A3, IGEMM_F("32x128"), DMA_D(1)),         # two groups
    ((4, 130, 14, 14, 34, 1, 1, 0, 1), A3, DMA_F, DMA_D(None)),                 # pointwise
    # D2: the same class edges on the register-staged data gradient (Cg <= 32), and its tiles
    ((2, 16, 11, 10, 8, 2, 3, 0, 1), A3, IGEMM_F("32x128"), IGEMM_D("32x128", 3)),
    ((1, 8, 13, 14, 8, 3, 4, 1, 1), A3, IGEMM_F("32x128"), IGEMM_D("32x128", 4)),
    ((1, 8, 17, 18, 8, 3, 8, 1, 1), None, None, IGEMM_D("32x128", 16)),         # stride 8: 64 classes in 16 launches
    ((2, 16, 9, 11, 16, 3, 2, 1, 2), A3, IGEMM_F("32x128"), IGEMM_D("32x128", 1)),
    ((4, 16, 11, 11, 8, 3, 2, 1, 1), None, None, IGEMM_D("32x128", 1)),         # 100 to 144 columns: one and two 128-column tiles
    ((2, 130, 128, 128, 4, 1, 1, 0, 1), (NONE,), IGEMM_F("32x128"), IGEMM_D("128x128", None)),
    ((2, 40, 9, 9, 4, 1, 1, 0, 1), A3, IGEMM_F("32x128"), IGEMM_D("64x128", None)),
    ((2, 40, 9, 9, 4, 3, 2, 1, 1), A3, IGEMM_F("32x128"), IGEMM_D("64x128", 1)),  # Mg < 8 keeps it off the LDS-DMA row
    # D3: the few-channel col2im data gradient (K <= 32, Mg >= 32, one group)
    ((2, 3, 16, 16, 32, 3, 1, 1, 1), A3, WINDOW(1), SMALLC_D),
    ((2, 2, 11, 13, 33, 4, 3, 1, 1), A3, IGEMM_F("64x128"), SMALLC_D),          # K = 32, stride 3, a remainder
    ((1, 1, 10, 9, 40, 2, 3, 0, 1), A3, IGEMM_F("64x128"), SMALLC_D),           # stride above the kernel size
    ((2, 3, 15, 15, 32, 3, 2, 0, 1), A3, DIRECT(1), SMALLC_D),
]
IDS = ["x".join(map(str, c[0])) for c in CASES]
# the raw forward with batch-norm statistics (TRAIN), for the rows whose epilogue emits them
RAW = [((2, 3, 30, 32, 64, 7, 2, 3, 1), STEM), ((32, 64, 32, 32, 64, 3, 1, 1, 1), FUSED_F()),
       ((57, 72, 15, 17, 96, 3, 1, 1, 1), FUSED_F()), ((2, 128, 14, 14, 128, 3, 1, 1, 1), UNFUSED_F),
       ((4, 34, 14, 14, 130, 1, 1, 0, 1), DMA_F), ((4, 32, 12, 12, 72, 3, 2, 1, 2), DMA_F),
       ((2, 3, 30, 30, 40, 7, 2, 3, 1), SMALLC_F)]
RAW_IDS = ["x".join(map(str, c[0])) for c in RAW]
W43_LAYER = (16, 64, 64, 64, 64, 3, 1, 1, 1)       # F(4x4,3x3): raw forward and data gradient, float data
CHUNK_LAYER = (19, 3, 224, 224, 32, 3, 1, 1, 1)    # D5: 18 images of col fit in 96 MiB, the 19th is a chunk of its own


# ---- a port of the shape rules (conv_window.hip, conv_direct.hip, conv_winograd*.hip, conv_large.hip, conv_igemm_dma.hip,
# conv_igemm.hip) at kCUs = 256 ---------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


class _Shape:
    def __init__(self, layer):
        self.N, self.C, self.H, self.W, self.F, self.k, self.st, self.pad, self.g = layer
        self.OH, self.OW = _out_hw(layer)
        self.Cg, self.Mg = self.C // self.g, self.F // self.g
        self.K = self.Cg * self.k * self.k
        self.HW, self.OHOW = self.H * self.W, self.OH * self.OW
        self.total_q, self.total_p = self.N * self.OHOW, self.N * self.HW
        self.pw = self.k == 1


def _window_ok(s):
    need = ((s.OW + 31) & ~31) + 6
    pitch = 232 if need <= 232 else 264 if need <= 264 else 0
    return (not s.pw and s.k == 3 and s.st == 1 and 1 <= s.Cg <= 3 and s.Mg <= 64 and s.pad <= 4 and s.W % 4 == 0 and
            s.total_q > 0 and pitch != 0 and s.W + 4 <= pitch and s.N * s.F * s.OHOW < 1 << 29 and s.N * s.C * s.HW < 1 << 29)


def _stem_ok(s):
    return (not s.pw and s.k == 7 and s.st == 2 and s.pad <= 4 and 1 <= s.Cg <= 3 and s.Mg <= 64 and s.W % 4 == 0 and
            s.W + 4 <= 232 and 2 * (s.OW - 1) + 7 + (4 - s.pad) <= 232 and s.total_q > 0)


def _direct_ok(s):
    return ((s.k == 3 and 1 <= s.Cg <= 3) or (s.k == 5 and s.Cg == 1)) and s.Mg <= 64


def _wino_base(s):
    return s.k == 3 and s.st == 1 and s.pad == 1 and s.g == 1


def _wino43_wanted(s, J, M):
    if not _wino_base(s) or s.H % 4 or s.W % 4 or s.H < 3 or s.W < 3 or J < 16 or J % 8 or M < 16:
        return False
    T = s.N * (s.H // 4) * (s.W // 4)
    return J >= 64 and M >= 64 and _cdiv(T, 32) * _cdiv(M, 32) >= KCUS


def _tiles2(s):
    return s.N * _cdiv(s.H, 2) * _cdiv(s.W, 2)


def _fused_wanted(s, J, M):
    if not _wino_base(s) or J < 16 or J % 8 or M < 32:
        return False
    return J >= 64 and M >= 64 and _tiles2(s) * _cdiv(M, 64) >= 64 * KCUS // 2


def _fused_names(s, J, M, plain):
    """wino_fused_run: the last round as half blocks, or (plain output only) cut along the channels with a fix-up pass"""
    nblocks = _cdiv(_tiles2(s), 64) * _cdiv(M, 64)
    grid = min(nblocks, KCUS)
    rem = nblocks % grid
    half = rem > 0 and 2 * rem <= grid and nblocks > grid
    tail = False
    if plain and rem > 0 and nblocks > grid:
        nc = _cdiv(J, 8)
        q = _cdiv(rem * nc, grid)
        tail = 1 <= q <= nc and q + 2 * 1.5 + 2.0 < (0.5 * nc if half else nc) + 1.5
    return {"wino_tail_fixup"} if tail else {"wino_fused:halfblocks"} if half else set()


def _unfused_wanted(s):
    T = _tiles2(s)
    return (_wino_base(s) and s.C >= 16 and s.F >= 64 and T > 0 and max(s.C, s.F) * 16 * T * 4 < 0x7ffffff0 and
            s.C >= 128 and s.F >= 128 and 16.0 * T * (s.C + s.F) * 4.0 <= 230e6)


def _dma_supported(s, M, J):
    return not (s.k > 7 and not s.pw) and M > 32 and J >= 8


def _tile(M, cols, groups, nclass):
    big = _cdiv(M, 128) * _cdiv(cols, 128) * groups * nclass
    return "conv_igemm_tile:" + ("32x128" if M <= 32 else "64x128" if M <= 64 or big < 2 * KCUS else "128x128")


def _port_fwd(layer, raw):
    s = _Shape(layer)
    if _window_ok(s):
        return WINDOW(1 if s.Mg <= 32 else 2)
    if _stem_ok(s):
        return set(STEM)
    if _direct_ok(s):
        return DIRECT(1 if s.Mg <= 32 else 2)
    if raw and _wino43_wanted(s, s.C, s.F):
        return set(W43_F)
    if _fused_wanted(s, s.C, s.F):
        return FUSED_F() | _fused_names(s, s.C, s.F, raw)
    if _unfused_wanted(s):
        return set(UNFUSED_F)
    if s.k > 7 and not s.pw:
        return set(LARGE_F)
    if _dma_supported(s, s.Mg, s.Cg):
        return set(DMA_F)
    if s.g == 1 and not s.pw and s.k <= 7 and s.Cg < 8 and s.Mg > 32 and s.K >= 64:
        return set(SMALLC_F)
    return {"conv_igemm_kernel:fwd", _tile(s.Mg, s.total_q, s.g, 1)}


def _class_launches(s):
    """[(classes, columns of the largest)] per launch of up to four stride-parity classes; launches without columns are skipped"""
    cols = []
    for ra in range(s.st):
        for rb in range(s.st):
            ih0, iw0 = (ra - s.pad) % s.st, (rb - s.pad) % s.st
            hc = _cdiv(s.H - ih0, s.st) if ih0 < s.H else 0
            wc = _cdiv(s.W - iw0, s.st) if iw0 < s.W else 0
            cols.append(s.N * hc * wc)
    out = [(len(cols[i:i + 4]), max(cols[i:i + 4])) for i in range(0, len(cols), 4)]
    return [v for v in out if v[1] > 0]


def _port_dx(layer):
    s = _Shape(layer)
    if _wino43_wanted(s, s.F, s.C):
        return set(W43_D)
    if _fused_wanted(s, s.F, s.C):
        return FUSED_D | _fused_names(s, s.F, s.C, True)
    if _unfused_wanted(s) and s.F >= 16 and s.C >= 64:
        return set(UNFUSED_D)
    if s.k > 7 and not s.pw:
        return set(LARGE_D)
    if not s.pw and s.g == 1 and s.K <= 32 and s.Mg >= 32:
        return set(SMALLC_D)
    if _dma_supported(s, s.Cg, s.Mg):
        return DMA_D(None if s.pw else len(_class_launches(s)))
    if s.pw:
        return {"conv_igemm_kernel:dx", _tile(s.Cg, s.total_q, s.g, 1)}
    launches = _class_launches(s)
    return {"conv_igemm_kernel:dx"} | {_tile(s.Cg, cols, s.g, nc) for nc, cols in launches} | _classes(len(launches))


def test_the_cases_agree_with_the_port_of_the_shape_rules():
    """no GPU: the names written out in CASES / RAW against the port, and every row and sub-branch has a case"""
    fwd, dx = set(), set()
    for layer, acts, want_fwd, want_dx in CASES:
        if want_fwd is not None:
            assert _port_fwd(layer, False) == want_fwd, (layer, sorted(_port_fwd(layer, False)))
            fwd |= want_fwd
        assert _port_dx(layer) == want_dx, (layer, sorted(_port_dx(layer)))
        dx |= want_dx
    for layer, want in RAW:
        assert _port_fwd(layer, True) == want, (layer, sorted(_port_fwd(layer, True)))
    for layer in [c[0] for c in CASES] + [c[0] for c in RAW]:
        f, g = layer[4], layer[8]
        t = _data(layer)
        for v in (t["slopes"], t["slopes"].abs(), t["b"]):       # a dropped g * Mg offset must change what is read
            rows = v.view(g, f // g)
            assert all(int((rows[0] != rows[gi]).sum()) >= max(2, f // g // 4) for gi in range(1, g)), (layer, v)
        assert float(t["slopes"].min()) < 0 < float(t["slopes"].max()) and float(t["slopes"].abs().min()) >= 0.125
    assert _port_fwd(W43_LAYER, True) == W43_F and _port_dx(W43_LAYER) == W43_D
    assert _port_dx(CHUNK_LAYER) == SMALLC_D
    fwd |= W43_F
    dx |= W43_D
    assert [k for k in FWD_FAMILIES if k not in fwd] == [] and [k for k in DX_FAMILIES if k not in dx] == []
    assert sorted(SUB_BRANCHES - fwd - dx) == []
    assert len(FWD_FAMILIES) == 10 and len(DX_FAMILIES) == 7


# ---- data, reference, runs ----------------------------------------------------------------------------------------------
def _limit(layer):
    """2^24 / 64 where an F(2x2,3x3) family can take the shape in some direction, 2^24 elsewhere"""
    n, c, h, w, f, k, st, pad, g = layer
    return LIMIT if (k == 3 and st == 1 and pad == 1 and g == 1 and min(c, f) >= 16) else 2.0 ** 24


def _data(layer):
    """the integers of tests/test_conv_dw_ladder.py; the last filter of every group has a bias of exactly 1.0; dyadic slopes
    of both signs, drawn per filter (no period that a group size could share: the groups' slopes differ, and so do their
    absolute values, which the backward side uses -- test_the_cases_agree_with_the_port_of_the_shape_rules)"""
    n, c, h, w, f, k, st, pad, g = layer
    t = _integers(layer)
    for gi in range(g):
        t["b"][(gi + 1) * (f // g) - 1] = 1.0
    rs = np.random.RandomState(sum(layer) + 7)
    sl = (rs.randint(1, 8, f) * rs.choice([-1, 1], f)).astype(np.float32) / 8   # +-1/8 .. +-7/8, drawn per filter
    t["slopes"] = torch.from_numpy(sl)
    return t


def _forward_candidates(z, act, slopes):
    """what the fused epilogue may store for the float64 value z (an integer): one float32 tensor, two for RAMP"""
    f = z.shape[1]
    tenth = float(np.float32(0.1))
    pos = z * (z > 0)
    if act == NONE:
        want = [z]
    elif act == RELU:
        want = [pos]
    elif act == PRELU:
        want = [torch.where(z > 0, z, z * slopes.double().view(1, f, 1, 1))]
    elif act == ABS:
        want = [z.abs()]
    elif act == CLAMP:
        want = [z.clamp(0.0, 1.0)]
    elif act == LRELU:
        return [torch.where(z > 0, z, tenth * z).float()]      # one rounding of the exact product
    elif act == RAMP:
        # tenth * z and the sums below are exact in float64 (24 + 24 bits): one rounding (fma) or two
        return [(pos + tenth * z).float(), (pos + (tenth * z).float().double()).float()]
    for v in want:
        assert torch.equal(v.float().double(), v), act          # exactly representable
    return [v.float() for v in want]


def _guarded(shape):
    """a NaN tensor of `shape` inside a larger buffer that holds the sentinel for GUARD floats on both sides"""
    numel = int(np.prod(shape))
    whole = torch.full((numel + 2 * GUARD,), SENTINEL, device=DEV)
    view = whole[GUARD:GUARD + numel].view(shape)
    view.fill_(float("nan"))
    return whole, view


def _guard_ok(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def _differ(got, cands):
    ok = torch.zeros(got.shape, dtype=torch.bool)
    for v in cands:
        ok |= got == v
    return int((~ok).sum())


@functools.lru_cache(maxsize=None)
def _ran(i):
    """case i once: the traces of its forward and backward runs and everything that was wrong, as text (shared by its own
    test and the row coverage; the tensors are not kept)"""
    from bcnn_amd import ops
    layer, acts, want_fwd, want_dx = CASES[i]
    n, c, h, w, f, k, st, pad, g = layer
    oh, ow = _out_hw(layer)
    bact = (NONE, RELU, PRELU)[i % 3]
    t = _data(layer)
    bslopes = t["slopes"].abs()
    ref, largest = _reference(t, layer, bact, bslopes)
    d = {key: v.to(DEV) for key, v in t.items()}
    wrong, traces = [], dict(fwd=set(), dx=set())
    if not largest < _limit(layer):
        wrong.append("precondition: the absolute values reach %g" % largest)
    for act in (acts if want_fwd is not None else ()):
        cands = _forward_candidates(ref["z"], act, t["slopes"])
        ys = []
        for rep in range(2):
            whole, y = _guarded((n, f, oh, ow))
            _trace_start()
            ops.conv_forward(d["x"], d["w"], d["b"], y, k, st, pad, g, act, d["slopes"] if act == PRELU else None)
            tr = _pick(_trace_stop(), FWD_NAMES)
            torch.cuda.synchronize()
            if tr != want_fwd:
                wrong.append("forward act %d ran on %s" % (act, sorted(tr)))
            if not _guard_ok(whole):
                wrong.append("forward act %d wrote outside y" % act)
            traces["fwd"] |= tr
            ys.append(y)
        bad = _differ(ys[0].cpu(), cands)
        if bad:
            wrong.append("forward act %d: %d of %d elements of y differ" % (act, bad, ys[0].numel()))
        if not torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32)):
            wrong.append("forward act %d: a second run gave other bits" % act)
    # backward from the reference's y: dy * act'(y) in place, the weight gradient (not compared here), then dx
    y = ref["y"].float().to(DEV)
    wsw, ws = _workspace(ops, layer)
    dxs = []
    for rep in range(2):
        whole, dx = _guarded((n, c, h, w))
        dw, db = d["dw0"].clone(), d["db0"].clone()
        _trace_start()
        ops.conv_backward(d["x"], d["w"], y, d["dy"].clone(), dx, dw, db, k, st, pad, g, bact, ws,
                          slopes=bslopes.to(DEV) if bact == PRELU else None,
                          dslopes=torch.zeros(f, device=DEV) if bact == PRELU else None)
        tr = _pick(_trace_stop(), DX_NAMES)
        torch.cuda.synchronize()
        if tr != want_dx:
            wrong.append("data gradient ran on %s" % sorted(tr))
        if not _guard_ok(whole):
            wrong.append("the data gradient wrote outside dx")
        traces["dx"] |= tr
        dxs.append(dx)
    if not bool((wsw[ws.numel():] == SENTINEL).all()):
        wrong.append("written behind conv_workspace_size floats")
    try:
        _assert_exact(dict(ref=ref, largest=largest, got=dict(dx=dxs[0].cpu())), layer, keys=("dx",), limit=_limit(layer))
    except AssertionError as e:
        wrong.append(str(e))
    if not torch.equal(dxs[0].view(torch.int32), dxs[1].view(torch.int32)):
        wrong.append("a second run gave another dx")
    return dict(traces=traces, wrong=wrong, bact=bact)


@gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_family_takes_the_layer_and_is_exact_on_integers(i):
    layer = CASES[i][0]
    r = _ran(i)
    print("%s: forward (acts %s) on %s; dX (act %d) on %s" % (layer, CASES[i][1], ", ".join(sorted(r["traces"]["fwd"])) or "-",
                                                            r["bact"], ", ".join(sorted(r["traces"]["dx"]))))
    assert r["wrong"] == [], (layer, r["wrong"])


def _bn(f, shape):
    Z = lambda: torch.zeros(f, device=DEV)
    whole, raw = _guarded(shape)
    return whole, dict(run_mean=Z(), run_var=Z(), scales=torch.ones(f, device=DEV), saved_mean=Z(), saved_var=Z(), workspace=raw)


def _rel(a, r):
    return float((a.double() - r).abs().max() / max(float(r.abs().max()), 1e-30))


@functools.lru_cache(maxsize=None)
def _ran_raw(j):
    from bcnn_amd import ops
    layer, want = RAW[j]
    n, c, h, w, f, k, st, pad, g = layer
    oh, ow = _out_hw(layer)
    t = _data(layer)
    d = {key: v.to(DEV) for key, v in t.items()}
    z = F.conv2d(t["x"].double(), t["w"].double(), None, st, pad, 1, g)
    largest = float(F.conv2d(t["x"].double().abs(), t["w"].double().abs(), None, st, pad, 1, g).max())
    out = []
    for rep in range(2):
        whole, bn = _bn(f, (n, f, oh, ow))
        y = torch.empty((n, f, oh, ow), device=DEV)
        _trace_start()
        ops.conv_forward(d["x"], d["w"], d["b"], y, k, st, pad, g, NONE, None, bn, ops.MODE_TRAIN)
        tr = _pick(_trace_stop(), FWD_NAMES)
        torch.cuda.synchronize()
        out.append((whole, bn, tr))
    (whole, bn, tr), (_, bn2, _) = out
    mean = z.mean(dim=(0, 2, 3))
    var = (z * z).mean(dim=(0, 2, 3)) - mean * mean
    return dict(trace=tr, largest=largest, guard=_guard_ok(whole), bad=_differ(bn["workspace"].cpu(), [z.float()]),
                exact_ref=torch.equal(z.float().double(), z), mean=_rel(bn["saved_mean"].cpu(), mean),
                var=_rel(bn["saved_var"].cpu(), var), min_var=float(var.min()), max_var=float(var.max()),
                repeat=all(torch.equal(bn[key], bn2[key]) for key in ("workspace", "saved_mean", "saved_var")))


@gpu
@pytest.mark.parametrize("j", range(len(RAW)), ids=RAW_IDS)
def test_the_raw_forward_is_exact_and_its_statistics_are_the_batch_moments(j):
    """bn["workspace"] (the bare convolution) equals float64; saved_mean / saved_var divide: the bars of
    tests/test_winograd_ksplit.py, 1e-5 of the largest mean (no F(4x4,3x3) kernel here) and 1e-4 of the largest variance"""
    layer, want = RAW[j]
    r = _ran_raw(j)
    print("raw forward of %s on %s: saved_mean %.2e of 1e-5, saved_var %.2e of 1e-4 (variances %.3g .. %.3g)" % (
        layer, ", ".join(sorted(r["trace"])), r["mean"], r["var"], r["min_var"], r["max_var"]))
    assert r["trace"] == want, (layer, sorted(r["trace"]))
    assert r["largest"] < _limit(layer) and r["exact_ref"], (layer, r["largest"])
    assert r["min_var"] > 0.1 * r["max_var"], (layer, "variances near zero")
    assert r["bad"] == 0, (layer, "%d elements of the bare convolution differ" % r["bad"])
    assert r["mean"] <= 1e-5 and r["var"] <= 1e-4, (layer, r["mean"], r["var"])
    assert r["repeat"], (layer, "a second run gave other bits")
    assert r["guard"], (layer, "written outside the batch-norm workspace")


@functools.lru_cache(maxsize=None)
def _ran_w43():
    """the F(4x4,3x3) rows on float data (their transforms divide by 6, 12 and 24): tests/test_winograd43.py and
    tests/test_winograd43_dw.py own them, here they only have to be hit"""
    from bcnn_amd import ops
    layer = W43_LAYER
    n, c, h, w, f, k, st, pad, g = layer
    t = _float_case(layer, 43)
    d = {key: v.to(DEV) for key, v in t.items()}
    whole_raw, bn = _bn(f, (n, f, h, w))
    y = torch.empty((n, f, h, w), device=DEV)
    _trace_start()
    ops.conv_forward(d["x"], d["w"], d["b"], y, k, st, pad, g, NONE, None, bn, ops.MODE_TRAIN)
    tr_fwd = _pick(_trace_stop(), FWD_NAMES)
    whole_dx, dx = _guarded((n, c, h, w))
    wsw, ws = _workspace(ops, layer)
    _trace_start()
    ops.conv_backward(d["x"], d["w"], y, d["dy"].clone(), dx, torch.zeros_like(d["w"]), torch.zeros(f, device=DEV), k, st, pad,
                      g, NONE, ws)
    tr_dx = _pick(_trace_stop(), DX_NAMES)
    torch.cuda.synchronize()
    z = F.conv2d(t["x"].double(), t["w"].double(), None, st, pad)
    dxr = F.conv_transpose2d(t["dy"].double(), t["w"].double(), None, st, pad)
    mean = z.mean(dim=(0, 2, 3))
    var = (z * z).mean(dim=(0, 2, 3)) - mean * mean
    elementwise = lambda a, r: float(((a.double() - r).abs() / (1e-4 * r.abs() + 1e-5 * float(r.abs().max()))).max())
    raw, dxc = bn["workspace"].cpu(), dx.cpu()
    return dict(fwd=tr_fwd, dx=tr_dx, guard=_guard_ok(whole_raw) and _guard_ok(whole_dx), raw_rel=_rel(raw, z),
                raw_el=elementwise(raw, z), dx_rel=_rel(dxc, dxr), dx_el=elementwise(dxc, dxr),
                mean=_rel(bn["saved_mean"].cpu(), mean), var=_rel(bn["saved_var"].cpu(), var))


@gpu
def test_the_winograd43_rows_are_hit_at_their_float_bars():
    r = _ran_w43()
    print("F(4x4,3x3) on %s: raw forward %.2e of 3e-5 (worst element %.3f of its bound), dX %.2e of 3e-5 (%.3f), saved_mean "
          "%.2e of 3e-5, saved_var %.2e of 1e-4" % (W43_LAYER, r["raw_rel"], r["raw_el"], r["dx_rel"], r["dx_el"], r["mean"],
                                                    r["var"]))
    assert r["fwd"] == W43_F and r["dx"] == W43_D, (sorted(r["fwd"]), sorted(r["dx"]))
    assert r["raw_rel"] <= 3e-5 and r["raw_el"] <= 1.0, (r["raw_rel"], r["raw_el"])
    assert r["dx_rel"] <= 3e-5 and r["dx_el"] <= 1.0, (r["dx_rel"], r["dx_el"])
    assert r["mean"] <= 3e-5 and r["var"] <= 1e-4, (r["mean"], r["var"])
    assert r["guard"]


@gpu
def test_the_second_chunk_of_the_few_channel_data_gradient():
    """D5: per_image = 27 * 50176 floats of col, 18 images fit in 96 MiB, image 18 is a chunk of its own with n0 = 18 offsets into
    dy and dx. Every image against float64, image by image (dx[n] depends on dy[n] only). The weight gradient runs with the
    call and is not looked at."""
    from bcnn_amd import ops
    layer = CHUNK_LAYER
    n, c, h, w, f, k, st, pad, g = layer
    per_image = c * k * k * h * w
    assert (96 << 20) // (per_image * 4) == 18 and n == 19
    rs = np.random.RandomState(5)
    wt = torch.from_numpy(rs.randint(-1, 2, (f, c, k, k)).astype(np.float32))
    dy = torch.from_numpy(rs.randint(-1, 2, (n, f, h, w)).astype(np.float32))
    assert f * k * k < 2.0 ** 24                                   # the convolution of the absolute values, at most
    x = torch.zeros((n, c, h, w), device=DEV)
    whole, dx = _guarded((n, c, h, w))
    dyd, wd = dy.to(DEV), wt.to(DEV)
    wsw, ws = _workspace(ops, layer)
    dw, db = torch.zeros_like(wd), torch.zeros(f, device=DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _trace_start()
    ops.conv_backward(x, wd, dyd, dyd, dx, dw, db, k, st, pad, g, NONE, ws)
    trace = _pick(_trace_stop(), DX_NAMES)
    torch.cuda.synchronize()
    print("dX of %s on %s: %.2f ms with its weight gradient" % (layer, ", ".join(sorted(trace)),
                                                               1e3 * (time.perf_counter() - t0)))
    assert trace == SMALLC_D, sorted(trace)
    got = dx.cpu()
    for i in range(n):
        want = F.conv_transpose2d(dy[i:i + 1].double(), wt.double(), None, st, pad)
        assert torch.equal(want.float().double(), want)
        bad = int((got[i:i + 1] != want.float()).sum())
        assert bad == 0, "image %d: %d of %d elements of dx differ" % (i, bad, want.numel())
    assert _guard_ok(whole) and bool((wsw[ws.numel():] == SENTINEL).all())
    dx2 = torch.full_like(dx, float("nan"))
    ops.conv_backward(x, wd, dyd, dyd, dx2, dw, db, k, st, pad, g, NONE, ws)
    torch.cuda.synchronize()
    assert torch.equal(dx.view(torch.int32), dx2.view(torch.int32))


@gpu
def test_every_row_of_both_tables_is_hit():
    fwd, dx = set(), set()
    for i in range(len(CASES)):
        r = _ran(i)
        fwd |= r["traces"]["fwd"]
        dx |= r["traces"]["dx"]
    for j in range(len(RAW)):
        fwd |= _ran_raw(j)["trace"]
    r = _ran_w43()
    fwd |= r["fwd"]
    dx |= r["dx"]
    assert [k for k in FWD_FAMILIES if k not in fwd] == [], sorted(fwd)
    assert [k for k in DX_FAMILIES if k not in dx] == [], sorted(dx)
    assert sorted(SUB_BRANCHES - fwd - dx) == [], (sorted(fwd), sorted(dx))
