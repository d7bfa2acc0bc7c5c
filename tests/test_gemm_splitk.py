"""bcnn_hip_gemm (csrc/gemm.hip) at the shapes the five single-pass goldens do not reach: several 64 x 64 tiles under
every transpose combination, the split-K path (gemm_kernel writing `partials`, gemm_splitk_finalize_kernel applying
alpha / beta), leading dimensions larger than the rows, and gemm_scale_kernel (k <= 0 or alpha == 0).

With kCUs = 256 the dispatcher splits when ceil(m / 64) * ceil(n / 64) < 128 and ceil(k / 16) >= 16:
    (70, 130, 200)   6 tiles, 13 k-tiles: one pass, ragged last tile in m, n and k
    (5, 37, 512)     32 k-tiles -> 8 splits of 4 (the full-connected forward in miniature)
    (40, 70, 530)    34 k-tiles -> 8 wanted, 5 tiles per split, re-derived 7 splits; the last holds 4 tiles, the last tile 2 columns
    (33, 65, 241)    16 k-tiles -> 4 splits of 4; two column tiles, the second one element wide; the last k-tile 1 column
    (3, 5, 300)      19 k-tiles -> 4 splits of 5, the last holds 4
    (70, 130, 530)   6 output tiles x 7 splits: the partial-tile index with several row and column tiles
The reference is float64 alpha op(A) op(B) + beta C0 (tests/_next_ref.py); C is a guarded view and C0 finite garbage."""
import ctypes as C

import numpy as np
import pytest

from tests import _golden as G
from tests import _next_ref as R
from tests.test_hip_parity import REL_TOL

F32 = np.float32
UNSPLIT = (70, 130, 200)
SPLIT = [(5, 37, 512), (40, 70, 530), (33, 65, 241), (3, 5, 300), (70, 130, 530)]
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
ALPHA_BETA = [(1.0, 0.0), (1.0, 1.0), (0.5, 2.0)]


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401
    from bcnn_amd import _lib
    return _lib.load()


def expected_splits(m, n, k):
    """the dispatcher's arithmetic restated, so that a case named "split" is known to split"""
    tiles, ktiles = -(-n // 64) * -(-m // 64), -(-k // 16)
    splits = 1
    if tiles < 128 and ktiles >= 16:
        splits = max(1, min(512 // tiles, ktiles // 4, 32))
    per = -(-ktiles // splits)
    return -(-ktiles // per), per, ktiles


def test_the_chosen_shapes_split_as_described():
    assert expected_splits(*UNSPLIT)[0] == 1
    assert expected_splits(5, 37, 512) == (8, 4, 32)
    assert expected_splits(40, 70, 530) == (7, 5, 34)
    assert expected_splits(33, 65, 241) == (4, 4, 16)
    assert expected_splits(3, 5, 300) == (4, 5, 19)
    assert expected_splits(70, 130, 530) == (7, 5, 34)


def run_gemm(L, ta, tb, m, n, k, alpha, beta, pad, seed=0):
    lda = (m if ta else k) + pad
    ldb = (k if tb else n) + pad
    ldc = n + pad
    A, B, C0 = R.gemm_operands(ta, tb, m, n, k, max(lda, 1), max(ldb, 1), ldc, 1000 * ta + 100 * tb + m + n + k + seed)
    ga, gb, gc = R.Guarded(A), R.Guarded(B), R.Guarded(C0)
    L.bcnn_hip_gemm(ta, tb, m, n, k, C.c_float(alpha), ga.ptr, max(lda, 1), gb.ptr, max(ldb, 1), C.c_float(beta), gc.ptr, ldc)
    L.bcnn_hip_sync()
    ga.assert_unchanged("A")
    gb.assert_unchanged("B")
    got = gc.read().reshape(m, ldc)
    assert np.array_equal(R.bits(got[:, n:]), R.bits(C0[:, n:])), "the padding columns of C were written"
    return got[:, :n], A, B, C0


def check_gemm(L, ta, tb, m, n, k, pad):
    for alpha, beta in ALPHA_BETA:
        tag = "gemm/t%d%d/%dx%dx%d/pad%d/a%g_b%g" % (ta, tb, m, n, k, pad, alpha, beta)
        got, A, B, C0 = run_gemm(L, ta, tb, m, n, k, alpha, beta, pad)
        want, bound = R.gemm64(ta, tb, m, n, k, alpha, A, B, beta, C0)
        assert np.all(np.isfinite(got)), tag
        G.assert_close(tag, got, want, REL_TOL)
        ratio = np.abs(got.astype(np.float64) - want) / bound
        i = np.unravel_index(ratio.argmax(), ratio.shape)
        assert ratio[i] <= 1.0, "%s: C%s is %.9g, want %.9g: %.2f x the forward-error bound" % (tag, i, got[i], want[i], ratio[i])


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("ta,tb", TRANS)
def test_gemm_several_tiles_one_pass(L, ta, tb, pad):
    check_gemm(L, ta, tb, *UNSPLIT, pad)


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("m,n,k", SPLIT)
def test_gemm_split_k(L, m, n, k, ta, tb, pad):
    check_gemm(L, ta, tb, m, n, k, pad)


@pytest.mark.gpu
@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("k,alpha", [(0, 1.0), (16, 0.0)], ids=["k0", "alpha0"])
def test_gemm_scale_path(L, k, alpha, beta):
    m, n = 33, 65
    got, _, _, C0 = run_gemm(L, 0, 1, m, n, k, alpha, beta, 3)
    if beta == 1.0:
        want = C0[:, :n]
    elif beta == 0.0:
        want = np.zeros((m, n), F32)
    else:
        want = C0[:, :n] * F32(beta)
    R.assert_bits("gemm_scale/k%d/a%g/b%g" % (k, alpha, beta), got, want)


@pytest.mark.gpu
def test_gemm_split_k_is_deterministic(L):
    m, n, k = SPLIT[1]
    first = run_gemm(L, 0, 1, m, n, k, 0.5, 2.0, 3)[0]
    second = run_gemm(L, 0, 1, m, n, k, 0.5, 2.0, 3)[0]
    R.assert_bits("gemm split-K run twice", second, first)      # the finalize adds the splits in order
