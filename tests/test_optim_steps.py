"""The optimiser steps of csrc/blas1.hip through the C-ABI -- bcnn_hip_sgd_update, bcnn_hip_adam_update,
bcnn_hip_sgd_update_chunks, bcnn_hip_zero_chunks -- against the float32 restatement of tests/_optim_ref.py (pinned to the
reference's arithmetic by test_optim_ref_pinning.py), bit for bit.

Every device buffer is a view between two bands of sentinel words (_next_ref.Guarded). What each size reaches:
  sgd_kernel / adam_kernel     one element per thread, the grid capped at 2048 workgroups of 256: 524 288 elements are one
                               sweep exactly, 524 289 put one element into the second, 2 * 524 288 + 77 a partial third
  sgd_chunks_kernel            one workgroup per table entry, `num_chunks` of them (no cap): counts either side of 256
                               (the workgroup's stride) and at BCNN_HIP_SGD_CHUNK, 3000 entries past the stream cap
  zero_chunks_kernel           scalar head up to a 16-byte boundary (0..3 elements, more than the chunk holds when
                               count < head), float4 body, scalar tail
"""
import ctypes as C

import numpy as np
import pytest

from tests import _next_ref as R
from tests import _optim_ref as O

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  (first, so that one HIP runtime serves torch and the library)
    from bcnn_amd import _lib
    return _lib.load()


def f(x):
    return C.c_float(x)


def garbage(n, seed):
    return np.random.RandomState(seed).uniform(-3, 3, n).astype(F32)


# ---- bcnn_hip_sgd_update ------------------------------------------------------------------------------------------------------
def sgd_on_device(L, w, b, dw, db, batch, momentum, decay, shift=0):
    g = [R.Guarded(a, shift) for a in (w, b, dw, db)]
    L.bcnn_hip_sgd_update(g[0].ptr, g[1].ptr, g[2].ptr, g[3].ptr, w.size, b.size, batch, f(O.LR), f(momentum), f(decay))
    L.bcnn_hip_sync()
    return [a.read() for a in g]


def check_sgd_steps(L, w_size, b_size, momentum, decay, batch, shift=0):
    cs = O.inputs(w_size, b_size, batch)
    tag = "sgd w%d b%d m%g d%g B%d s%d" % (w_size, b_size, momentum, decay, batch, shift)
    want = [cs["w0"], cs["b0"], np.zeros(w_size, F32), np.zeros(b_size, F32)]
    got = [a.copy() for a in want]
    for t in range(O.STEPS):                      # the gradient buffers carry g * momentum into the next step
        want[2], want[3] = want[2] + cs["dw"][t], want[3] + cs["db"][t]
        got[2], got[3] = got[2] + cs["dw"][t], got[3] + cs["db"][t]
        want = list(O.sgd_update(*want, batch, O.LR, momentum, decay))
        got = sgd_on_device(L, *got, batch, momentum, decay, shift)
        for name, a, e in zip(("w", "b", "dw", "db"), got, want):
            R.assert_bits("%s step %d %s" % (tag, t, name), a, e)


@pytest.mark.parametrize("w_size,b_size", O.SIZES)
def test_sgd_update_is_the_restatement_in_bits(L, w_size, b_size):
    for momentum, decay in O.SGD_HYPER:
        for batch in O.BATCHES:
            check_sgd_steps(L, w_size, b_size, momentum, decay, batch)


@pytest.mark.parametrize("w_size,b_size", [(257, 5), (O.SWEEP + 1, 257)])
def test_sgd_update_on_misaligned_buffers(L, w_size, b_size):
    check_sgd_steps(L, w_size, b_size, 0.9, 5e-4, 16, shift=1)


def test_sgd_update_skips_an_absent_side(L):
    cs = O.inputs(257, 5, 16)
    w0, b0, dw0, db0 = cs["w0"], cs["b0"], cs["dw"][0], cs["db"][0]
    ew, eb, edw, edb = O.sgd_update(w0, b0, dw0, db0, 16, O.LR, 0.9, 5e-4)
    args = (16, f(O.LR), f(0.9), f(5e-4))
    for null in ("w", "dw", "w_size"):            # the weights side is absent, the biases step
        w, b, dw, db = (R.Guarded(a) for a in (w0, b0, dw0, db0))
        L.bcnn_hip_sgd_update(None if null == "w" else w.ptr, b.ptr, None if null == "dw" else dw.ptr, db.ptr,
                              0 if null == "w_size" else 257, 5, *args)
        L.bcnn_hip_sync()
        w.assert_unchanged("w, no " + null)
        dw.assert_unchanged("dw, no " + null)
        R.assert_bits("b, no " + null, b.read(), eb)
        R.assert_bits("db, no " + null, db.read(), edb)
    for null in ("b", "db", "b_size"):            # the converse
        w, b, dw, db = (R.Guarded(a) for a in (w0, b0, dw0, db0))
        L.bcnn_hip_sgd_update(w.ptr, None if null == "b" else b.ptr, dw.ptr, None if null == "db" else db.ptr,
                              257, 0 if null == "b_size" else 5, *args)
        L.bcnn_hip_sync()
        b.assert_unchanged("b, no " + null)
        db.assert_unchanged("db, no " + null)
        R.assert_bits("w, no " + null, w.read(), ew)
        R.assert_bits("dw, no " + null, dw.read(), edw)


# ---- bcnn_hip_adam_update -----------------------------------------------------------------------------------------------------
NAMES6 = ("w", "b", "dw", "db", "m", "v")


def adam_on_device(L, st, it, beta1, beta2, decay):
    g = [R.Guarded(a) for a in st]
    L.bcnn_hip_adam_update(*[a.ptr for a in g], st[0].size, st[1].size, O.ADAM_BATCH, it, f(beta1), f(beta2), f(O.LR),
                           f(O.ADAM_MOMENTUM), f(decay))
    L.bcnn_hip_sync()
    return [a.read() for a in g]


@pytest.mark.parametrize("w_size,b_size", O.SIZES)
def test_adam_update_is_the_restatement_in_bits(L, w_size, b_size):
    cs = O.inputs(w_size, b_size, O.ADAM_BATCH)
    zb = O.zero_block(w_size)
    for beta1, beta2, iters in O.ADAM_HYPER:
        for decay in O.ADAM_DECAYS:
            tag = "adam w%d b%d (%g, %g) d%g" % (w_size, b_size, beta1, beta2, decay)
            want = [cs["w0"], cs["b0"], np.zeros(w_size, F32), np.zeros(b_size, F32), cs["m0"], cs["v0"]]
            got = [a.copy() for a in want]
            for t, it in enumerate(iters):        # m, v and the biases' momentum are carried from step to step
                want[2], want[3] = want[2] + cs["dw"][t], want[3] + cs["db"][t]
                got[2], got[3] = got[2] + cs["dw"][t], got[3] + cs["db"][t]
                before = got[0].copy()
                want = list(O.adam_update(*want, O.ADAM_BATCH, it, beta1, beta2, O.LR, O.ADAM_MOMENTUM, decay))
                got = adam_on_device(L, got, it, beta1, beta2, decay)
                for name, a, e in zip(NAMES6, got, want):
                    R.assert_bits("%s iter %d %s" % (tag, it, name), a, e)
                assert not np.any(R.bits(got[2])), tag + ": dw is +0 everywhere after the step"
                if decay == 0:                    # g == m == v == 0: 0 / (0 + 1e-7), the weights keep their bits
                    R.assert_bits(tag + " w of the zero block", got[0][zb], before[zb])
                    assert not np.any(R.bits(got[4][zb])) and not np.any(R.bits(got[5][zb])), tag + ": m, v stay +0"


# ---- bcnn_hip_sgd_update_chunks -----------------------------------------------------------------------------------------------
class SgdChunk(C.Structure):
    _fields_ = [("w_d", C.c_void_p), ("g_d", C.c_void_p), ("count", C.c_uint), ("use_decay", C.c_uint)]


class FillChunk(C.Structure):
    _fields_ = [("p_d", C.c_void_p), ("count", C.c_uint), ("reserved", C.c_uint)]


def device_table(entries):
    """the ctypes array on the device (a tensor the caller keeps alive)"""
    import torch
    raw = np.frombuffer(bytes(entries), np.uint8).copy()
    return torch.from_numpy(raw).to(R.DEVICE)


def test_chunk_structs_have_the_header_layout():
    """include/bcnn_hip.h: bcnn_hip_sgd_chunk is two pointers and two unsigned ints (24 bytes), bcnn_hip_fill_chunk one
    pointer and two unsigned ints (16 bytes); the device code indexes its tables by these sizes"""
    assert C.sizeof(C.c_void_p) == 8
    assert C.sizeof(SgdChunk) == 24 and (SgdChunk.g_d.offset, SgdChunk.count.offset, SgdChunk.use_decay.offset) == (8, 16, 20)
    assert C.sizeof(FillChunk) == 16 and (FillChunk.count.offset, FillChunk.reserved.offset) == (8, 12)


def layout(counts, gap):
    """offsets of the entries in an arena: never a multiple of 4 floats, `gap` or more untouched floats between two"""
    offs, pos = [], 1
    for i, n in enumerate(counts):
        pos += (1 + i % 3 - pos) % 4                # offset % 4 cycles through 1, 2, 3
        offs.append(pos)
        pos += n + gap
    return offs, pos


COUNTS = [1, 63, 255, 256, 257, 2047, 2048]
TABLES = {"counts": (COUNTS * 2, 5),                                     # 7 is odd: every count under use_decay 0 and 1
          "3000x64": ([64] * 3000, 3)}                                   # more workgroups than the stream cap


@pytest.mark.parametrize("momentum,decay,batch", [(0.9, 5e-4, 16), (1.0, 5e-4, 1), (0.0, 0.0, 16)])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_sgd_update_chunks(L, table, momentum, decay, batch):
    counts, gap = TABLES[table]
    offs, total = layout(counts, gap)
    w0, g0 = garbage(total, 11), garbage(total, 12)
    use = [i % 2 for i in range(len(counts))]
    if table == "counts":
        assert {(n, u) for n, u in zip(counts, use)} >= {(n, u) for n in COUNTS for u in (0, 1)}
    neg, wd = O.neg_lr_b(O.LR, batch), O.wd_b(decay, batch)
    ew, eg = w0.copy(), g0.copy()
    for o, n, u in zip(offs, counts, use):
        ew[o:o + n], eg[o:o + n] = O.sgd_step(w0[o:o + n], g0[o:o + n], wd if u else F32(0), neg, momentum)
    args = (batch, f(O.LR), f(momentum), f(decay))

    gw, gg = R.Guarded(w0), R.Guarded(g0)
    entries = (SgdChunk * len(counts))(*[SgdChunk(gw.ptr + 4 * o, gg.ptr + 4 * o, n, u)
                                         for o, n, u in zip(offs, counts, use)])
    dev = device_table(entries)
    L.bcnn_hip_sgd_update_chunks(dev.data_ptr(), 0, *args)               # no entries: nothing moves
    L.bcnn_hip_sync()
    gw.assert_unchanged("w, num_chunks 0")
    gg.assert_unchanged("g, num_chunks 0")
    L.bcnn_hip_sgd_update_chunks(dev.data_ptr(), len(counts), *args)
    L.bcnn_hip_sync()
    cw, cg = gw.read(), gg.read()
    R.assert_bits("chunks w (entries and gaps)", cw, ew)
    R.assert_bits("chunks g (entries and gaps)", cg, eg)
    assert np.array_equal(dev.cpu().numpy(), np.frombuffer(bytes(entries), np.uint8)), "the table is read-only"

    # the same parameters through bcnn_hip_sgd_update, buffer by buffer: weights rule or biases rule
    gw, gg = R.Guarded(w0), R.Guarded(g0)
    for o, n, u in zip(offs, counts, use):
        wp, gp = gw.ptr + 4 * o, gg.ptr + 4 * o
        if u:
            L.bcnn_hip_sgd_update(wp, None, gp, None, n, 0, *args)
        else:
            L.bcnn_hip_sgd_update(None, wp, None, gp, 0, n, *args)
    L.bcnn_hip_sync()
    R.assert_bits("per-buffer w against the chunked launch", gw.read(), cw)
    R.assert_bits("per-buffer g against the chunked launch", gg.read(), cg)


# ---- bcnn_hip_zero_chunks -----------------------------------------------------------------------------------------------------
ZERO_COUNTS = [1, 2, 3, 4, 5, 7, 8, 1023, 1027, 16384]


def nan_words(n):
    return np.full(n, R.SENTINEL, np.uint32).view(F32)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_zero_chunks_one_entry(L, shift):
    for n in ZERO_COUNTS:                          # shift 1 leaves a head of 3: counts 1 and 2 end inside it
        buf = R.Guarded(nan_words(n), shift)
        entries = (FillChunk * 1)(FillChunk(buf.ptr, n, 0))
        dev = device_table(entries)
        L.bcnn_hip_zero_chunks(dev.data_ptr(), 0)
        L.bcnn_hip_sync()
        buf.assert_unchanged("num_chunks 0")
        L.bcnn_hip_zero_chunks(dev.data_ptr(), 1)
        L.bcnn_hip_sync()
        got = buf.read()                           # asserts the bands
        assert not np.any(R.bits(got)), "shift %d count %d: %d words are not +0" % (shift, n, np.count_nonzero(R.bits(got)))


def test_zero_chunks_table_of_mixed_alignments(L):
    counts = [n for n in ZERO_COUNTS for _ in range(4)]
    offs, pos = [], 0
    for i, n in enumerate(counts):
        pos += (i % 4 - pos) % 4                   # offset % 4 cycles through 0, 1, 2, 3 under every count
        offs.append(pos)
        pos += n + 5
    arena = R.Guarded(nan_words(pos))
    want = arena.host[arena.start:arena.start + arena.n].copy()
    for o, n in zip(offs, counts):
        want[o:o + n] = 0
    entries = (FillChunk * len(counts))(*[FillChunk(arena.ptr + 4 * o, n, 0) for o, n in zip(offs, counts)])
    dev = device_table(entries)
    L.bcnn_hip_zero_chunks(dev.data_ptr(), len(counts))
    L.bcnn_hip_sync()
    got = R.bits(arena.read())
    assert np.array_equal(got, want), "%d words differ (chunks +0, every word between them unchanged)" % np.count_nonzero(got != want)
