"""Plain numpy restatement of the optimiser steps of csrc/blas1.hip (sgd_kernel, sgd_chunks_kernel, adam_kernel), for
test_optim_steps.py. TEST INFRASTRUCTURE ONLY.

Everything is float32 with ONE rounding per operation: a numpy float32 array times a np.float32 scalar is one correctly
rounded product, the sum after it one correctly rounded sum (numpy never contracts the two), np.sqrt and the division are
correctly rounded as well. The host scalars are formed in np.float32 in the order bcnn_hip_sgd_update /
bcnn_hip_adam_update form them; powf and sqrtf of the bias correction come from the C library, the libm the shared
library itself links. test_optim_ref_pinning.py runs these forms against oracle/bcnn_oracle.c (orc_sgd_update,
orc_adam_update) on the CPU, so they are a statement of the reference and not of the HIP code.

The module also makes the inputs the GPU test and the pinning test share."""
import ctypes as C
import ctypes.util
import functools

import numpy as np

F32 = np.float32

SWEEP = 2048 * 256                     # threads of one capped stream_grid launch: one element each in sgd / adam
W_SIZES = [1, 255, 256, 257, SWEEP, SWEEP + 1, 2 * SWEEP + 77]
B_SIZES = [1, 5, 257]
SMALL = [(w, B_SIZES[i % 3]) for i, w in enumerate(W_SIZES) if w < SWEEP]      # what the CPU pinning test runs
SIZES = [(w, B_SIZES[i % 3]) for i, w in enumerate(W_SIZES)]                   # every b_size under small and large w_size
SGD_HYPER = [(0.9, 5e-4), (0.0, 0.0), (1.0, 5e-4), (0.9, 0.0)]                 # (momentum, decay)
BATCHES = [1, 16]
LR = 0.01
# (beta1, beta2, iter of each step)
ADAM_HYPER = [(0.5, 0.75, (1,)),               # both powers exact: mu does not depend on libm
              (0.9, 0.999, (0,)),
              (0.9, 0.999, (4, 8, 12)),         # three steps, m and v carried
              (0.8, 0.99, (1000000,))]          # the powers underflow, mu == 1
ADAM_DECAYS = [0.0, 5e-4]
ADAM_BATCH, ADAM_MOMENTUM = 4, 0.9
STEPS = 3
SEED = 20240611


@functools.lru_cache(maxsize=None)
def _libm():
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.powf.restype, m.powf.argtypes = C.c_float, [C.c_float, C.c_float]
    m.sqrtf.restype, m.sqrtf.argtypes = C.c_float, [C.c_float]
    return m


# ---- host scalars -----------------------------------------------------------------------------------------------------------
def neg_lr_b(lr, batch):
    """-lr / batch_size: the negation is exact, the int converts to float, one float division"""
    return F32(-F32(lr)) / F32(batch)


def wd_b(decay, batch):
    """decay * batch_size"""
    return F32(decay) * F32(batch)


def adam_mu(beta1, beta2, it):
    """sqrtf(1.0f - powf(beta2, (float)iter + 1)) / (1.0f - powf(beta1, (float)iter + 1))"""
    m = _libm()
    e = F32(F32(it) + F32(1))
    num = F32(m.sqrtf(F32(1) - F32(m.powf(F32(beta2), e))))
    return num / (F32(1) - F32(m.powf(F32(beta1), e)))


# ---- the steps --------------------------------------------------------------------------------------------------------------
def sgd_step(w, g, wd, neg, momentum):
    """sgd_kernel on one buffer; returns (w', g'')"""
    w, g = np.asarray(w, F32), np.asarray(g, F32)
    wd, neg, momentum = F32(wd), F32(neg), F32(momentum)
    if wd != 0:
        g = (w * wd).astype(F32) + g
    w = (g * neg).astype(F32) + w
    if momentum == 0:
        g = np.zeros_like(g)
    elif momentum != 1:
        g = (g * momentum).astype(F32)
    return w.astype(F32), g.astype(F32).copy()


def sgd_update(w, b, dw, db, batch, lr, momentum, decay):
    """bcnn_hip_sgd_update: the biases with wd = 0, the weights with decay * batch; returns (w, b, dw, db)"""
    neg = neg_lr_b(lr, batch)
    b, db = sgd_step(b, db, F32(0), neg, momentum)
    w, dw = sgd_step(w, dw, wd_b(decay, batch), neg, momentum)
    return w, b, dw, db


def adam_weights(w, g, m, v, wd, one_m_b1, b1, one_m_b2, b2, step):
    """adam_kernel; returns (w', g'' = 0, m', v')"""
    w, g, m, v = (np.asarray(a, F32) for a in (w, g, m, v))
    wd, one_m_b1, b1, one_m_b2, b2, step = (F32(a) for a in (wd, one_m_b1, b1, one_m_b2, b2, step))
    g = (w * wd).astype(F32) + g                                   # the decay axpy, taken at wd == 0 as well
    m = (one_m_b1 * g).astype(F32) + (b1 * m).astype(F32)
    v = (one_m_b2 * (g * g).astype(F32)).astype(F32) + (b2 * v).astype(F32)
    q = m / (np.sqrt(v) + F32(0.0000001))
    w = (q * step).astype(F32) + w
    return w.astype(F32), np.zeros_like(g), m.astype(F32), v.astype(F32)


def adam_update(w, b, dw, db, m, v, batch, it, beta1, beta2, lr, momentum, decay):
    """bcnn_hip_adam_update; returns (w, b, dw, db, m, v)"""
    neg = neg_lr_b(lr, batch)
    step = neg * adam_mu(beta1, beta2, it)                          # -lr / batch_size * mu, left to right
    b, db = sgd_step(b, db, F32(0), neg, momentum)
    w, dw, m, v = adam_weights(w, dw, m, v, wd_b(decay, batch), F32(1) - F32(beta1), F32(beta1),
                               F32(1) - F32(beta2), F32(beta2), step)
    return w, b, dw, db, m, v


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
def zero_block(n):
    """the elements whose gradient, m and v are all zero (Adam's 0 / (0 + 1e-7)); empty below 4 elements"""
    return slice(n // 3, n // 3 + max(1, min(64, n // 4))) if n >= 4 else slice(0, 0)


@functools.lru_cache(maxsize=None)
def inputs(w_size, b_size, batch):
    """w0, b0, the fresh gradients of STEPS steps (scaled by the batch size, as a backward pass over a batch leaves them;
    oracle/ref_cases.make_optim) and Adam's starting moments. Read-only: shared between tests."""
    rs = np.random.RandomState(SEED + 7 * w_size + b_size + 1000003 * batch)
    u = lambda *shape: rs.uniform(-1, 1, shape).astype(F32)
    case = dict(w0=u(w_size), b0=u(b_size), dw=u(STEPS, w_size) * F32(batch), db=u(STEPS, b_size) * F32(batch),
                m0=u(w_size) * F32(batch), v0=(u(w_size) * F32(batch)) ** 2)
    zb = zero_block(w_size)
    case["dw"][:, zb] = 0
    case["m0"][zb] = 0
    case["v0"][zb] = 0
    for a in case.values():
        a.setflags(write=False)
    return case
