"""tests/_optim_ref.py against the C restatement of the reference (oracle/bcnn_oracle.c: orc_sgd_update, orc_adam_update)
on the CPU, on the inputs test_optim_steps.py runs on the device, at the sizes below one sweep. No GPU.

The SGD step, and Adam's m, v and dw, are chains of single float32 operations on both sides: bits. Adam's w is not: the
reference takes powf(v, 0.5f) for the root (bcnn_pow), the HIP kernel and the restatement the correctly rounded sqrt."""
import numpy as np
import pytest

from oracle import orc_bind as ob
from tests import _next_ref as R
from tests import _optim_ref as O
from tests.test_hip_parity import REL_TOL

F32 = np.float32

# Largest distance, in float32 ulps of the restatement's w, between the restatement (sqrt) and the oracle (powf(v, 0.5f))
# over every Adam case below -- measured on the CPU with the inputs of _optim_ref.inputs (SEED = 20240611).
ADAM_W_ULPS = 0


def ulps(got, want):
    """|got - want| in units of the spacing of float32 at |want|"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize("batch", O.BATCHES)
@pytest.mark.parametrize("momentum,decay", O.SGD_HYPER)
@pytest.mark.parametrize("w_size,b_size", O.SMALL)
def test_sgd_restatement_is_the_oracle_in_bits(w_size, b_size, momentum, decay, batch):
    L = ob.lib()
    cs = O.inputs(w_size, b_size, batch)
    w, b = cs["w0"].copy(), cs["b0"].copy()
    dw, db = np.zeros_like(w), np.zeros_like(b)
    ow, obias, odw, odb = w.copy(), b.copy(), dw.copy(), db.copy()
    for t in range(O.STEPS):
        dw, db = dw + cs["dw"][t], db + cs["db"][t]
        odw += cs["dw"][t]
        odb += cs["db"][t]
        w, b, dw, db = O.sgd_update(w, b, dw, db, batch, O.LR, momentum, decay)
        L.orc_sgd_update(ob.P(ow), ob.P(obias), ob.P(odw), ob.P(odb), w_size, b_size, batch, O.LR, momentum, decay)
        for name, got, want in (("w", w, ow), ("b", b, obias), ("dw", dw, odw), ("db", db, odb)):
            R.assert_bits("sgd step %d %s" % (t, name), got, want)


def _adam_runs(w_size, b_size, beta1, beta2, iters, decay):
    """every step of one Adam case on both sides: yields (step, restatement tuple, oracle tuple)"""
    L = ob.lib()
    cs = O.inputs(w_size, b_size, O.ADAM_BATCH)
    st = [cs["w0"].copy(), cs["b0"].copy(), np.zeros(w_size, F32), np.zeros(b_size, F32), cs["m0"].copy(), cs["v0"].copy()]
    orc = [a.copy() for a in st]
    for t, it in enumerate(iters):
        st[2], st[3] = st[2] + cs["dw"][t], st[3] + cs["db"][t]
        orc[2] += cs["dw"][t]
        orc[3] += cs["db"][t]
        st = list(O.adam_update(*st, O.ADAM_BATCH, it, beta1, beta2, O.LR, O.ADAM_MOMENTUM, decay))
        L.orc_adam_update(ob.P(orc[0]), ob.P(orc[1]), ob.P(orc[2]), ob.P(orc[3]), ob.P(orc[4]), ob.P(orc[5]), w_size,
                          b_size, O.ADAM_BATCH, it, beta1, beta2, O.LR, O.ADAM_MOMENTUM, decay)
        yield t, st, orc
        orc[0][:] = st[0]      # the next step starts from the same weights on both sides: the bound is per step


@pytest.mark.parametrize("decay", O.ADAM_DECAYS)
@pytest.mark.parametrize("beta1,beta2,iters", O.ADAM_HYPER)
@pytest.mark.parametrize("w_size,b_size", O.SMALL)
def test_adam_restatement_against_the_oracle(w_size, b_size, beta1, beta2, iters, decay):
    """m, v, dw, b, db: bits. w: within ADAM_W_ULPS float32 ulps, which must not exceed the REL_TOL the optim_* goldens
    are held to. Measured over all 32 cases (w_size 1 / 255 / 256 / 257, input seed _optim_ref.SEED = 20240611): 0 ulp at
    every step -- this libm's powf(v, 0.5f) returns the correctly rounded root on these values -- so w is held to bits."""
    assert ADAM_W_ULPS * 2.0 ** -23 <= REL_TOL
    for t, st, orc in _adam_runs(w_size, b_size, beta1, beta2, iters, decay):
        for k, name in ((1, "b"), (2, "dw"), (3, "db"), (4, "m"), (5, "v")):
            R.assert_bits("adam step %d %s" % (t, name), st[k], orc[k])
        assert not np.any(R.bits(st[2])), "dw is +0 after the step"
        worst = float(ulps(orc[0], st[0]).max())
        print("adam w%d decay %g (%g, %g) step %d: w differs by at most %.3g ulp" % (w_size, decay, beta1, beta2, t, worst))
        if ADAM_W_ULPS == 0:
            R.assert_bits("adam step %d w" % t, st[0], orc[0])
        else:
            assert worst <= ADAM_W_ULPS, worst
