"""Pins the numpy restatement of batch normalisation (tests/_bn_ref.py) on the CPU: on the six golden bn_* cases and three
seeded larger ones the float64 form agrees with the C oracle (oracle.orc_bind.orc_bn) and, where oracle/_ref is present, with
the unmodified reference (oracle.ref_cases.ref_bn), under the bars test_hip_parity.py holds the HIP kernels to. This is what
makes _bn_ref.py a statement of the reference and not of the HIP code. The float32 per-element chains are pinned bit for
bit on the same cases (the oracle divides and multiplies in the same order), and the input generator of the GPU tests is
checked here for the precondition that makes its sums exact."""
import numpy as np
import pytest

from oracle import orc_bind as ob
from oracle import ref_bind as rb
from oracle import ref_cases as rc
from tests import _bn_ref as B
from tests import _golden as G
from tests import _next_ref as R
from tests.test_hip_parity import REL_TOL, VAR_KEYS

F32, F64 = np.float32, np.float64
SEEDED = {"seeded_5x3x14x14": (5, 3, 14, 14), "seeded_2x2x33x31": (2, 2, 33, 31), "seeded_7x4x1x1": (7, 4, 1, 1)}
NAMES = G.names("bn_") + sorted(SEEDED)


def load(name):
    if name in SEEDED:
        n, c, h, w = SEEDED[name]
        return rc.make_bn(n * 100 + c * 10 + h, n, c, h, w, carry=True, shift=0.3, name=name)
    return G.load(name)[0]


def restated64(cs):
    n, c, h, w, mode = (int(cs[q]) for q in ("n", "c", "h", "w", "mode"))
    x = cs["x"].reshape(n, c, h * w)
    f = B.forward64(x, cs["run_mean0"], cs["run_var0"], cs["scales"], cs["bias"], mode)
    out = {k: f[k] for k in ("y", "run_mean", "run_var", "saved_mean", "saved_var") if k in f}
    if mode == B.MODE_TRAIN:
        z = np.zeros(c, F32)
        out.update(B.backward64(cs["dy"].reshape(n, c, h * w), x, cs["scales"], f["saved_mean"].astype(F32),
                                f["saved_var"].astype(F32), cs.get("dscales0", z), cs.get("db0", z)))
        if n * h * w == 1:
            # one sample per channel: x = mean and dmean = -(g scale / sqrt(var + 1e-5)), so the three terms of the input
            # gradient cancel to exactly 0 and what the reference leaves there is its own rounding noise (1e-7 of a term).
            # No bar relative to the result can be held against 0; test_float32_chains_... pins these two keys bit for bit.
            del out["dy_out"], out["dx"]
    return out


def check(tag, got, want):
    for key, have in got.items():
        if key not in want:
            assert key in ("dy_out", "dx") and have.size == have.shape[1], (tag, key)      # see restated64
            continue
        ref = np.asarray(want[key], F64).reshape(have.shape)
        if key in VAR_KEYS:
            assert np.allclose(have, ref, rtol=1e-4, atol=1e-6), (tag, key, np.abs(have - ref).max())
        else:
            G.assert_close("%s/%s" % (tag, key), have, ref, REL_TOL, rtol=REL_TOL, afrac=REL_TOL / 10)


@pytest.mark.parametrize("name", NAMES)
def test_float64_form_agrees_with_the_oracle_and_the_reference(name):
    assert len(G.names("bn_")) == 6
    cs = load(name)
    want = restated64(cs)
    check("orc/" + name, ob.orc_bn(cs), want)
    if name not in SEEDED:
        check("golden/" + name, {k: v for k, v in G.load(name)[1].items() if k != "dy"}, want)
    if rb.available():
        check("ref/" + name, rc.ref_bn(cs), want)


@pytest.mark.parametrize("name", NAMES)
def test_float32_chains_reproduce_the_oracle_bit_for_bit(name):
    """given the oracle's own statistics, every per-element step of the float32 form is the oracle's operation"""
    cs = load(name)
    n, c, h, w, mode = (int(cs[q]) for q in ("n", "c", "h", "w", "mode"))
    x = cs["x"].reshape(n, c, h * w)
    orc = ob.orc_bn(cs)
    if mode == B.MODE_PREDICT:
        R.assert_bits(name + "/y", orc["y"], B.predict32(x, cs["scales"], cs["bias"]))
        return
    mean, var = (orc["saved_mean"], orc["saved_var"]) if mode == B.MODE_TRAIN else (cs["run_mean0"], cs["run_var0"])
    assert np.array_equal(orc["y"].ravel(), B.affine32(B.normalize32(x, mean, var), cs["scales"], cs["bias"]).ravel())
    if mode == B.MODE_TRAIN:
        dx = B.bwd_apply32(cs["dy"].reshape(x.shape), x, mean, var, cs["scales"], orc["dmean"], orc["dvar"], n * h * w)
        assert np.array_equal(orc["dy_out"].ravel(), dx.ravel())
        assert np.array_equal(orc["dx"].ravel(), dx.ravel())


def test_finalize_forms_agree_with_the_float64_form():
    """the float32 finalize chains (written as the kernels write them) against the float64 statement, on inputs whose sums
    are exact: the only differences are the roundings of the chain itself"""
    p = B.exact_inputs(7, 5, 196)
    f = B.forward64(p.x, p.run_mean0, p.run_var0, p.scales, p.bias, B.MODE_TRAIN)
    mean, var, run_mean, run_var = B.stats_finalize32(p.S, p.SS, p.M, p.run_mean0, p.run_var0)
    check("finalize32", {"saved_mean": mean, "saved_var": var, "run_mean": run_mean, "run_var": run_var}, f)
    b = B.backward64(p.dy, p.x, p.scales, p.mean, p.var, p.dscales0, p.dbias0)
    db, dsc, dmean, dvar = B.bwd_finalize32(p.S1, p.S2, p.scales, p.var, p.dscales0, p.dbias0)
    check("bwd_finalize32", {"db": db, "dscales": dsc, "dmean": dmean}, b)
    live = np.arange(p.c) != p.const      # var = 0: -0.5 / (0 + 1e-5f) amplifies; S2 = 0 there on both sides
    check("bwd_finalize32", {"dvar": dvar[live]}, {"dvar": b["dvar"][live]})
    assert dvar[p.const] == 0 and b["dvar"][p.const] == 0


def test_exact_inputs_hold_their_precondition_for_every_gpu_shape():
    """exact_inputs() asserts sum x^2 < 2^24 and GRAIN * sum |g (x - mean)| < 2^24 per channel itself; here every shape the
    GPU tests draw is generated once on the CPU, so a case that breaks the precondition fails without a GPU"""
    from tests import test_batchnorm_edges as E
    for args in E.all_exact_cases():
        p = B.exact_inputs(*args)
        assert p.x.shape == (p.n, p.c, p.hw) and np.all(np.abs(p.x) <= 4)
        assert np.all(np.abs(p.S) < 2 ** 24) and np.all(p.SS < 2 ** 24)
        assert np.all(np.abs(p.S2) * B.GRAIN < 2 ** 24)
        assert np.array_equal(p.mean * 4, np.round(p.mean * 4))
