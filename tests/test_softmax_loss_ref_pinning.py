"""Pins tests/_softmax_loss_ref.py, the float64 restatement the GPU tests of the softmax-loss node compare with, to
torch's F.cross_entropy(ignore_index=..., reduction="sum" / "mean") and its autograd gradient in float64 (CPU).

torch knows two classes of label only: ignore_index and a class index (anything else is an error there), so the labels
the node calls "out of range" are mapped to ignore_index before torch sees them -- the restatement must then give them the
same zero contribution while counting them on their own."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _softmax_loss_ref as R

IGNORE = 255


def _torch(x, kind, cls, norm, scale, n):
    """loss and gradient by torch in float64; norm by the reduction that matches it"""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    target = torch.tensor(np.where(kind == R.VALID, cls, IGNORE).astype(np.int64))
    if norm == R.NORM_VALID and (kind == R.VALID).any():
        loss = F.cross_entropy(xt, target, ignore_index=IGNORE, reduction="mean")
    else:   # "mean" is 0 / 0 = NaN for V = 0, where the node says 0: the sum form covers it
        loss = F.cross_entropy(xt, target, ignore_index=IGNORE, reduction="sum") / R.denominator(norm, int((kind == R.VALID).sum()), n)
    (scale * loss).backward()
    return float(loss.detach()), xt.grad.numpy()


def _logits(n, C, HW, seed):
    return np.random.RandomState(seed).uniform(-4, 4, (n, C, HW)).astype(np.float32)


@pytest.mark.parametrize("norm", [R.NORM_NONE, R.NORM_VALID, R.NORM_VALID_PER_IMAGE])
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_restatement_matches_torch(norm, pattern):
    n, C, HW = 3, 5, 41
    x = _logits(n, C, HW, 11)
    lab, ignore = R.labels(pattern, n, C, HW, seed=5)
    ref = R.reference(x, lab, ignore, norm, scale=0.75)
    want_loss, want_dx = _torch(x, ref["kind"], ref["cls"], norm, float(np.float32(0.75)), n)
    assert ref["valid"] + ref["ignored"] + ref["out_of_range"] == n * HW
    if pattern == "all_ignored":
        assert ref["valid"] == 0 and ref["loss"] == 0.0 and not ref["dx"].any()   # V = 0: zeros, not NaN
    np.testing.assert_allclose(ref["loss"], want_loss, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(ref["dx"], want_dx, rtol=1e-12, atol=1e-16)
    np.testing.assert_allclose(ref["p"], F.softmax(torch.tensor(x, dtype=torch.float64), dim=1).numpy(), rtol=1e-13)
    assert np.array_equal(ref["arg"], torch.tensor(x).argmax(dim=1).numpy())
    assert ref["confusion"].trace() == ref["correct"] and ref["confusion"].sum() == ref["valid"]


def test_denominators():
    assert R.denominator("none", 12, 4) == 1.0 and R.denominator("none", 0, 4) == 1.0
    assert R.denominator("valid", 12, 4) == 12.0 and R.denominator("valid", 0, 4) == 1.0
    assert R.denominator("valid_per_image", 12, 4) == 3.0 and R.denominator("valid_per_image", 0, 4) == 0.25


def test_label_classes_on_their_boundaries():
    C = 5
    t = np.array([0, 4, 5, -1, 254, 255, 1.5, 4.000001, np.nan, np.inf, -np.inf, -0.0, 3e9, 2 ** 24], np.float32)
    kind, cls = R.classify(t, 255, C)
    V, I, O = R.VALID, R.IGNORED, R.OUT_OF_RANGE
    assert kind.tolist() == [V, V, O, O, O, I, O, O, O, O, O, V, O, O]
    assert cls.tolist() == [0, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, -1, -1]
    kind, cls = R.classify(t, -1, C)        # nothing is ignored on purpose: -1 and 255 are out of range
    assert kind.tolist() == [V, V, O, O, O, O, O, O, O, O, O, V, O, O]
    kind, cls = R.classify(t, 4, C)         # the ignore label wins over the range
    assert kind[1] == I and cls[1] == -1 and kind[0] == V
    kind, cls = R.classify(np.array([299, 300, 254], np.float32), 255, 300)   # more classes than the ignore label
    assert kind.tolist() == [V, O, V] and cls.tolist() == [299, -1, 254]


def test_first_maximum_wins_on_equal_logits():
    x = np.full((1, 4, 3), 0.7310585, np.float32)
    ref = R.reference(x, np.zeros((1, 3), np.float32), 255, R.NORM_VALID)
    assert ref["correct"] == 3 and ref["confusion"][0, 0] == 3
    np.testing.assert_allclose(ref["loss"], np.log(4.0), rtol=1e-12)
    ref = R.reference(x, np.ones((1, 3), np.float32), 255, R.NORM_VALID)
    assert ref["correct"] == 0 and ref["confusion"][1, 0] == 3
