"""The softmax cross-entropy loss over class-index label maps (bcnn_amd/csrc/softmax_loss.hip), restated in float64
numpy: label classification, probabilities, loss, gradient, counts and the confusion matrix. Pinned to torch's
F.cross_entropy by tests/test_softmax_loss_ref_pinning.py; the GPU tests compare the kernels with this file.

Shapes: x (n, C, HW) float32 logits, label (n, HW) float32 class indices."""
import numpy as np

F32, F64 = np.float32, np.float64
VALID, IGNORED, OUT_OF_RANGE = 0, 1, 2
NORM_NONE, NORM_VALID, NORM_VALID_PER_IMAGE = 0, 1, 2
NORMS = {"none": NORM_NONE, "valid": NORM_VALID, "valid_per_image": NORM_VALID_PER_IMAGE}


def classify(label, ignore_label, C):
    """(kind, cls): kind VALID / IGNORED / OUT_OF_RANGE per label value, cls the class index where VALID and -1 elsewhere.
    The ignore label wins over the range; ignore_label < 0 ignores nothing on purpose."""
    t = np.asarray(label, F32)
    with np.errstate(invalid="ignore"):
        ignored = (t == F32(ignore_label)) if ignore_label >= 0 else np.zeros(t.shape, bool)
        inside = (t >= 0) & (t < C) & (np.floor(t) == t)
    valid = inside & ~ignored
    kind = np.where(ignored, IGNORED, np.where(valid, VALID, OUT_OF_RANGE))
    cls = np.where(valid, np.where(valid, t, 0).astype(np.int64), -1)
    return kind, cls


def denominator(norm, V, n):
    norm = NORMS.get(norm, norm)
    v = float(max(V, 1))
    return {NORM_NONE: 1.0, NORM_VALID: v, NORM_VALID_PER_IMAGE: v / n}[norm]


def reference(x, label, ignore_label=-1, norm=NORM_VALID_PER_IMAGE, scale=1.0):
    """everything the node computes, in float64 on the float32 inputs. Returns a dict:
    p (n, C, HW), lse (n, HW), loss, D, dx (n, C, HW), kind, cls, valid, ignored, out_of_range, correct, confusion (C, C)"""
    x64 = np.asarray(x, F32).astype(F64)
    n, C, HW = x64.shape
    kind, cls = classify(np.asarray(label, F32).reshape(n, HW), ignore_label, C)
    m = x64.max(axis=1, keepdims=True)
    e = np.exp(x64 - m)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    lse = (m + np.log(s))[:, 0, :]
    valid = kind == VALID
    safe = np.where(valid, cls, 0)
    xt = np.take_along_axis(x64, safe[:, None, :], axis=1)[:, 0, :]
    per_pixel = np.where(valid, lse - xt, 0.0)
    V = int(valid.sum())
    D = denominator(norm, V, n)
    onehot = np.zeros_like(x64)
    np.put_along_axis(onehot, safe[:, None, :], 1.0, axis=1)
    dx = np.where(valid[:, None, :], float(F32(scale)) / D * (p - onehot), 0.0)
    arg = np.asarray(x, F32).argmax(axis=1)   # the first maximum, like torch's argmax
    confusion = np.zeros((C, C), np.int64)
    np.add.at(confusion, (cls[valid], arg[valid]), 1)
    return dict(p=p, lse=lse, loss=float(per_pixel.sum() / D), D=D, dx=dx, kind=kind, cls=cls, valid=V,
                ignored=int((kind == IGNORED).sum()), out_of_range=int((kind == OUT_OF_RANGE).sum()),
                correct=int((arg[valid] == cls[valid]).sum()), confusion=confusion, onehot=onehot, arg=arg)


# ---- label patterns of the operator test ------------------------------------------------------------------------------------
PATTERNS = ["all_valid", "all_ignored", "ignore_runs", "one_class", "out_of_range", "minus_one_no_ignore"]


def labels(pattern, n, C, HW, seed, x=None):
    """(label (n, HW) float32, ignore_label). Where x is given, the rows of tests/_next_ref.softmax_inputs whose logits are
    all equal get label 0 wherever the pattern leaves them valid: the first maximum wins, so they must count as correct."""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, C, (n, HW)).astype(F32)
    ignore = 255
    flat = lab.reshape(-1)
    if pattern == "all_ignored":
        flat[:] = ignore
    elif pattern == "ignore_runs":
        # runs of 37 ignored pixels every 101: they straddle the 64-pixel wave, the 256-pixel (and 1024-pixel, in the
        # 16-byte form) workgroup boundaries at varying phases
        idx = np.arange(flat.size)
        flat[(idx % 101) < 37] = ignore
        flat[max(0, min(flat.size, 256) - 3):min(flat.size, 256 + 3)] = ignore
    elif pattern == "one_class":
        flat[:] = C - 1
    elif pattern == "out_of_range":
        if C > ignore - 1:   # ignore_label - 1 would be a class then
            ignore = C + 7
        bad = [F32(C), F32(-1), F32(ignore - 1), F32(1.5), F32(np.inf), F32(np.nan), F32(-np.inf), F32(3e9)]
        for k in range(0, flat.size, 3):
            flat[k] = bad[(k // 3) % len(bad)]
        flat[1::7] = ignore
    elif pattern == "minus_one_no_ignore":
        ignore = -1
        flat[::4] = -1
    if x is not None:
        equal = np.all(np.asarray(x) == np.asarray(x)[:, :1, :], axis=1)   # (n, HW)
        kind, _ = classify(lab, ignore, C)
        lab[equal & (kind == VALID)] = 0
    return lab, ignore
