"""The dice-loss kernels (bcnn_amd/csrc/dice_loss.hip) at operator level against `reference`, one float64 numpy function
on the same float32 inputs. Logits in [-6, 6]; labels are classes with the ignore value, -1, C, 2.5 and NaN sprinkled in.

Bounds, u = 2^-24, L the longest float32 chain of one lane's sums (four pixels per lane and tile
in the 16-byte form, one otherwise; plus 6 xor steps, 3 wave additions, 1 for second-order terms):
    p     bit for bit the softmax-loss node's p; e_p = (C + 3) u on the register and rows branches, (3 C + 4) u streaming
    I     |I - I64| <= (e_p + (L + 10) u) I64 =: r_I I64;   Z  <= ((2 | 1) e_p + (L + 11) u) Z64 =: r_Z Z64;  Y, counts exact
    loss  |ce_weight| ((k C + 16 + ln C) u + u |CE|) + |dice_weight| (max (r_I + r_Z) + u) + u |loss|, k = 1 or 3 as e_p:
          per pixel logf, the rounded sum and x_t - max; a Dice term moves by at most r_I + r_Z as (2 I + s) / Den <= 1
    dx    |dx - dx64| <= |dice_weight| 2 Gamma (r_I + 2 r_Z + 3 e_p + (C + 10) u) + g (e_p + 3 u) + 2 u max |dx64| with
          Gamma = max (|A| + 2 |B|), g = |ce_weight| / max(V, 1); measured: at most 0.03 of it, as a fraction of max |dx64|
          at most 6.6e-7 (I 0.18, Z 0.23, the loss 0.04 of theirs). Pixels that are not valid: +0.0 (overwrite) or the
          start bits (add); the add form on valid pixels is fl(dx0 + the overwrite form's value), bit for bit.
A second run gives the same bits of the workspace and of dx."""
import ctypes
import functools

import numpy as np
import pytest
import torch

DEV, BAND, U, IGNORE = "cuda:0", 64, 2.0 ** -24, 255
F64 = np.float64


def reference(x, lab, ignore, cw, dw, smooth, squared, reduce):
    n, C, HW = x.shape
    x64 = x.astype(F64)
    m = x64.max(1, keepdims=True)
    e = np.exp(x64 - m)
    s = e.sum(1, keepdims=True)
    p = e / s
    with np.errstate(invalid="ignore"):
        ign = (lab == np.float32(ignore)) if ignore >= 0 else np.zeros(lab.shape, bool)
        inr = (lab >= 0) & (lab < C) & (lab == np.floor(lab))
    valid, oor = inr & ~ign, ~inr & ~ign
    cls = np.where(valid, lab, 0).astype(np.int64)
    onehot = ((np.arange(C)[None, :, None] == cls[:, None, :]) & valid[:, None, :]).astype(F64)
    V = max(int(valid.sum()), 1)
    l = np.log(s[:, 0]) + m[:, 0] - np.take_along_axis(x64, cls[:, None, :], 1)[:, 0]
    ce = float(l[valid].sum()) / V
    pv = p * valid[:, None, :]
    z = pv * p if squared else pv
    axes = (0, 2) if reduce == "batch" else (2,)
    I, Z, Y = ((a.sum(axes)).reshape(-1, C) for a in (p * onehot, z, onehot))
    G = I.shape[0]
    den, num = Z + Y + smooth, 2 * I + smooth
    ok = den > 0
    sden = np.where(ok, den, 1.0)
    dice = float(np.where(ok, 1 - num / sden, 0.0).sum()) / (G * C)
    A, B = np.where(ok, -2 / (G * C * sden), 0.0), np.where(ok, num / (G * C * sden ** 2), 0.0)
    gamma = A[:, :, None] * onehot + B[:, :, None] * (2 * p if squared else 1.0)
    dx = (dw * p * (gamma - (gamma * p).sum(1, keepdims=True)) + cw / V * (p - onehot)) * valid[:, None, :]
    correct = int(((x.argmax(1) == cls) & valid).sum())
    return dict(p=p, izy=np.stack([I, Z, Y], -1), ce=ce, dice=dice, loss=cw * ce + dw * dice, dx=dx, valid3=np.broadcast_to(
        valid[:, None, :], x.shape), A=A, B=B, counts=(int(valid.sum()), int(ign.sum()), int(oor.sum()), correct))


def test_reference_on_hand_values():
    """two pixels, two classes, p = (1/2, 1/2) at both; labels 0 and ignore: I = Z_plain = 1/2, Y = (1, 0)"""
    r = reference(np.zeros((1, 2, 2), np.float32), np.array([[0, IGNORE]], np.float32), IGNORE, 1.0, 1.0, 0.0, False, "batch")
    assert np.allclose(r["izy"][0], [[0.5, 0.5, 1], [0, 0.5, 0]]) and abs(r["ce"] - np.log(2)) < 1e-15
    assert abs(r["dice"] - 0.5 * ((1 - 1 / 1.5) + 1)) < 1e-15 and r["counts"] == (1, 1, 0, 1) and not r["dx"][0, :, 1].any()


def _labels(rs, n, C, HW, pattern):
    lab = rs.randint(0, C, (n, HW)).astype(np.float32)
    if pattern == "all_ignored":
        lab[...] = IGNORE
    elif pattern == "absent_class" and C > 1:
        lab[lab == C - 1] = 0
    else:
        special = rs.rand(n, HW) < 0.15
        lab[special] = rs.choice(np.array([IGNORE, -1, C, 2.5, np.nan], np.float32), int(special.sum()))
    return lab


@functools.lru_cache(maxsize=None)
def _case(n, C, HW, reduce, squared, pattern):
    rs = np.random.RandomState(1000 * C + HW + n)
    x = rs.uniform(-6, 6, (n, C, HW)).astype(np.float32)
    lab = _labels(rs, n, C, HW, pattern)
    dx0 = rs.uniform(-1, 1, x.shape).astype(np.float32)
    cw, dw, smooth = (0.4, 0.6, 1e-5) if squared else (0.5, 0.5, 1.0)
    return x, lab, dx0, (cw, dw, smooth), reference(x, lab, IGNORE, float(np.float32(cw)), float(np.float32(dw)),
                                                    float(np.float32(smooth)), squared, reduce)


def _guarded(shape, off, values=None):
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * BAND + off,), 7.0, dtype=torch.float32, device=DEV)
    t = buf[BAND + off:BAND + off + numel].view(shape)
    if values is not None:
        t.copy_(torch.tensor(values))
    return buf, t


def _trace(on):
    from bcnn_amd import _lib
    L = _lib.load()
    if on:
        return L.bcnn_hip_trace_enable(1)
    n = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return buf.value.decode().split()


def _run(x, lab, dx0, weights, reduce, squared, off):
    from bcnn_amd import ops
    n, C, HW = x.shape
    cw, dw, smooth = weights
    kw = dict(ignore_label=IGNORE, dice_weight=dw, squared=squared, reduce=reduce)
    bufs = [_guarded(x.shape, off, x), _guarded((n, 1, HW), off, lab.reshape(n, 1, HW)), _guarded(x.shape, off), _guarded(x.shape, off),
            _guarded(x.shape, off, dx0), _guarded(x.shape, off)]
    xd, ld, pd, over, add, psl = (t for _, t in bufs)
    ws = ops.dice_loss_workspace(n, C, HW, reduce)
    _trace(True)
    ops.dice_loss_forward(xd, ld, pd, ws, ce_weight=cw, smooth=smooth, **kw)
    ops.dice_loss_backward(pd, ld, ws, over, overwrite=True, **kw)
    ops.dice_loss_backward(pd, ld, ws, add, overwrite=False, **kw)
    names = _trace(False)
    ops.softmax_loss_forward(xd, None, psl, None)
    torch.cuda.synchronize()
    wide = ops.dice_loss_path(n, C, HW, off == 0) == 1
    assert names == ["dice_loss_fwd"] + ["dice_loss_sums"] * wide + ["dice_loss_finalize", "dice_loss_bwd", "dice_loss_bwd"], names
    for buf, t in bufs:
        edge = torch.cat([buf[:BAND + off], buf[BAND + off + t.numel():]])
        assert bool((edge == 7.0).all()), "a write outside its tensor"
    rec, sums, coef = ops.dice_loss_read_workspace(ws, n, C, reduce)
    return dict(p=pd.cpu().numpy(), psl=psl.cpu().numpy(), over=over.cpu().numpy(), add=add.cpu().numpy(), rec=rec, sums=sums,
                coef=coef, ws_bits=ws.cpu().numpy().view(np.int64).copy(), wide=wide)


def _chain(n, C, HW, vec, wide):
    """the float32 additions behind one lane's sum: dl_split of dice_loss.hip restated"""
    qn = HW // 4 if vec else HW
    per_image = (C + 7) // 8 if wide else 1
    parts = min((qn + 255) // 256, max(1, 2048 // (n * per_image)))
    return (4 if vec else 1) * -(-qn // (parts * 256))


BITS = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)
SMALL = [(C, HW) for C in (1, 2, 31, 32, 33, 70) for HW in (1, 3, 4, 5, 255, 257, 1020, 1028)]
# n, reduce and squared cycle at different periods along hw and shift with C, so every pairing occurs on both paths
CASES = [((1, 3)[(k + k // 8) % 2], C, HW, ("batch", "image")[(k % 8 // 2 + k // 8) % 2], bool((k % 8 // 4 + k // 16 + k) % 2), "mixed", 0)
         for k, (C, HW) in enumerate(SMALL)]
CASES += [(3, 2, 1020, "image", True, "mixed", 1), (3, 33, 1028, "image", True, "mixed", 1), (3, 32, 4, "batch", False, "mixed", 1),
          (3, 5, 257, "image", True, "all_ignored", 0), (2, 70, 64, "batch", True, "all_ignored", 0),
          (3, 6, 1028, "image", True, "absent_class", 0), (2, 40, 255, "batch", False, "absent_class", 0),
          # a persistent workgroup takes more than one tile: past 682 x 256 lanes per image (n = 3), 16-byte and scalar form,
          # and past 136 x 256 in the class-major sums launch (C = 33: five chunks)
          (3, 2, 700000, "image", True, "mixed", 0), (3, 2, 180001, "batch", False, "mixed", 0), (3, 33, 36001, "image", True, "mixed", 0),
          # the same for the 8-, 16-, 24- and 32-class register instances: n = 64 leaves 32 workgroups per image, 8301 pixels
          # are 33 tiles of the scalar form
          (64, 8, 8301, "image", True, "mixed", 0), (64, 16, 8301, "batch", False, "mixed", 0),
          (64, 24, 8301, "batch", True, "mixed", 0), (64, 32, 8301, "image", True, "mixed", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,C,HW,reduce,squared,pattern,off", CASES, ids=lambda v: str(v))
def test_dice_loss_against_float64(n, C, HW, reduce, squared, pattern, off):
    x, lab, dx0, weights, ref = _case(n, C, HW, reduce, squared, pattern)
    cw, dw, smooth = (float(np.float32(w)) for w in weights)
    got = _run(x, lab, dx0, weights, reduce, squared, off)
    vec = HW > 1 and HW % 4 == 0 and off == 0
    assert np.array_equal(BITS(got["p"]), BITS(got["psl"])), "p has the softmax-loss node's bits"
    rec = got["rec"]
    assert (rec["valid"], rec["ignored"], rec["out_of_range"], rec["correct"]) == ref["counts"]
    I, Z, Y = (ref["izy"][..., k] for k in range(3))
    assert np.array_equal(got["sums"][..., 2], Y), "Y is exact"
    k = 3 if got["wide"] and HW > 1 else 1
    e_p = (k * C + 3 + (k == 3)) * U
    L = _chain(n, C, HW, vec, got["wide"])
    r_I, r_Z = e_p + (L + 10) * U, (2 if squared else 1) * e_p + (L + 11) * U
    f_I = float((np.abs(got["sums"][..., 0] - I) / np.maximum(r_I * I, 1e-300)).max())
    f_Z = float((np.abs(got["sums"][..., 1] - Z) / np.maximum(r_Z * Z, 1e-300)).max())
    loss_bound = abs(cw) * ((k * C + 16 + np.log(C)) * U + U * abs(ref["ce"])) + abs(dw) * (r_I + r_Z + U) + U * abs(ref["loss"])
    f_loss = abs(rec["loss"] - ref["loss"]) / loss_bound
    V = max(ref["counts"][0], 1)
    gamma = float((np.abs(ref["A"]) + 2 * np.abs(ref["B"])).max())
    top = float(np.abs(ref["dx"]).max())
    tol = abs(dw) * 2 * gamma * (r_I + 2 * r_Z + 3 * e_p + (C + 10) * U) + abs(cw) / V * (e_p + 3 * U) + 2 * U * top
    v3 = ref["valid3"]
    err = float(np.abs(got["over"] - ref["dx"])[v3].max()) if v3.any() else 0.0
    print("n%d c%d hw%d %s sq%d %s off%d: I %.3f Z %.3f loss %.3f dx %.3f of the bounds, dx err / max|dx| %.2e, L %d" % (
        n, C, HW, reduce, squared, pattern, off, f_I, f_Z, f_loss, err / tol, err / top if top else 0.0, L))
    assert f_I <= 1 and f_Z <= 1, (f_I, f_Z)
    assert np.isfinite(rec["loss"]) and f_loss <= 1, (rec, ref["loss"], ref["ce"], ref["dice"])
    assert abs(rec["ce"] - ref["ce"]) <= loss_bound and abs(rec["dice"] - ref["dice"]) <= loss_bound
    assert err <= tol, (err, tol)
    assert bool((BITS(got["over"])[~v3] == 0).all()), "+0.0 where the pixel is not valid"
    assert np.array_equal(BITS(got["add"])[~v3], BITS(dx0)[~v3]), "the add form leaves those bits"
    assert np.array_equal(BITS(got["add"])[v3], BITS(dx0 + got["over"])[v3]), "the add form adds the same value"
    if pattern == "all_ignored":
        assert rec["valid"] == 0 and rec["ce"] == 0.0 and not got["over"].any()
    if pattern == "absent_class":
        assert Y[:, C - 1].max() == 0 and rec["valid"] > 0
    again = _run(x, lab, dx0, weights, reduce, squared, off)
    for name in ("ws_bits", "over", "add"):
        assert np.array_equal(got[name].view(np.int32), again[name].view(np.int32)), name
