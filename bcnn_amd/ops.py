"""Host-side mirror of the reference's per-layer workers on torch device tensors.

Each function takes/returns torch CUDA(=HIP) float32/int32 tensors and forwards to the C-ABI in
lib/libbcnn_hip.so with raw device pointers; argument meaning follows the reference layer code
(file:line cited per function). torch is plumbing only (device memory + streams); no torch op computes
anything on this path, and a missing extension raises (bcnn_amd/_lib.py).
"""
import ctypes as _C

import torch

from . import _lib

ACT = dict(none=0, tanh=1, relu=2, ramp=3, softplus=4, lrelu=5, abs=6, clamp=7, prelu=8, logistic=9)
# The appended activations (no reference counterpart), and every name. ACT itself stays the reference's ten: tests iterate
# over it as "every activation the reference has". relu6 / hard_sigmoid go wherever an `act` argument is taken; hard_swish,
# swish and mish through activation_forward[_keep] / activation_backward_from_input only.
ACT_APPENDED = dict(relu6=10, hard_sigmoid=11, hard_swish=12, swish=13, mish=14)
ACT_ALL = dict(ACT, **ACT_APPENDED)
MODE_PREDICT, MODE_TRAIN, MODE_VALID = 0, 1, 2


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device, contiguous tensors only"
    return t.data_ptr()


def _f32(t):
    assert t is None or t.dtype == torch.float32
    return _p(t)


def conv_out_hw(h, w, k, s, p):
    """bcnn_conv_layer.c:126-134"""
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def conv_workspace_size(n, c, h, w, f, k, s, p, g):
    return int(_lib.load().bcnn_hip_conv_workspace_size(n, c, h, w, f, k, s, p, g))


def conv_forward(x, wt, bias, y, k, stride, pad, groups=1, act=0, slopes=None, bn=None, mode=MODE_TRAIN):
    """bcnn_forward_conv_layer (bcnn_conv_layer.c:367-485). bn: dict(run_mean, run_var, scales,
    saved_mean, saved_var, x_norm (optional), workspace) for a fused batch-norm node, else None."""
    n, c, h, w = x.shape
    f = wt.shape[0]
    L = _lib.load()
    b = bn or {}
    L.bcnn_hip_conv_forward(_f32(x), _f32(wt), _f32(bias), _f32(y), n, c, h, w, f, k, stride, pad, groups,
                            act, _f32(slopes), 1 if bn else 0, _f32(b.get("run_mean")), _f32(b.get("run_var")),
                            _f32(b.get("scales")), _f32(b.get("saved_mean")), _f32(b.get("saved_var")),
                            _f32(b.get("x_norm")), _f32(b.get("workspace")), mode)


def conv_forward_bf16(x, wt, bias, y, k, stride, pad, groups=1, act=0, slopes=None, bn=None, mode=MODE_PREDICT):
    """conv_forward for inference with the convolution on the bf16 matrix cores (bcnn_hip_conv_forward_bf16): fp32
    tensors, operands rounded to bf16 inside the kernel, fp32 accumulator, the fp32 path's bias / batch-norm / activation.
    mode is MODE_PREDICT or MODE_VALID; returns False, and launches and writes nothing, for MODE_TRAIN."""
    n, c, h, w = x.shape
    f = wt.shape[0]
    b = bn or {}
    return bool(_lib.load().bcnn_hip_conv_forward_bf16(
        _f32(x), _f32(wt), _f32(bias), _f32(y), n, c, h, w, f, k, stride, pad, groups, act, _f32(slopes), 1 if bn else 0,
        _f32(b.get("run_mean")), _f32(b.get("run_var")), _f32(b.get("scales")), _f32(b.get("saved_mean")),
        _f32(b.get("saved_var")), _f32(b.get("x_norm")), _f32(b.get("workspace")), mode))


def conv_backward(x, wt, y, dy, dx, dw, dbias, k, stride, pad, groups, act, workspace, slopes=None,
                  dslopes=None, bn=None, bias=None):
    """bcnn_backward_conv_layer (bcnn_conv_layer.c:487-587). dy is updated in place; dx may be None.
    bias (optional): the forward bias; lets the fused batch-norm backward recompute y instead of reading it."""
    n, c, h, w = x.shape
    f = wt.shape[0]
    L = _lib.load()
    b = bn or {}
    L.bcnn_hip_conv_backward(_f32(x), _f32(wt), _f32(bias), _f32(y), _f32(dy), _f32(dx), _f32(dw), _f32(dbias), n, c, h, w,
                             f, k, stride, pad, groups, act, _f32(slopes), _f32(dslopes), 1 if bn else 0,
                             _f32(b.get("scales")), _f32(b.get("dscales")), _f32(b.get("saved_mean")),
                             _f32(b.get("saved_var")), _f32(b.get("dmean")), _f32(b.get("dvar")),
                             _f32(b.get("x_norm")), _f32(b.get("workspace")), _f32(workspace),
                             workspace.numel() if workspace is not None else 0)


def deconv_out_hw(h, w, k, s, p):
    """bcnn_deconv_layer.c:96-101"""
    return s * (h - 1) + k - 2 * p, s * (w - 1) + k - 2 * p


def deconv_workspace_size(n, c, h, w, f, k, s, p):
    return int(_lib.load().bcnn_hip_deconv_workspace_size(n, c, h, w, f, k, s, p))


def deconv_forward(x, wt, bias, y, k, stride, pad, act=0):
    """bcnn_forward_deconv_layer (bcnn_deconv_layer.c:150-193). wt: [c_in][f][k][k] (any shape of that size), y is
    overwritten with act(transposed convolution + bias)."""
    n, c, h, w = x.shape
    f = y.shape[1]
    assert wt.numel() == c * f * k * k
    _lib.load().bcnn_hip_deconv_forward(_f32(x), _f32(wt), _f32(bias), _f32(y), n, c, h, w, f, k, stride, pad, act)


def deconv_backward(x, wt, y, dy, dx, dw, dbias, k, stride, pad, act, workspace):
    """bcnn_backward_deconv_layer (bcnn_deconv_layer.c:195-246). dy is updated in place (dy * act'(y)), dbias and
    dw accumulate (dw += (1/n) x dyᵀ), dx (may be None) is overwritten."""
    n, c, h, w = x.shape
    f = y.shape[1]
    assert wt.numel() == c * f * k * k
    _lib.load().bcnn_hip_deconv_backward(_f32(x), _f32(wt), _f32(y), _f32(dy), _f32(dx), _f32(dw), _f32(dbias), n, c,
                                         h, w, f, k, stride, pad, act, _f32(workspace),
                                         workspace.numel() if workspace is not None else 0)


def dilated_conv_out_hw(h, w, k, s, p, d):
    """extent of a k x k kernel with taps d apart: torch.nn.functional.conv2d(dilation=d)"""
    return (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1


def dilated_conv_workspace_size(n, c, h, w, f, k, s, p, d, g=1):
    return int(_lib.load().bcnn_hip_dilated_conv_workspace_size(n, c, h, w, f, k, s, p, d, g))


def dilated_conv_forward(x, wt, bias, y, k, stride, pad, dilation, groups=1, act=0):
    """bcnn_hip_dilated_conv_forward (conv_dilated.hip). wt: [f][c / groups][k][k] (any shape of that size), y is
    overwritten with act(dilated convolution + bias)."""
    n, c, h, w = x.shape
    f = y.shape[1]
    assert wt.numel() == f * (c // groups) * k * k
    _lib.load().bcnn_hip_dilated_conv_forward(_f32(x), _f32(wt), _f32(bias), _f32(y), n, c, h, w, f, k, stride, pad,
                                              dilation, groups, act)


def dilated_conv_backward(x, wt, y, dy, dx, dw, dbias, k, stride, pad, dilation, groups, act, workspace):
    """bcnn_hip_dilated_conv_backward. dy is updated in place (dy * act'(y)), dbias and dw accumulate (dw += x dyᵀ, no
    scaling), dx (may be None) is overwritten. workspace: at least f * (c / groups) * k * k floats."""
    n, c, h, w = x.shape
    f = y.shape[1]
    assert wt.numel() == f * (c // groups) * k * k
    _lib.load().bcnn_hip_dilated_conv_backward(_f32(x), _f32(wt), _f32(y), _f32(dy), _f32(dx), _f32(dw), _f32(dbias), n,
                                               c, h, w, f, k, stride, pad, dilation, groups, act, _f32(workspace),
                                               workspace.numel() if workspace is not None else 0)


DILATED_DEPTHWISE_PATHS = ("generic", "plane", "bands")


def dilated_depthwise_path(n, c, h, w, k, s, p, d, backward=False):
    """bcnn_hip_dilated_depthwise_path: the kernel family of the shape, 0 generic, 1 plane, 2 bands
    (DILATED_DEPTHWISE_PATHS); -1 for a shape the workers refuse. Needs no device."""
    return int(_lib.load().bcnn_hip_dilated_depthwise_path(n, c, h, w, k, s, p, d, 1 if backward else 0))


def dilated_depthwise_workspace_size(n, c, h, w, k, s, p, d):
    return int(_lib.load().bcnn_hip_dilated_depthwise_workspace_size(n, c, h, w, k, s, p, d))


def dilated_depthwise_forward(x, wt, bias, y, k, stride, pad, dilation, act=0):
    """bcnn_hip_dilated_depthwise_forward (depthwise_dilated.hip). wt: [c][k][k] (any shape of that size), y
    [n][c][oh][ow] with (oh, ow) = dilated_conv_out_hw(...) is overwritten with act(dilated depthwise convolution + bias)."""
    n, c, h, w = x.shape
    assert wt.numel() == c * k * k and y.shape[1] == c
    _lib.load().bcnn_hip_dilated_depthwise_forward(_f32(x), _f32(wt), _f32(bias), _f32(y), n, c, h, w, k, stride, pad,
                                                   dilation, act)


def dilated_depthwise_backward(x, wt, y, dy, dx, dw, dbias, k, stride, pad, dilation, act, overwrite, workspace):
    """bcnn_hip_dilated_depthwise_backward. dy is updated in place (dy * act'(y)), dbias and dw accumulate (no scaling), dx
    (may be None) accumulates, or is assigned when overwrite is set. workspace: at least
    dilated_depthwise_workspace_size(...) floats."""
    n, c, h, w = x.shape
    assert wt.numel() == c * k * k
    _lib.load().bcnn_hip_dilated_depthwise_backward(_f32(x), _f32(wt), _f32(y), _f32(dy), _f32(dx), _f32(dw),
                                                    _f32(dbias), n, c, h, w, k, stride, pad, dilation, act,
                                                    1 if overwrite else 0, _f32(workspace),
                                                    workspace.numel() if workspace is not None else 0)


def lrn_forward(x, y, local_size, alpha, beta, k):
    """LRN across channels (include/bcnn_hip.h; the reference's bcnn_lrn_layer.c:106-149 with its deviations fixed):
    y = x * (k + alpha/n sum_window x^2)^-beta, overwritten."""
    n, c, h, w = x.shape
    _lib.load().bcnn_hip_lrn_forward(_f32(x), _f32(y), n, c, h, w, local_size, alpha, beta, k)


def lrn_backward(x, dy, dx, local_size, alpha, beta, k, overwrite=0):
    """LRN data gradient from x and dy (s and y recomputed); dx += (overwrite 0) or = (overwrite 1)."""
    n, c, h, w = x.shape
    _lib.load().bcnn_hip_lrn_backward(_f32(x), _f32(dy), _f32(dx), n, c, h, w, local_size, alpha, beta, k, overwrite)


def lifted_struct_workspace_size(batch, k):
    return int(_lib.load().bcnn_hip_lifted_struct_workspace_size(batch, k))


def lifted_struct_forward(x, label, g, record, workspace, margin=1.0, accumulate=False):
    """Lifted-structure loss of a [B][K] embedding with a one-hot [B][K] label (include/bcnn_hip.h): g = (or +=) the
    unscaled gradient the reference's forward leaves (bcnn_lifted_structure_loss.c:16-298), record = 2 x 4 bytes on the
    device, {float loss, int32 P}; workspace holds at least lifted_struct_workspace_size(B, K) floats."""
    b, k = x.shape[0], x.numel() // x.shape[0]
    assert label.numel() == x.numel() and g.numel() == x.numel() and record.numel() * record.element_size() >= 8
    assert workspace.numel() >= lifted_struct_workspace_size(b, k)
    _lib.load().bcnn_hip_lifted_struct_forward(_f32(x), _f32(label), _f32(g), b, k, margin, 1 if accumulate else 0,
                                               record.data_ptr(), _f32(workspace))


def lifted_struct_backward(g, record, scale):
    """g *= scale / P with P read from the record on the device (P == 0: g *= 0), bcnn_lifted_structure_loss.c:300-320"""
    b, k = g.shape[0], g.numel() // g.shape[0]
    _lib.load().bcnn_hip_lifted_struct_backward(_f32(g), b, k, scale, record.data_ptr())


def dropout_forward(x, rate, key, step):
    """In-place dropout of x with the Philox mask of (key, step) (include/bcnn_hip.h; bcnn_dropout_layer.c:66-82)."""
    _lib.load().bcnn_hip_dropout_forward(_f32(x), x.numel(), rate, key, step)


def dropout_backward(dx, rate, key, step):
    """The same mask and scale applied to the gradient in place (bcnn_dropout_layer.c:93-111)."""
    _lib.load().bcnn_hip_dropout_backward(_f32(dx), dx.numel(), rate, key, step)


def batchnorm_forward(x, y, run_mean, run_var, scales, bias, saved_mean, saved_var, workspace, mode,
                      x_norm=None, act=0):
    """bcnn_forward_batchnorm_cpu (bcnn_batchnorm_layer.c:196-242)"""
    n, c, h, w = x.shape
    _lib.load().bcnn_hip_batchnorm_forward(_f32(x), _f32(y), _f32(run_mean), _f32(run_var), _f32(scales),
                                           _f32(bias), _f32(saved_mean), _f32(saved_var), _f32(x_norm),
                                           _f32(workspace), n, c, h * w, mode, act)


def batchnorm_backward(dy, dx, scales, dscales, dbias, saved_mean, saved_var, dmean, dvar, workspace,
                       y=None, act=0, x_norm=None):
    """bcnn_backward_batchnorm_cpu (bcnn_batchnorm_layer.c:301-332)"""
    n, c, h, w = dy.shape
    _lib.load().bcnn_hip_batchnorm_backward(_f32(dy), _f32(dx), _f32(y), act, _f32(scales), _f32(dscales),
                                            _f32(dbias), _f32(saved_mean), _f32(saved_var), _f32(dmean),
                                            _f32(dvar), _f32(x_norm), _f32(workspace), n, c, h * w)


def maxpool_forward(x, y, indexes, size, stride):
    """bcnn_forward_maxpool_layer_cpu (bcnn_maxpool_layer.c:145-191)"""
    n, c, h, w = x.shape
    assert indexes.dtype == torch.int32
    _lib.load().bcnn_hip_maxpool_forward(_f32(x), _f32(y), _p(indexes), n, c, h, w, y.shape[2], y.shape[3],
                                         size, stride)


def maxpool_backward(dy, indexes, dx, size, stride, overwrite=False):
    """bcnn_backward_maxpool_layer_cpu (bcnn_maxpool_layer.c:258-273). overwrite: dx := 0 + sums (the caller skipped
    the zero fill) instead of dx += sums."""
    n, c, h, w = dx.shape
    _lib.load().bcnn_hip_maxpool_backward(_f32(dy), _p(indexes), _f32(dx), n, c, h, w, dy.shape[2], dy.shape[3],
                                          size, stride, 1 if overwrite else 0)


def avgpool_forward(x, y):
    """bcnn_forward_avgpool_layer_cpu (bcnn_avgpool_layer.c:82-99)"""
    n, c, h, w = x.shape
    _lib.load().bcnn_hip_avgpool_forward(_f32(x), _f32(y), n, c, h, w)


def avgpool_backward(dy, dx):
    """bcnn_backward_avgpool_layer_cpu (bcnn_avgpool_layer.c:109-125)"""
    n, c, h, w = dx.shape
    _lib.load().bcnn_hip_avgpool_backward(_f32(dy), _f32(dx), n, c, h, w)


POOL2D_MAX, POOL2D_AVG = 0, 1


class Pool2dDesc(_C.Structure):
    """struct bcnn_hip_pool2d_desc (include/bcnn_hip.h)"""
    _fields_ = [("kind", _C.c_int), ("size", _C.c_int), ("stride", _C.c_int), ("pad", _C.c_int),
                ("ceil_mode", _C.c_int), ("count_include_pad", _C.c_int)]


def _pool2d_desc(kind, size, stride, pad, ceil_mode, count_include_pad):
    kind = {"max": POOL2D_MAX, "avg": POOL2D_AVG}.get(kind, kind)
    return Pool2dDesc(kind, size, stride, pad, 1 if ceil_mode else 0, 1 if count_include_pad else 0)


def pool2d_out_hw(kind, h, w, size, stride, pad=0, ceil_mode=False):
    """bcnn_hip_pool2d_out_extent per axis (torch's max_pool2d / avg_pool2d shape rule); (0, 0) axes are refused
    parameter sets. Needs the library, not a device."""
    d = _pool2d_desc(kind, size, stride, pad, ceil_mode, True)
    L = _lib.load()
    return int(L.bcnn_hip_pool2d_out_extent(_C.byref(d), h)), int(L.bcnn_hip_pool2d_out_extent(_C.byref(d), w))


class InterpDesc(_C.Structure):
    """struct bcnn_hip_interp_desc (include/bcnn_hip.h)"""
    _fields_ = [("out_h", _C.c_int), ("out_w", _C.c_int), ("align_corners", _C.c_int)]


def interp_out_hw(h, w, scale=0, zoom=0, out_h=0, out_w=0):
    """the interp node's output extents, exactly one form: scale >= 1 (in * scale), zoom >= 1 ((in - 1) * zoom + 1,
    Caffe-DeepLab's Interp) or out_h, out_w > 0; (0, 0) for anything else, an extent of 2^31 - 1 or more included.
    A restatement in Python for shaping tensors: the library's rule is bcnn_interp_out_extent (csrc/interp_rule.h), which
    is inline in the builder and in bcnn_resize_net and not exported; tests/test_interp_graph.py holds the node's shapes
    to this function."""
    if min(h, w) < 1 or min(scale, zoom, out_h, out_w) < 0 or (out_h > 0) != (out_w > 0):
        return 0, 0
    if (scale > 0) + (zoom > 0) + (out_w > 0) != 1:
        return 0, 0
    if scale:
        out = h * scale, w * scale
    elif zoom:
        out = (h - 1) * zoom + 1, (w - 1) * zoom + 1
    else:
        out = out_h, out_w
    return out if max(out) < 0x7fffffff else (0, 0)


def interp_forward(x, y, align_corners=False):
    """bcnn_hip_interp_forward: y (its shape gives the output extents) = bilinear interpolation of x, the rule of
    torch.nn.functional.interpolate(x, size=y.shape[2:], mode="bilinear", align_corners=align_corners)"""
    n, c, h, w = x.shape
    assert tuple(y.shape[:2]) == (n, c) and y.dim() == 4, "y is [n][c][out_h][out_w]"
    d = InterpDesc(y.shape[2], y.shape[3], 1 if align_corners else 0)
    _lib.load().bcnn_hip_interp_forward(_C.byref(d), _f32(x), _f32(y), n, c, h, w)


def interp_backward(dy, dx, align_corners=False, overwrite=False):
    """bcnn_hip_interp_backward: dx += (overwrite: dx = 0 +) the gathered gradient of interp_forward; no atomics"""
    n, c, h, w = dx.shape
    assert tuple(dy.shape[:2]) == (n, c) and dy.dim() == 4, "dy is [n][c][out_h][out_w]"
    d = InterpDesc(dy.shape[2], dy.shape[3], 1 if align_corners else 0)
    _lib.load().bcnn_hip_interp_backward(_C.byref(d), _f32(dy), _f32(dx), n, c, h, w, 1 if overwrite else 0)


def interp_axis_taps(size_in, size_out, align_corners=False):
    """bcnn_hip_interp_axis_taps (host code of the library, no device): numpy (i0, i1, l1) of one axis"""
    import numpy as np
    i0, i1 = np.zeros(size_out, np.int32), np.zeros(size_out, np.int32)
    l1 = np.zeros(size_out, np.float32)
    _lib.load().bcnn_hip_interp_axis_taps(size_in, size_out, 1 if align_corners else 0, i0.ctypes.data, i1.ctypes.data,
                                          l1.ctypes.data)
    return i0, i1, l1


LOSS_NORM_NONE, LOSS_NORM_VALID, LOSS_NORM_VALID_PER_IMAGE = 0, 1, 2
LOSS_NORMS = {"none": LOSS_NORM_NONE, "valid": LOSS_NORM_VALID, "valid_per_image": LOSS_NORM_VALID_PER_IMAGE}


class SoftmaxLossDesc(_C.Structure):
    """struct bcnn_hip_softmax_loss_desc (include/bcnn_hip.h)"""
    _fields_ = [("ignore_label", _C.c_int), ("norm", _C.c_int), ("scale", _C.c_float)]


class SoftmaxLossRecord(_C.Structure):
    """struct bcnn_hip_softmax_loss_record (include/bcnn_hip.h): what a forward with a label leaves on the device"""
    _fields_ = [("loss", _C.c_float), ("grad_factor", _C.c_float), ("valid", _C.c_int), ("ignored", _C.c_int),
                ("out_of_range", _C.c_int), ("correct", _C.c_int)]


def softmax_loss_c_reg():
    """the largest class count whose logits the pixel kernels of the softmax loss hold in registers"""
    return int(_lib.load().bcnn_hip_softmax_loss_c_reg())


def softmax_loss_record():
    """a zeroed device record (6 words, as an int32 tensor) for softmax_loss_forward / softmax_loss_backward"""
    import torch
    return torch.zeros(_C.sizeof(SoftmaxLossRecord) // 4, dtype=torch.int32, device="cuda")


def softmax_loss_read_record(record):
    """the device record as a dict (loss, grad_factor, valid, ignored, out_of_range, correct); synchronises"""
    raw = record.cpu().numpy().tobytes()
    r = SoftmaxLossRecord.from_buffer_copy(raw)
    return {name: getattr(r, name) for name, _ in SoftmaxLossRecord._fields_}


def _softmax_loss_desc(ignore_label, normalize, scale):
    return SoftmaxLossDesc(int(ignore_label), LOSS_NORMS.get(normalize, normalize), float(scale))


def softmax_loss_forward(x, label, p, record, ignore_label=-1, normalize="valid_per_image", scale=1.0):
    """bcnn_hip_softmax_loss_forward: p = softmax over dim 1 of x ([n][C][hw] or [n][C][h][w]); with `label` ([n][1][...],
    class indices as floats) and `record` also the loss, scale / D and the counts, into the record. label None: p only."""
    n, c = x.shape[:2]
    hw = x.numel() // max(n * c, 1)
    assert p.numel() == x.numel() and (label is None or label.numel() == n * hw)
    d = _softmax_loss_desc(ignore_label, normalize, scale)
    _lib.load().bcnn_hip_softmax_loss_forward(_C.byref(d), _f32(x), _f32(label) if label is not None else None, _f32(p),
                                              record.data_ptr() if record is not None else None, n, c, hw)


def softmax_loss_backward(p, label, record, dx, ignore_label=-1, normalize="valid_per_image", scale=1.0, overwrite=False):
    """bcnn_hip_softmax_loss_backward: dx += (overwrite: dx =) record.grad_factor * (p - onehot(label)) on valid pixels"""
    n, c = p.shape[:2]
    hw = p.numel() // max(n * c, 1)
    assert dx.numel() == p.numel() and label.numel() == n * hw
    d = _softmax_loss_desc(ignore_label, normalize, scale)
    _lib.load().bcnn_hip_softmax_loss_backward(_C.byref(d), _f32(p), _f32(label), record.data_ptr(), _f32(dx), n, c, hw,
                                               1 if overwrite else 0)


def softmax_loss_confusion(p, label, ignore_label=-1):
    """bcnn_hip_softmax_loss_confusion: the C x C matrix (row = label, column = first argmax of p) over valid pixels, as an
    int64 numpy array; synchronises"""
    import torch
    n, c = p.shape[:2]
    hw = p.numel() // max(n * c, 1)
    assert label.numel() == n * hw
    counts = torch.empty(c * c, dtype=torch.int32, device=p.device)
    d = _softmax_loss_desc(ignore_label, LOSS_NORM_NONE, 1.0)
    _lib.load().bcnn_hip_softmax_loss_confusion(_C.byref(d), _f32(p), _f32(label), counts.data_ptr(), n, c, hw)
    return counts.cpu().numpy().astype("int64").reshape(c, c)


IMAGE_FIT_STRETCH, IMAGE_FIT_LETTERBOX = 0, 1


class LabelMapImage(_C.Structure):
    """struct bcnn_hip_label_map_image (include/bcnn_hip.h): the extent of an image and its rectangle of the tensor plane"""
    _fields_ = [("out_w", _C.c_int), ("out_h", _C.c_int), ("roi_x", _C.c_int), ("roi_y", _C.c_int), ("roi_w", _C.c_int),
                ("roi_h", _C.c_int)]


def _label_map_images(images):
    """a C array of LabelMapImage from LabelMapImage objects or (out_w, out_h, roi_x, roi_y, roi_w, roi_h) tuples"""
    arr = (LabelMapImage * max(len(images), 1))()
    for b, im in enumerate(images):
        arr[b] = im if isinstance(im, LabelMapImage) else LabelMapImage(*[int(v) for v in im])
    return arr


def label_map_fit(fit, w, h, iw, ih):
    """bcnn_hip_label_map_fit (host code of the library, no device): (out_w, out_h, roi_x, roi_y, roi_w, roi_h) of an
    iw x ih image in the w x h plane for IMAGE_FIT_STRETCH / IMAGE_FIT_LETTERBOX, or None when the library refuses"""
    out = LabelMapImage(-1, -1, -1, -1, -1, -1)
    if _lib.load().bcnn_hip_label_map_fit(int(fit), int(w), int(h), int(iw), int(ih), _C.byref(out)) != 0:
        assert tuple(getattr(out, name) for name, _ in LabelMapImage._fields_) == (-1,) * 6, "a refusal wrote its output"
        return None
    return tuple(getattr(out, name) for name, _ in LabelMapImage._fields_)


def label_maps_plan(images, c, h, w, with_truths=False):
    """bcnn_hip_label_maps_plan (host, no device): (row_strides, offsets, total_bytes) of the result block of a call over
    `images` (see label_maps), or None when the library refuses (and then wrote nothing)"""
    import numpy as np
    k = len(images)
    strides = np.full(max(k, 1), 0xFFFFFFFF, np.uint32)
    offsets = np.full(max(k, 1), 2 ** 64 - 1, np.uint64)
    total = _C.c_ulonglong(2 ** 64 - 1)
    st = _lib.load().bcnn_hip_label_maps_plan(_C.cast(_label_map_images(images), _C.c_void_p), k, int(c), int(h), int(w),
                                              1 if with_truths else 0, strides.ctypes.data, offsets.ctypes.data,
                                              _C.cast(_C.pointer(total), _C.c_void_p))
    if st != 0:
        assert (strides == 0xFFFFFFFF).all() and (offsets == 2 ** 64 - 1).all() and total.value == 2 ** 64 - 1
        return None
    return [int(v) for v in strides[:k]], [int(v) for v in offsets[:k]], int(total.value)


def label_maps(x, images, align_corners=False, truths=None, ignore_label=-1, labels=True, counts=None):
    """bcnn_hip_label_maps_batch: x is the [n][C][h][w] float32 device tensor, images one LabelMapImage or (out_w, out_h,
    roi_x, roi_y, roi_w, roi_h) per batch entry from 0 on (label_map_fit makes them). Returns the list of uint8 numpy
    arrays [out_h][out_w]: per pixel the first argmax over C of the bilinear resampling of the rectangle. With `truths`
    (uint8 arrays of the same extents) returns (labels, counts, ignored, out_of_range): counts the C x C int64 matrix
    (row = truth, column = label) over the valid pixels -- added into `counts` when one is given. labels=False asks for
    the counts alone (None in place of the list). Synchronises. Raises ValueError when the library refuses."""
    import numpy as np
    n, c, h, w = x.shape
    k = len(images)
    arr = _label_map_images(images)
    out = [np.empty((arr[b].out_h, arr[b].out_w), np.uint8) for b in range(k)] if labels else None
    lptr = (_C.c_void_p * max(k, 1))(*[a.ctypes.data for a in out]) if labels else None
    tptr, keep = None, []
    ign, oor = _C.c_longlong(0), _C.c_longlong(0)
    if truths is not None:
        keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in truths]
        assert len(keep) == k and all(t.shape == (arr[b].out_h, arr[b].out_w) for b, t in enumerate(keep)), \
            "one truth map per image, of its size"
        tptr = (_C.c_void_p * max(k, 1))(*[t.ctypes.data for t in keep])
        if counts is None:
            counts = np.zeros((c, c), np.int64)
        assert counts.dtype == np.int64 and counts.size == c * c and counts.flags.c_contiguous
    st = _lib.load().bcnn_hip_label_maps_batch(
        _f32(x), n, c, h, w, 1 if align_corners else 0, _C.cast(arr, _C.c_void_p), k,
        None if lptr is None else _C.cast(lptr, _C.c_void_p), None, None if tptr is None else _C.cast(tptr, _C.c_void_p),
        None, int(ignore_label), None if truths is None else counts.ctypes.data, _C.cast(_C.pointer(ign), _C.c_void_p),
        _C.cast(_C.pointer(oor), _C.c_void_p))
    if st != 0:
        raise ValueError("bcnn_hip_label_maps_batch refused the call (status %d)" % st)
    if truths is None:
        return out
    return out, counts, int(ign.value), int(oor.value)


def pool2d_forward(x, y, indexes, kind, size, stride, pad=0, ceil_mode=False, count_include_pad=True):
    """bcnn_hip_pool2d_forward: windowed max / average pooling with `pad` on all four sides. indexes (int32, y's shape)
    may be None: max pooling then stores no winners; average pooling never does."""
    n, c, h, w = x.shape
    d = _pool2d_desc(kind, size, stride, pad, ceil_mode, count_include_pad)
    assert tuple(y.shape) == (n, c) + pool2d_out_hw(kind, h, w, size, stride, pad, ceil_mode), "y has the pooled shape"
    assert indexes is None or (indexes.dtype == torch.int32 and indexes.numel() == y.numel())
    _lib.load().bcnn_hip_pool2d_forward(_C.byref(d), _f32(x), _f32(y), _p(indexes), n, c, h, w)


def pool2d_backward(dy, indexes, dx, kind, size, stride, pad=0, ceil_mode=False, count_include_pad=True, overwrite=False):
    """bcnn_hip_pool2d_backward: dx += (overwrite: dx = 0 +) the gathered gradient; indexes as the forward stored them
    (max), ignored for average pooling."""
    n, c, h, w = dx.shape
    d = _pool2d_desc(kind, size, stride, pad, ceil_mode, count_include_pad)
    assert tuple(dy.shape) == (n, c) + pool2d_out_hw(kind, h, w, size, stride, pad, ceil_mode), "dy has the pooled shape"
    assert indexes is None or (indexes.dtype == torch.int32 and indexes.numel() == dy.numel())
    _lib.load().bcnn_hip_pool2d_backward(_C.byref(d), _f32(dy), _p(indexes), _f32(dx), n, c, h, w, 1 if overwrite else 0)


def activation_forward(x, act, slopes=None, spatial=1, channels=1):
    """bcnn_forward_activation_cpu (bcnn_activation_layer.c:90-146), in place"""
    _lib.load().bcnn_hip_activation_forward(_f32(x), x.numel(), act, _f32(slopes), spatial, channels)


def activation_forward_keep(x, x_saved, act):
    """bcnn_hip_activation_forward_keep: x = act(x) in place and, unless x_saved is None, x_saved = the input. The forward
    of hard_swish / swish / mish, whose backward (activation_backward_from_input) needs the input."""
    assert x_saved is None or x_saved.numel() == x.numel()
    _lib.load().bcnn_hip_activation_forward_keep(_f32(x), _f32(x_saved), x.numel(), act)


def activation_backward_from_input(x_saved, dx, act):
    """bcnn_hip_activation_backward_from_input: dx *= act'(x_saved) in place; hard_swish / swish / mish only"""
    assert x_saved.numel() == dx.numel()
    _lib.load().bcnn_hip_activation_backward_from_input(_f32(x_saved), _f32(dx), dx.numel(), act)


def _scale_gate_form(x, gate):
    n, c, h, w = x.shape
    if tuple(gate.shape) == (n, c, h, w) and h * w > 1:
        return 1
    assert gate.numel() == n * c, "the gate is [N,C,1,1] or has x's shape"
    return 0


def scale_channels_forward(x, gate, y):
    """bcnn_hip_scale_channels_forward: y = x * gate; gate is [N,C,1,1] (one factor per plane) or x's shape"""
    n, c, h, w = x.shape
    assert y.shape == x.shape
    _lib.load().bcnn_hip_scale_channels_forward(_f32(x), _f32(gate), _f32(y), n, c, h * w, _scale_gate_form(x, gate))


def scale_channels_backward(x, gate, dy, dx, dgate):
    """bcnn_hip_scale_channels_backward: dx += dy * gate, dgate += the plane sums of dy * x (dy * x itself for a gate of
    x's shape), in one sweep; dx or dgate may be None (that half is skipped)"""
    n, c, h, w = x.shape
    assert dy.shape == x.shape and (dx is None or dx.shape == x.shape) and (dgate is None or dgate.numel() == gate.numel())
    _lib.load().bcnn_hip_scale_channels_backward(_f32(x), _f32(gate), _f32(dy), _f32(dx), _f32(dgate), n, c, h * w,
                                                 _scale_gate_form(x, gate))


GROUP_NORM_PATHS = ("lanes", "resident", "split")


def group_norm_path(n, c, hw, groups, backward=False):
    """bcnn_hip_group_norm_path: the kernel family of the shape, 0 lanes, 1 resident, 2 split (GROUP_NORM_PATHS)"""
    return int(_lib.load().bcnn_hip_group_norm_path(n, c, hw, groups, 1 if backward else 0))


def group_norm_forward(x, gamma, beta, y, mean, rstd, groups, eps=1e-5):
    """bcnn_hip_group_norm_forward: y = (x - mean) * rstd * gamma[ch] + beta[ch], statistics per (image, group) over its
    (C / groups) * H * W values; mean and rstd ([N * groups]) receive them, or are both None (nothing is stored)"""
    n, c, h, w = x.shape
    assert y.shape == x.shape and gamma.numel() == c and beta.numel() == c and groups > 0 and c % groups == 0
    assert (mean is None) == (rstd is None) and (mean is None or (mean.numel() == n * groups and rstd.numel() == n * groups))
    _lib.load().bcnn_hip_group_norm_forward(_f32(x), _f32(gamma), _f32(beta), _f32(y), _f32(mean), _f32(rstd), n, c, h * w,
                                            groups, eps)


def group_norm_backward(x, gamma, mean, rstd, dy, dx, dgamma, dbeta, groups, overwrite=False):
    """bcnn_hip_group_norm_backward from the stored mean and rstd: dx = (overwrite) or += the data gradient,
    dgamma += sum dy * xh, dbeta += sum dy; each of dx, dgamma, dbeta may be None (that output is skipped)"""
    n, c, h, w = x.shape
    assert dy.shape == x.shape and (dx is None or dx.shape == x.shape) and gamma.numel() == c and c % groups == 0
    assert mean.numel() == n * groups and rstd.numel() == n * groups
    assert (dgamma is None or dgamma.numel() == c) and (dbeta is None or dbeta.numel() == c)
    _lib.load().bcnn_hip_group_norm_backward(_f32(x), _f32(gamma), _f32(mean), _f32(rstd), _f32(dy), _f32(dx), _f32(dgamma),
                                             _f32(dbeta), n, c, h * w, groups, 1 if overwrite else 0)


def activation_backward(x, dx, act, slopes=None, dslopes=None, spatial=1, channels=1):
    """bcnn_backward_activation_cpu (bcnn_activation_layer.c:165-226), dx in place"""
    _lib.load().bcnn_hip_activation_backward(_f32(x), _f32(dx), x.numel(), act, _f32(slopes), _f32(dslopes),
                                             spatial, channels)


def depthwise_forward(x, wt, bias, y, k, stride, pad, act=0):
    """bcnn_forward_depthwise_conv_layer_cpu (bcnn_depthwise_conv_layer.c:165-293)"""
    n, c, h, w = x.shape
    _lib.load().bcnn_hip_depthwise_forward(_f32(x), _f32(wt), _f32(bias), _f32(y), n, c, h, w, k, stride, pad, act)


def depthwise_backward(x, wt, y, dy, dx, dw, dbias, k, stride, pad, act=0, overwrite=False):
    """bcnn_backward_depthwise_conv_layer_cpu (bcnn_depthwise_conv_layer.c:295-547); overwrite: dx = 0 + sums
    (the executor's no-fill mode for a sole gradient writer) instead of dx += sums"""
    n, c, h, w = x.shape
    _lib.load().bcnn_hip_depthwise_backward(_f32(x), _f32(wt), _f32(y), _f32(dy), _f32(dx), _f32(dw),
                                            _f32(dbias), n, c, h, w, k, stride, pad, act, 1 if overwrite else 0)


def batchnorm_apply(x, y, scales, bias, mean, var, act=0):
    """y = act((x - mean) / sqrtf(var + 1e-6) * scale + bias) with given statistics (bcnn_batchnorm_layer.c:226-241)"""
    n, c, h, w = x.shape
    _lib.load().bcnn_hip_batchnorm_apply(_f32(x), _f32(y), _f32(scales), _f32(bias), _f32(mean), _f32(var), n, c, h * w, act)


def maxpool_bn_fusable(x, out_h, out_w, size, stride, act):
    n, c, h, w = x.shape
    return bool(_lib.load().bcnn_hip_maxpool_bn_fusable(n, c, h, w, out_h, out_w, size, stride, act, _f32(x)))


def maxpool_forward_bn(x, y, indexes, size, stride, scales, bias, mean, var, act):
    """max-pooling over act(batch-norm(x)) normalised on the fly: bcnn_forward_maxpool_layer_cpu
    (bcnn_maxpool_layer.c:145-191) on the tensor bcnn_batchnorm_layer.c:226-241 would have written"""
    n, c, h, w = x.shape
    assert indexes.dtype == torch.int32
    _lib.load().bcnn_hip_maxpool_forward_bn(_f32(x), _f32(y), _p(indexes), n, c, h, w, y.shape[2], y.shape[3], size, stride,
                                            _f32(scales), _f32(bias), _f32(mean), _f32(var), act)


def depthwise_forward_stats(x, wt, bias, y, k, stride, pad, act, stats):
    """bcnn_hip_depthwise_forward that also leaves per-channel (sum, sum of squares) partials of y in `stats`;
    returns the number of partials per channel (0: none, run the plain batch-norm forward)"""
    n, c, h, w = x.shape
    return _lib.load().bcnn_hip_depthwise_forward_stats(_f32(x), _f32(wt), _f32(bias), _f32(y), n, c, h, w, k, stride,
                                                        pad, act, _f32(stats), stats.numel())


def depthwise_stats_size(n, c, h, w, k, stride, pad):
    return _lib.load().bcnn_hip_depthwise_stats_size(n, c, h, w, k, stride, pad)


def batchnorm_forward_stats(x, y, run_mean, run_var, scales, bias, saved_mean, saved_var, workspace, mode, stats, splits):
    """bcnn_forward_batchnorm_cpu (bcnn_batchnorm_layer.c:196-242) with the statistics partials of the producer"""
    n, c, h, w = x.shape
    _lib.load().bcnn_hip_batchnorm_forward_stats(_f32(x), _f32(y), _f32(run_mean), _f32(run_var), _f32(scales), _f32(bias),
                                                 _f32(saved_mean), _f32(saved_var), None, _f32(workspace), n, c, h * w,
                                                 mode, 0, _f32(stats), splits)


def depthwise_bn_fusable(n, c, h, w, k, stride, pad, act):
    return bool(_lib.load().bcnn_hip_depthwise_bn_fusable(n, c, h, w, k, stride, pad, act))


def batchnorm_backward_sums(dy, scales, dscales, dbias, saved_mean, saved_var, dmean, dvar, x):
    """first sweep of bcnn_backward_batchnorm_cpu (bcnn_batchnorm_layer.c:301-332): the per-channel sums only"""
    n, c, h, w = x.shape
    _lib.load().bcnn_hip_batchnorm_backward_sums(_f32(dy), _f32(scales), _f32(dscales), _f32(dbias), _f32(saved_mean),
                                                 _f32(saved_var), _f32(dmean), _f32(dvar), _f32(x), n, c, h * w)


def depthwise_backward_bn(x, wt, y, dz, dx, dw, dbias, k, stride, pad, act, overwrite, mean, var, scales, dmean, dvar):
    """depthwise backward on the gradient a following stand-alone batch-norm node would hand down, applied on the fly"""
    n, c, h, w = x.shape
    _lib.load().bcnn_hip_depthwise_backward_bn(_f32(x), _f32(wt), _f32(y), _f32(dz), _f32(dx), _f32(dw), _f32(dbias), n, c,
                                               h, w, k, stride, pad, act, 1 if overwrite else 0, _f32(mean), _f32(var),
                                               _f32(scales), _f32(dmean), _f32(dvar))


def gemm(ta, tb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc):
    """bcnn_gemm (bcnn_mat.c:2627-2650)"""
    _lib.load().bcnn_hip_gemm(ta, tb, m, n, k, alpha, _f32(a), lda, _f32(b), ldb, beta, _f32(c), ldc)


def im2col(im, k, pad, stride, col):
    c, h, w = im.shape
    _lib.load().bcnn_hip_im2col(_f32(im), c, h, w, k, pad, stride, _f32(col))


def col2im(col, k, pad, stride, im):
    c, h, w = im.shape
    _lib.load().bcnn_hip_col2im(_f32(col), c, h, w, k, pad, stride, _f32(im))


def adam_update(w, b, dw, db, adam_m, adam_v, batch_size, it, beta1, beta2, lr, momentum, decay):
    """bcnn_adam_update_cpu (bcnn_learner.c:106-131)"""
    _lib.load().bcnn_hip_adam_update(_f32(w), _f32(b), _f32(dw), _f32(db), _f32(adam_m), _f32(adam_v),
                                     w.numel() if w is not None else 0, b.numel() if b is not None else 0,
                                     batch_size, it, beta1, beta2, lr, momentum, decay)


def sgd_update(w, b, dw, db, batch_size, lr, momentum, decay):
    """bcnn_sgd_update_cpu (bcnn_learner.c:67-83)"""
    _lib.load().bcnn_hip_sgd_update(_f32(w), _f32(b), _f32(dw), _f32(db), w.numel() if w is not None else 0,
                                    b.numel() if b is not None else 0, batch_size, lr, momentum, decay)


class LetterboxImage(_C.Structure):
    """bcnn_hip_letterbox_image (include/bcnn_hip.h)"""
    _fields_ = [("pixels", _C.c_void_p), ("w", _C.c_int32), ("h", _C.c_int32), ("new_w", _C.c_int32), ("new_h", _C.c_int32),
                ("x_off", _C.c_int32), ("y_off", _C.c_int32)]


def augment_letterbox_batch(dst, images, boxes, records=None, taps=None, swap_to_bgr=False, num_samples=None):
    """bcnn_hip_augment_letterbox_batch: dst is the [n][c][h][w] float32 device tensor; images are HOST uint8 arrays
    [hi][wi][c] (numpy, C-contiguous), boxes one (new_w, new_h, x_off, y_off) per image, records a HOST int32 array
    [num][8] (bcnn_hip_augment_record; None: identity records), taps a HOST int32 array [num][(w + h) * 2] or None.
    Returns the entry's status: 0, or 1 with nothing staged or queued."""
    import numpy as np
    n, c, h, w = dst.shape
    num = len(images) if num_samples is None else num_samples
    arr = (LetterboxImage * max(len(images), 1))()
    keep = []
    for b, (img, box) in enumerate(zip(images, boxes)):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        keep.append(img)
        hi, wi = img.shape[:2]
        arr[b] = LetterboxImage(img.ctypes.data, wi, hi, *[int(v) for v in box])
    if records is None:
        records = np.zeros((max(num, 1), 8), np.int32)
    records = np.ascontiguousarray(records, dtype=np.int32)
    if taps is not None:
        taps = np.ascontiguousarray(taps, dtype=np.int32)
    return int(_lib.load().bcnn_hip_augment_letterbox_batch(
        _f32(dst), n, c, h, w, num, _C.cast(arr, _C.c_void_p), records.ctypes.data,
        None if taps is None else taps.ctypes.data, 1 if swap_to_bgr else 0))


def augment_label_batch(label, maps, records=None, taps=None, fill=255, num_samples=None):
    """bcnn_hip_augment_label_batch: label is the [n][1][h][w] float32 device tensor (written in place and returned by
    reference: planes num_samples .. n - 1 are left alone); maps a HOST uint8 array [num][h][w] of class indices, records
    a HOST int32 array [num][8] (bcnn_hip_augment_record; None: identity records), taps a HOST int32 array
    [num][(w + h) * 2] or None. Returns the entry's status: 0, or 1 with nothing staged or queued."""
    import numpy as np
    n, _, h, w = label.shape
    maps = np.ascontiguousarray(maps, dtype=np.uint8)
    num = maps.shape[0] if num_samples is None else num_samples
    if records is None:
        records = np.zeros((max(num, 1), 8), np.int32)
    records = np.ascontiguousarray(records, dtype=np.int32)
    if taps is not None:
        taps = np.ascontiguousarray(taps, dtype=np.int32)
    return int(_lib.load().bcnn_hip_augment_label_batch(
        _f32(label), n, h, w, num, maps.ctypes.data, records.ctypes.data, None if taps is None else taps.ctypes.data,
        int(fill)))


_bip = None


def _libbip():
    global _bip
    if _bip is None:
        import os
        _bip = _C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libbip.so"))
        i32, vp = _C.c_int32, _C.c_void_p
        _bip.bip_warp_label_map.restype = _C.c_int
        _bip.bip_warp_label_map.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp]
    return _bip


def warp_label_map(label_map, record=None, taps=None, fill=255):
    """bip_warp_label_map (libbip, host): the label map that belongs to an augmented image. label_map is a HOST uint8
    array [h][w], record the 8 int32 of a bcnn_hip_augment_record (flags, x_ul, y_ul, ca, sa, ...; None: the identity),
    taps the (w + h) * 2 int32 of its tap table or None. Returns the warped uint8 array [h][w]; raises ValueError with
    the bip_status when the function refuses."""
    import numpy as np
    m = np.ascontiguousarray(label_map, dtype=np.uint8)
    h, w = m.shape
    r = np.zeros(8, np.int32) if record is None else np.ascontiguousarray(record, dtype=np.int32).reshape(-1)
    tx = ty = None
    if taps is not None:
        t = np.ascontiguousarray(taps, dtype=np.int32).reshape(-1)
        tx, ty = t.ctypes.data, t.ctypes.data + 8 * w
    out = np.empty_like(m)
    st = _libbip().bip_warp_label_map(m.ctypes.data, w, h, int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), tx, ty,
                                      int(fill), out.ctypes.data)
    if st != 0:
        raise ValueError("bip_warp_label_map: status %d" % st)
    return out
