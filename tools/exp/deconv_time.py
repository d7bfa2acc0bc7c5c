#!/usr/bin/env python3
"""Transposed convolution: the fused kernels of deconv.hip (bcnn_hip_deconv_forward / _backward) against the
reference's structure on this library's own kernels -- per image bcnn_hip_gemm (Wᵀ x) + bcnn_hip_col2im for the
forward, bcnn_hip_im2col + bcnn_hip_gemm for the weight and the data gradient (bcnn_deconv_layer.c:150-246). N = 32,
activation none, device events on the library's stream after warm-up.
  forward : fused = bcnn_hip_deconv_forward (bias included);  baseline = 32 x (gemm + col2im) + bcnn_hip_add_bias
  dW      : fused = bcnn_hip_deconv_backward without dx / db;  baseline = 32 x (im2col + gemm, alpha 1/N, beta 1)
  dx      : fused = bcnn_hip_deconv_backward without dW / db;  baseline = 32 x (im2col + gemm, beta 0)
The baseline runs on the uncropped s (h - 1) + k extent (col2im / im2col with pad 0, as the reference does); with
pad > 0 it is a timing stand-in only (the reference's padded result is not the transposed convolution). For pad == 0
the forward, dW and dx of both are compared on the timed data.
FLOP = 2 N c_in c_out k^2 h w per direction; peak 157.3 TFLOP/s (fp32 MFMA).
    python tools/exp/deconv_time.py [--reps 20]
Under rocprofv3:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/exp/deconv_time.py --reps 5"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: one HIP runtime for torch and the library)

from bcnn_amd import _lib, ops  # noqa: E402

PEAK = 157.3e12
SHAPES = [  # name, n, c_in, h, w, c_out, k, s, p
    ("dcgan_256to128_32to64_k4s2p1", 32, 256, 32, 32, 128, 4, 2, 1),
    ("unet_128to64_64to128_k2s2p0", 32, 128, 64, 64, 64, 2, 2, 0),
    ("same_64to64_56_k3s1p0", 32, 64, 56, 56, 64, 3, 1, 0),
]


def timed(L, fn, reps, warm=3):
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    for _ in range(warm):
        fn()
    L.bcnn_hip_sync()
    L.bcnn_hip_event_record(e0)
    for _ in range(reps):
        fn()
    L.bcnn_hip_event_record(e1)
    L.bcnn_hip_event_sync(e1)
    ms = L.bcnn_hip_event_elapsed_ms(e0, e1) / reps
    L.bcnn_hip_event_destroy(e0)
    L.bcnn_hip_event_destroy(e1)
    return ms


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def one_shape(L, name, n, c, h, w, f, k, s, p, reps):
    ho, wo = ops.deconv_out_hw(h, w, k, s, p)
    hf, wf = s * (h - 1) + k, s * (w - 1) + k
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((n, c, h, w), device="cuda", generator=g) * 2 - 1
    wt = (torch.rand((c, f, k, k), device="cuda", generator=g) - 0.5) * 0.2
    b = torch.zeros(f, device="cuda")
    y = torch.empty((n, f, ho, wo), device="cuda")
    dy = torch.rand((n, f, ho, wo), device="cuda", generator=g) * 2 - 1
    dw = torch.zeros_like(wt)
    dx = torch.empty_like(x)
    ws = torch.zeros(ops.deconv_workspace_size(n, c, h, w, f, k, s, p), device="cuda")
    X, W, B, Y, DY, DW, DX, WS = (t.data_ptr() for t in (x, wt, b, y, dy, dw, dx, ws))
    # baseline buffers: one image's column matrix, outputs on the uncropped extent
    col = torch.empty(f * k * k * h * w, device="cuda")
    yb = torch.empty((n, f, hf, wf), device="cuda")
    dyb = torch.zeros((n, f, hf, wf), device="cuda")
    dyb[:, :, p:hf - p, p:wf - p] = dy
    dwb = torch.zeros_like(wt)
    dxb = torch.empty_like(x)
    COL, YB, DYB, DWB, DXB = (t.data_ptr() for t in (col, yb, dyb, dwb, dxb))
    m, hw, fo = f * k * k, h * w, f * hf * wf

    def fwd():
        L.bcnn_hip_deconv_forward(X, W, B, Y, n, c, h, w, f, k, s, p, 0)

    def dw_fused():
        L.bcnn_hip_deconv_backward(X, W, Y, DY, None, DW, None, n, c, h, w, f, k, s, p, 0, WS, ws.numel())

    def dx_fused():
        L.bcnn_hip_deconv_backward(X, W, Y, DY, DX, None, None, n, c, h, w, f, k, s, p, 0, WS, ws.numel())

    def fwd_base():
        for i in range(n):
            L.bcnn_hip_gemm(1, 0, m, hw, c, 1.0, W, m, X + 4 * i * c * hw, hw, 0.0, COL, hw)
            L.bcnn_hip_col2im(COL, f, hf, wf, k, 0, s, YB + 4 * i * fo)
        L.bcnn_hip_add_bias(YB, B, n, f, hf * wf)

    def dw_base():
        for i in range(n):
            L.bcnn_hip_im2col(DYB + 4 * i * fo, f, hf, wf, k, 0, s, COL)
            L.bcnn_hip_gemm(0, 1, c, m, hw, 1.0 / n, X + 4 * i * c * hw, hw, COL, hw, 1.0, DWB, m)

    def dx_base():
        for i in range(n):
            L.bcnn_hip_im2col(DYB + 4 * i * fo, f, hf, wf, k, 0, s, COL)
            L.bcnn_hip_gemm(0, 0, c, hw, m, 1.0, W, m, COL, hw, 0.0, DXB + 4 * i * c * hw, hw)

    flop = 2.0 * n * c * f * k * k * h * w
    out = dict(shape=dict(n=n, c_in=c, h=h, w=w, c_out=f, k=k, s=s, p=p), gflop=flop / 1e9)
    for key, fn in (("fwd", fwd), ("fwd_base", fwd_base), ("dw", dw_fused), ("dw_base", dw_base), ("dx", dx_fused),
                    ("dx_base", dx_base)):
        ms = timed(L, fn, reps)
        out[key] = dict(ms=ms, tflops=flop / (ms * 1e-3) / 1e12, of_peak=flop / (ms * 1e-3) / PEAK)
    # same results (pad 0: the baseline is the reference's computation); dw / dwb hold the sums of equally many calls
    L.bcnn_hip_sync()
    dw.zero_()
    dwb.zero_()
    fwd(); fwd_base(); dw_fused(); dw_base(); dx_fused(); dx_base()  # noqa: E702
    L.bcnn_hip_sync()
    if p == 0:
        out["rel_diff"] = dict(y=rel(y, yb), dw=rel(dw, dwb), dx=rel(dx, dxb))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    L = _lib.load()
    res = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    print("%-30s %-8s %9s %8s %7s   %9s %8s   %s" % ("shape", "pass", "fused ms", "TFLOP/s", "of pk", "base ms",
                                                   "TFLOP/s", "speed-up"))
    for sh in SHAPES:
        r = one_shape(L, *sh, reps=args.reps)
        res["shapes"][sh[0]] = r
        for key in ("fwd", "dw", "dx"):
            a, b = r[key], r[key + "_base"]
            print("%-30s %-8s %9.3f %8.1f %7.3f   %9.3f %8.1f   %.2fx" % (sh[0], key, a["ms"], a["tflops"], a["of_peak"],
                                                                         b["ms"], b["tflops"], b["ms"] / a["ms"]))
        if "rel_diff" in r:
            print("%-30s same results: max |diff| / max |baseline|  y %.2g  dw %.2g  dx %.2g" % (
                sh[0], r["rel_diff"]["y"], r["rel_diff"]["dw"], r["rel_diff"]["dx"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
