#!/usr/bin/env python3
"""Forward, dX and dW times of the large-kernel convolution family (bcnn_amd/csrc/conv_large.hip):
  (a) AlexNet conv1 at full size: N=128, 3 -> 96, 227 x 227, 11x11 / s4 (no dX: the input carries no gradient)
  (b) N=64, 64 -> 64, 28 x 28, 9x9 / s1 / p4
  (c) the same layer with 7x7 / p3: the kernels that were there before (LDS-DMA / register-staged), the yardstick
Device events on the library's stream, a warm-up of at least 80 ms per measurement, five repetitions; median and spread
(max - min) of the repetitions. FLOP/s are the executed 2 * N*OH*OW * F * C/g*k*k; for (a) also the fraction of the
157 TFLOP/s fp32-MFMA peak and of 8 TB/s on the algorithmic bytes (every tensor once).
    python tools/exp/large_conv_time.py
Under rocprofv3:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/exp/large_conv_time.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: one HIP runtime for torch and the library)

from bcnn_amd import _lib, ops  # noqa: E402

MFMA_PEAK = 157.3e12  # fp32 FLOP/s, MI355X
HBM_PEAK = 8.0e12     # B/s

CASES = [  # name, (n, c, h, w, f, k, s, p, g), with dX
    ("a_alexnet_conv1_11x11s4", (128, 3, 227, 227, 96, 11, 4, 0, 1), False),
    ("b_64ch_28x28_9x9", (64, 64, 28, 28, 64, 9, 1, 4, 1), True),
    ("c_64ch_28x28_7x7", (64, 64, 28, 28, 64, 7, 1, 3, 1), True),
]
REPS = 5


def measure(L, fn):
    """median and spread (ms) of REPS timed runs of fn, each the mean of a burst that lasts >= ~20 ms"""
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    t0 = time.time()
    calls = 0
    while time.time() - t0 < 0.08 or calls < 3:  # warm-up: at least 80 ms and three calls
        fn()
        L.bcnn_hip_sync()
        calls += 1
    per_call = (time.time() - t0) / calls
    burst = max(3, min(200, int(0.02 / max(per_call, 1e-6))))
    ms = []
    for _ in range(REPS):
        L.bcnn_hip_event_record(e0)
        for _ in range(burst):
            fn()
        L.bcnn_hip_event_record(e1)
        L.bcnn_hip_event_sync(e1)
        ms.append(L.bcnn_hip_event_elapsed_ms(e0, e1) / burst)
    L.bcnn_hip_event_destroy(e0)
    L.bcnn_hip_event_destroy(e1)
    ms.sort()
    return ms[len(ms) // 2], ms[-1] - ms[0]


def run_case(L, shape, with_dx):
    n, c, h, w, f, k, s, p, g = shape
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand((n, c, h, w), device=dev, generator=gen) * 2 - 1
    wt = (torch.rand((f, c // g, k, k), device=dev, generator=gen) * 2 - 1) * 0.05
    b = torch.rand(f, device=dev, generator=gen) - 0.5
    oh, ow = ops.conv_out_hw(h, w, k, s, p)
    y = torch.empty((n, f, oh, ow), device=dev)
    dy = (torch.rand(y.shape, device=dev, generator=gen) * 2 - 1) * 0.1
    dw, db = torch.zeros_like(wt), torch.zeros_like(b)
    dx = torch.empty_like(x)
    ws = torch.zeros(max(1, ops.conv_workspace_size(n, c, h, w, f, k, s, p, g)), device=dev)
    flops = 2.0 * n * oh * ow * f * (c // g) * k * k
    nbytes = 4.0 * (x.numel() + wt.numel() + y.numel())
    out = {"flops": flops, "bytes": nbytes}
    fwd = measure(L, lambda: ops.conv_forward(x, wt, b, y, k, s, p, g, 0))
    dw_only = measure(L, lambda: ops.conv_backward(x, wt, y, dy, None, dw, db, k, s, p, g, 0, ws))
    out["fwd"], out["dw"] = fwd, dw_only
    if with_dx:
        both = measure(L, lambda: ops.conv_backward(x, wt, y, dy, dx, dw, db, k, s, p, g, 0, ws))
        # dX alone: the backward call with dX minus the one without (the same dW and bias-gradient launches in both)
        out["dx"] = (both[0] - dw_only[0], both[1] + dw_only[1])
    return out


def main():
    L = _lib.load()
    res = {"device": torch.cuda.get_device_name(0)}
    print("%-26s %-4s %10s %10s %10s %8s %8s" % ("case", "dir", "median ms", "spread ms", "TFLOP/s", "of MFMA", "of HBM"))
    for name, shape, with_dx in CASES:
        r = run_case(L, shape, with_dx)
        res[name] = {}
        for d in ("fwd", "dx", "dw"):
            if d not in r:
                continue
            med, spread = r[d]
            tf = r["flops"] / (med * 1e-3) / 1e12
            tf_lo = r["flops"] / ((med + spread) * 1e-3) / 1e12
            hbm = r["bytes"] / (med * 1e-3) / HBM_PEAK
            res[name][d] = dict(ms=med, spread_ms=spread, tflops=tf, tflops_spread=tf - tf_lo, of_mfma_peak=tf * 1e12 / MFMA_PEAK,
                                of_hbm_peak=hbm)
            print("%-26s %-4s %10.4f %10.4f %10.2f %8.3f %8.3f" % (name, d, med, spread, tf, tf * 1e12 / MFMA_PEAK, hbm))
    b, c = res[CASES[1][0]], res[CASES[2][0]]
    for d in ("fwd", "dx", "dw"):
        bar = c[d]["tflops"] - c[d]["tflops_spread"]
        print("bar %-3s: (b) %.2f TFLOP/s against (c) %.2f - %.2f = %.2f: %s" % (
            d, b[d]["tflops"], c[d]["tflops"], c[d]["tflops_spread"], bar, "met" if b[d]["tflops"] >= bar else "MISSED"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
