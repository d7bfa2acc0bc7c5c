#!/usr/bin/env python
"""Time per call of the dilated-convolution kernels (bcnn_amd/csrc/conv_dilated.hip) between device
events, next to two yardsticks measured in the same process on the same tensors. N = 16, fp32, 3x3, stride 1:

  shape    C -> F      H x W    d = p
  aspp6    512 -> 256  33 x 33  6      (DeepLab ASPP branches)
  aspp12   512 -> 256  33 x 33  12
  aspp18   512 -> 256  33 x 33  18
  res2     512 -> 512  28 x 28  2      (a dilated ResNet stage)

  new_fwd / new_dx / new_dw      bcnn_hip_dilated_conv_forward; _backward with only dx; with only dw (no bias gradient)
  d1_fwd / d1_dx / d1_dw         the same entry points at d = 1, p = 1 (same output extent, every tap dense)
  conv_fwd                       bcnn_hip_conv_forward at d = 1, p = 1: what the convolution node's ladder picks
  conv_bwd / conv_bwd_nodx       bcnn_hip_conv_backward with and without the data gradient (its difference is the dX kernel)

Each record carries the trace names of the launches of one call (the family the ladder picked for the yardsticks), the
nominal 2 N OH OW F C k^2 operations of the direction (conv_bwd: twice that), and their share of the 157 TFLOP/s
fp32-MFMA peak DESIGN.md uses. Nominal: taps that fall into the padding are counted although they multiply zeros, which at
d = 18 on a 33 x 33 plane is most of the eight outer taps.

Every (shape, repeat) runs in a fresh process that measures the legs one after the other; a leg warms up for at least 80 ms
and 3 calls, then times --iters calls between two device events. The summary is the median over the processes with the
spread (min, max). A process that finds no device fails.

    python tools/dilated_conv_time.py [--out profiles/dilated_conv.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
PEAK_FLOPS = 157e12
#          n   c    h   w   f    k  s  p   d
SHAPES = {"aspp6": (16, 512, 33, 33, 256, 3, 1, 6, 6), "aspp12": (16, 512, 33, 33, 256, 3, 1, 12, 12),
          "aspp18": (16, 512, 33, 33, 256, 3, 1, 18, 18), "res2": (16, 512, 28, 28, 512, 3, 1, 2, 2)}
LEGS = ("new_fwd", "new_dx", "new_dw", "d1_fwd", "d1_dx", "d1_dw", "conv_fwd", "conv_bwd", "conv_bwd_nodx")


def _shape(name, iters):
    sys.path.insert(0, ROOT)
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    n, c, h, w, f, k, s, p, d = SHAPES[name]
    oh, ow = ops.dilated_conv_out_hw(h, w, k, s, p, d)
    assert (oh, ow) == ops.dilated_conv_out_hw(h, w, k, s, 1, 1) == ops.conv_out_hw(h, w, k, s, 1)
    gen = torch.Generator().manual_seed(1)
    dev = "cuda:0"
    x = torch.randn((n, c, h, w), generator=gen).to(dev)
    wt = (torch.randn((f, c, k, k), generator=gen) * 0.02).to(dev)
    b = torch.randn(f, generator=gen).to(dev)
    dy = torch.randn((n, f, oh, ow), generator=gen).to(dev)
    y, dx, dw, db = torch.empty_like(dy), torch.empty_like(x), torch.zeros_like(wt), torch.zeros_like(b)
    ws = torch.zeros(max(ops.dilated_conv_workspace_size(n, c, h, w, f, k, s, p, d, 1),
                         ops.dilated_conv_workspace_size(n, c, h, w, f, k, s, 1, 1, 1),
                         ops.conv_workspace_size(n, c, h, w, f, k, s, 1, 1), 1), device=dev)
    ops.dilated_conv_forward(x, wt, b, y, k, s, p, d, 1, 0)
    fns = {
        "new_fwd": lambda: ops.dilated_conv_forward(x, wt, b, y, k, s, p, d, 1, 0),
        "new_dx": lambda: ops.dilated_conv_backward(x, wt, y, dy, dx, None, None, k, s, p, d, 1, 0, ws),
        "new_dw": lambda: ops.dilated_conv_backward(x, wt, y, dy, None, dw, None, k, s, p, d, 1, 0, ws),
        "d1_fwd": lambda: ops.dilated_conv_forward(x, wt, b, y, k, s, 1, 1, 1, 0),
        "d1_dx": lambda: ops.dilated_conv_backward(x, wt, y, dy, dx, None, None, k, s, 1, 1, 1, 0, ws),
        "d1_dw": lambda: ops.dilated_conv_backward(x, wt, y, dy, None, dw, None, k, s, 1, 1, 1, 0, ws),
        "conv_fwd": lambda: ops.conv_forward(x, wt, b, y, k, s, 1, 1, 0),
        "conv_bwd": lambda: ops.conv_backward(x, wt, y, dy, dx, dw, db, k, s, 1, 1, 0, ws),
        "conv_bwd_nodx": lambda: ops.conv_backward(x, wt, y, dy, None, dw, db, k, s, 1, 1, 0, ws),
    }
    flops = 2.0 * n * oh * ow * f * c * k * k
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    for leg in LEGS:
        fn = fns[leg]
        t0, warm = time.perf_counter(), 0
        while warm < 3 or time.perf_counter() - t0 < MIN_WARM_S:
            fn()
            L.bcnn_hip_sync()
            warm += 1
        L.bcnn_hip_trace_enable(1)
        fn()
        L.bcnn_hip_sync()
        size = L.bcnn_hip_trace_read(None, 0)
        buf = ctypes.create_string_buffer(size + 1)
        L.bcnn_hip_trace_read(buf, size + 1)
        L.bcnn_hip_trace_enable(0)
        L.bcnn_hip_event_record(e0)
        for _ in range(iters):
            fn()
        L.bcnn_hip_event_record(e1)
        L.bcnn_hip_event_sync(e1)
        ms = L.bcnn_hip_event_elapsed_ms(e0, e1) / iters
        ops_leg = flops * (2 if leg == "conv_bwd" else 1)
        print(json.dumps({"shape": name, "dims": list(SHAPES[name]), "leg": leg, "kernels": buf.value.decode().split(),
                          "iters": iters, "ms": ms, "flops": ops_leg, "tflops": ops_leg / ms * 1e-9,
                          "share_of_peak": ops_leg / (ms * 1e-3) / PEAK_FLOPS}), flush=True)


def _child(name, iters):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--iters", str(iters)],
                       capture_output=True, text=True, cwd=ROOT, timeout=180)   # a hung child ends the whole run
    if r.returncode != 0:
        raise SystemExit("shape %s failed (%d):\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return [json.loads(line) for line in r.stdout.strip().splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the raw record as JSON here")
    ap.add_argument("--shape", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.shape:
        _shape(a.shape, a.iters)
        return
    runs = []
    for rep in range(a.repeats):   # alternating: every shape once per round
        for name in SHAPES:
            for r in _child(name, a.iters):
                r["repeat"] = rep
                runs.append(r)
                print("%-7s %-14s rep %d  %8.4f ms %6.1f TFLOP/s %5.1f %% of peak   %s" % (
                    name, r["leg"], rep, r["ms"], r["tflops"], 100 * r["share_of_peak"], " ".join(r["kernels"])), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    summary = {}
    for name in SHAPES:
        for leg in LEGS:
            mine = [r for r in runs if r["shape"] == name and r["leg"] == leg]
            summary[name + "_" + leg] = {"dims": mine[0]["dims"], "kernels": mine[0]["kernels"],
                                         "ms": med([r["ms"] for r in mine]),
                                         "ms_spread": [min(r["ms"] for r in mine), max(r["ms"] for r in mine)],
                                         "tflops": med([r["tflops"] for r in mine]),
                                         "share_of_peak": med([r["share_of_peak"] for r in mine])}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/dilated_conv_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary,
                       "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
