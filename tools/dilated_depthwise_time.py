#!/usr/bin/env python
"""Time per call of the dilated depthwise kernels (bcnn_amd/csrc/depthwise_dilated.hip) between device
events, next to three yardsticks on the same tensors in the same process. N = 16, fp32, 3x3, stride 1, pad = d, ReLU:

  shape        C     H x W    d
  mnv2_576     576   33 x 33  2      (MobileNet-v2 DeepLab backbone, output stride 16)
  mnv2_960     960   33 x 33  2
  xc_384       384   65 x 65  2      (output stride 8)
  mnv2_960_os8 960   65 x 65  4
  xc_1536      1536  33 x 33  2      (Xception exit flow)
  aspp6/12/18  2048  33 x 33  6, 12, 18   (separable ASPP branches of DeepLab v3+)

  new_fwd / new_bwd    bcnn_hip_dilated_depthwise_forward; _backward with dx (assigned), dw and dbias
  gemm_fwd / gemm_bwd  bcnn_hip_dilated_conv_forward / _backward at groups = f = c: the implicit GEMM with one channel per
                       group, the only route to this layer before the depthwise family
  dense_fwd / dense_bwd  bcnn_hip_depthwise_forward / _backward at the same shape with pad = 1: what dense taps cost on the
                       tuned depthwise ladder
  floor                the bytes of the direction at SWEEP_RATE, the rate a read-and-write sweep reaches on this part
                       (tools/micro/store_floor.hip and tools/micro/stream.hip): forward x read and y
                       written, 2 N C H W 4 bytes; backward x, y, dy read and dy, dx written, five tensor passes

Each record carries the trace names of the launches of one call. Every (shape, repeat) runs in a fresh process that measures
the legs one after the other; a leg warms up for at least 80 ms and 3 calls, then times --iters calls between two device
events. The summary is the median over the processes with the spread (min, max) and the ratios of the medians. A process
that finds no device fails.

    python tools/dilated_depthwise_time.py [--out profiles/dilated_depthwise.json]
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
SWEEP_RATE = 6.3e12   # bytes/s
ACT_RELU = 2
#          n   c    h   w   k  s  p   d
SHAPES = {"mnv2_576": (16, 576, 33, 33, 3, 1, 2, 2), "mnv2_960": (16, 960, 33, 33, 3, 1, 2, 2),
          "xc_384": (16, 384, 65, 65, 3, 1, 2, 2), "mnv2_960_os8": (16, 960, 65, 65, 3, 1, 4, 4),
          "xc_1536": (16, 1536, 33, 33, 3, 1, 2, 2), "aspp6": (16, 2048, 33, 33, 3, 1, 6, 6),
          "aspp12": (16, 2048, 33, 33, 3, 1, 12, 12), "aspp18": (16, 2048, 33, 33, 3, 1, 18, 18)}
LEGS = ("new_fwd", "new_bwd", "gemm_fwd", "gemm_bwd", "dense_fwd", "dense_bwd")


def floor_ms(dims, leg):
    n, c, h, w = dims[:4]
    return (5 if leg.endswith("bwd") else 2) * n * c * h * w * 4 / SWEEP_RATE * 1e3


def _shape(name, iters):
    sys.path.insert(0, ROOT)
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    n, c, h, w, k, s, p, d = SHAPES[name]
    assert ops.dilated_conv_out_hw(h, w, k, s, p, d) == (h, w) == ops.conv_out_hw(h, w, k, s, 1)
    gen = torch.Generator().manual_seed(1)
    dev = "cuda:0"
    x = torch.randn((n, c, h, w), generator=gen).to(dev)
    wt = (torch.randn((c, 1, k, k), generator=gen) * 0.3).to(dev)
    b = torch.randn(c, generator=gen).to(dev)
    dy0 = torch.randn((n, c, h, w), generator=gen).to(dev)
    y, dy, dx, dw, db = torch.empty_like(x), dy0.clone(), torch.empty_like(x), torch.zeros_like(wt), torch.zeros_like(b)
    ws = torch.zeros(ops.dilated_depthwise_workspace_size(n, c, h, w, k, s, p, d), device=dev)
    wsg = torch.zeros(max(ops.dilated_conv_workspace_size(n, c, h, w, c, k, s, p, d, c), 1), device=dev)
    fns = {
        "new_fwd": lambda: ops.dilated_depthwise_forward(x, wt, b, y, k, s, p, d, ACT_RELU),
        "new_bwd": lambda: ops.dilated_depthwise_backward(x, wt, y, dy, dx, dw, db, k, s, p, d, ACT_RELU, True, ws),
        "gemm_fwd": lambda: ops.dilated_conv_forward(x, wt, b, y, k, s, p, d, c, ACT_RELU),
        "gemm_bwd": lambda: ops.dilated_conv_backward(x, wt, y, dy, dx, dw, db, k, s, p, d, c, ACT_RELU, wsg),
        "dense_fwd": lambda: ops.depthwise_forward(x, wt, b, y, k, s, 1, ACT_RELU),
        "dense_bwd": lambda: ops.depthwise_backward(x, wt, y, dy, dx, dw, db, k, s, 1, ACT_RELU, overwrite=True),
    }
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    for leg in LEGS:
        fn = fns[leg]
        if leg.endswith("bwd"):   # every backward leg works on the y of its own forward and a fresh dy
            fns[leg[:-3] + "fwd"]()
            dy.copy_(dy0)
            dw.zero_()
            db.zero_()
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
        print(json.dumps({"shape": name, "dims": list(SHAPES[name]), "leg": leg, "kernels": buf.value.decode().split(),
                          "iters": iters, "warm_calls": warm, "ms": ms, "floor_ms": floor_ms(SHAPES[name], leg)}), flush=True)


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
                print("%-13s %-10s rep %d  %8.4f ms (floor %.4f)   %s" % (name, r["leg"], rep, r["ms"], r["floor_ms"],
                                                                          " ".join(r["kernels"])), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    summary = {}
    for name in SHAPES:
        for leg in LEGS:
            mine = [r for r in runs if r["shape"] == name and r["leg"] == leg]
            summary[name + "_" + leg] = {"dims": mine[0]["dims"], "kernels": mine[0]["kernels"],
                                         "ms": med([r["ms"] for r in mine]),
                                         "ms_spread": [min(r["ms"] for r in mine), max(r["ms"] for r in mine)],
                                         "floor_ms": mine[0]["floor_ms"]}
        for way in ("fwd", "bwd"):
            new = summary[name + "_new_" + way]
            new["gemm_over_new"] = summary[name + "_gemm_" + way]["ms"] / new["ms"]
            new["new_over_dense"] = new["ms"] / summary[name + "_dense_" + way]["ms"]
            new["new_over_floor"] = new["ms"] / new["floor_ms"]
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/dilated_depthwise_time.py", "iters": a.iters, "repeats": a.repeats,
                       "sweep_rate": SWEEP_RATE, "summary": summary, "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
