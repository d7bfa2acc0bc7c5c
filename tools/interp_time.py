#!/usr/bin/env python
"""Time per call of the bilinear interpolation kernels (bcnn_amd/csrc/interp.hip) between device
events, next to two yardsticks measured in the same process. fp32:

  case      input (N, C, H, W)     form                     output       what it is
  head      (8, 21, 65, 65)        zoom 8, align_corners    513 x 513    DeepLab's logits back to the image
  decoder   (8, 256, 33, 33)       scale 4                  132 x 132    the DeepLab v3+ decoder's first x4
  fpn       (16, 256, 32, 32)      scale 2                  64 x 64      an FPN top-down step

  interp_fwd / interp_bwd      bcnn_hip_interp_forward; _backward in its overwrite form
  nearest_fwd / nearest_bwd    bcnn_hip_upsample_forward / _backward (nearest neighbour) at the same input and integer
                               factor -- the head at 64 -> 512, scale 8: (nearly) the same bytes written and read
  memset_out / memset_in       hipMemsetAsync of the output bytes (the forward's write) and of the input-gradient bytes
                               (the backward's write), through bcnn_hip_fill_f32(.., 0)

Each record carries the trace names of one call's launches and the bytes the direction must move (x + y forward, dy + dx
backward; the yardsticks their own). Every (case, repeat) runs in a fresh process that measures the legs one after the
other; a leg warms up for at least 80 ms and 3 calls, then times --iters calls between two device events. The summary is
the median over the processes with the spread (min, max), and the two ratios interp / nearest and interp / memset. A
process that finds no device fails.

    python tools/interp_time.py [--out profiles/interp.json]
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
#         (n, c, h, w), interp form, align_corners, (nearest input extent, factor)
CASES = {"head": ((8, 21, 65, 65), dict(zoom=8), True, (64, 8)),
         "decoder": ((8, 256, 33, 33), dict(scale=4), False, (33, 4)),
         "fpn": ((16, 256, 32, 32), dict(scale=2), False, (32, 2))}
LEGS = ("interp_fwd", "interp_bwd", "nearest_fwd", "nearest_bwd", "memset_out", "memset_in")


def _case(name, iters):
    sys.path.insert(0, ROOT)
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    (n, c, h, w), form, align_corners, (nh, factor) = CASES[name]
    oh, ow = ops.interp_out_hw(h, w, **form)
    gen = torch.Generator().manual_seed(1)
    dev = "cuda:0"
    x = torch.randn((n, c, h, w), generator=gen).to(dev)
    dy = torch.randn((n, c, oh, ow), generator=gen).to(dev)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    nx = torch.randn((n, c, nh, nh), generator=gen).to(dev)
    ny = torch.randn((n, c, nh * factor, nh * factor), generator=gen).to(dev)
    ndx = torch.zeros_like(nx)
    fns = {
        "interp_fwd": (lambda: ops.interp_forward(x, y, align_corners), 4 * (x.numel() + y.numel())),
        "interp_bwd": (lambda: ops.interp_backward(dy, dx, align_corners, overwrite=True), 4 * (x.numel() + y.numel())),
        "nearest_fwd": (lambda: L.bcnn_hip_upsample_forward(nx.data_ptr(), ny.data_ptr(), n, c, nh, nh, factor),
                        4 * (nx.numel() + ny.numel())),
        # the nearest backward adds into dx: it reads dx as well
        "nearest_bwd": (lambda: L.bcnn_hip_upsample_backward(ndx.data_ptr(), ny.data_ptr(), n, c, nh, nh, factor),
                        4 * (2 * nx.numel() + ny.numel())),
        "memset_out": (lambda: L.bcnn_hip_fill_f32(y.data_ptr(), y.numel(), 0.0), 4 * y.numel()),
        "memset_in": (lambda: L.bcnn_hip_fill_f32(dx.data_ptr(), dx.numel(), 0.0), 4 * dx.numel()),
    }
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    for leg in LEGS:
        fn, nbytes = fns[leg]
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
        print(json.dumps({"case": name, "input": [n, c, h, w], "output": [oh, ow], "leg": leg,
                          "kernels": buf.value.decode().split(), "iters": iters, "ms": ms, "bytes": nbytes,
                          "gbps": nbytes / ms * 1e-6}), flush=True)


def _child(name, iters):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--iters", str(iters)],
                       capture_output=True, text=True, cwd=ROOT, timeout=180)   # a hung child ends the whole run
    if r.returncode != 0:
        raise SystemExit("case %s failed (%d):\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return [json.loads(line) for line in r.stdout.strip().splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the raw record as JSON here")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        _case(a.case, a.iters)
        return
    runs = []
    for rep in range(a.repeats):   # alternating: every case once per round
        for name in CASES:
            for r in _child(name, a.iters):
                r["repeat"] = rep
                runs.append(r)
                print("%-8s %-12s rep %d  %8.4f ms %7.0f GB/s   %s" % (name, r["leg"], rep, r["ms"], r["gbps"],
                                                                       " ".join(r["kernels"])), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    summary = {}
    for name in CASES:
        for leg in LEGS:
            mine = [r for r in runs if r["case"] == name and r["leg"] == leg]
            summary[name + "_" + leg] = {"input": mine[0]["input"], "output": mine[0]["output"], "kernels": mine[0]["kernels"],
                                         "ms": med([r["ms"] for r in mine]),
                                         "ms_spread": [min(r["ms"] for r in mine), max(r["ms"] for r in mine)],
                                         "gbps": med([r["gbps"] for r in mine])}
        for d, fill in (("fwd", "memset_out"), ("bwd", "memset_in")):
            new = summary[name + "_interp_" + d]["ms"]
            summary[name + "_" + d + "_ratios"] = {"interp_over_nearest": new / summary[name + "_nearest_" + d]["ms"],
                                                   "interp_over_memset": new / summary[name + "_" + fill]["ms"]}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/interp_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary,
                       "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
