#!/usr/bin/env python
"""Time of bcnn_hip_label_maps_batch (bcnn_amd/csrc/label_map.hip) next to the route the library
offered before it for the same result. fp32 tensors of standard-normal values, STRETCH, align_corners = 1:

  case       tensor (N, C, H, W)    images
  voc_head   (8, 21, 65, 65)        eight images around 500 x 375 of differing sizes (a DeepLab head back to the images)
  voc_full   (8, 21, 513, 513)      the same images (a full-resolution head: downsampling)
  ade_head   (8, 150, 65, 65)       eight images of 512 x 512

  kernel         the label-map kernel alone, between two device events inside the call (bcnn_hip_label_maps_kernel_ms)
  call           the whole call, wall clock: staging, copy in, kernel, copy back of the bytes, rows to the caller's buffers
  eval_kernel    the kernel of the evaluating form (truth maps of the images' sizes, counts)
  eval_call      the whole evaluating call, labels and counts, wall clock
  parent_route   what the same result cost without this entry point, wall clock: per image bcnn_hip_interp_forward of
                 its batch entry to the image's size, a device-to-host copy of the C x h x w floats, numpy argmax over the
                 classes as uint8
  interp_fwd     the device part of that route alone: the eight bcnn_hip_interp_forward calls between two device events

Every record carries the bytes the kernel must move at the least (the tensor's floats read once, one byte per pixel
written) and the GB/s of that figure over the kernel time; the kernel issues 16 * C gathered four-byte loads per item of
four pixels and is expected to be bound by those, not by its bytes. Every (case, repeat) runs in a fresh process that
measures the legs one after the other; a leg warms up for at least 80 ms and one call, then times --iters calls (the slow
parent route: --parent-iters). The summary is the median over the processes with the spread (min, max) and the ratios of
the parent route over the new call -- never the other way round. A process that finds no device fails.

    python tools/label_maps_time.py [--out profiles/label_maps.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
VOC_SIZES = [(500, 375), (375, 500), (500, 333), (480, 360), (500, 374), (334, 500), (500, 400), (461, 346)]
CASES = {"voc_head": ((8, 21, 65, 65), VOC_SIZES), "voc_full": ((8, 21, 513, 513), VOC_SIZES),
         "ade_head": ((8, 150, 65, 65), [(512, 512)] * 8)}
LEGS = ("kernel", "call", "eval_kernel", "eval_call", "parent_route", "interp_fwd")
ALIGN = True


def _case(name, iters, parent_iters):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    (n, c, h, w), sizes = CASES[name]
    gen = torch.Generator().manual_seed(1)
    x = torch.randn((n, c, h, w), generator=gen).to("cuda:0")
    images = [ops.label_map_fit(ops.IMAGE_FIT_STRETCH, w, h, iw, ih) for iw, ih in sizes]
    rs = np.random.RandomState(2)
    truths = [rs.randint(0, c, (ih, iw)).astype(np.uint8) for iw, ih in sizes]
    ys = [torch.empty((1, c, ih, iw), device="cuda:0") for iw, ih in sizes]
    pixels = sum(iw * ih for iw, ih in sizes)
    min_bytes = 4 * x.numel() + pixels

    def parent_route():
        out = []
        for b in range(n):
            ops.interp_forward(x[b:b + 1], ys[b], ALIGN)
            out.append(ys[b].cpu().numpy()[0].argmax(0).astype(np.uint8))
        return out

    def interp_only():
        for b in range(n):
            ops.interp_forward(x[b:b + 1], ys[b], ALIGN)

    # the two routes give the same bytes, or the comparison means nothing
    new, old = ops.label_maps(x, images, ALIGN), parent_route()
    assert all(np.array_equal(a, b) for a, b in zip(new, old)), "the routes disagree"
    L.bcnn_hip_label_maps_kernel_ms(1)
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    plain = lambda: ops.label_maps(x, images, ALIGN)                           # noqa: E731
    evalf = lambda: ops.label_maps(x, images, ALIGN, truths=truths, ignore_label=255)  # noqa: E731
    fns = {"kernel": (plain, "kernel", iters), "call": (plain, "wall", iters), "eval_kernel": (evalf, "kernel", iters),
           "eval_call": (evalf, "wall", iters), "parent_route": (parent_route, "wall", parent_iters),
           "interp_fwd": (interp_only, "events", iters)}
    for leg in LEGS:
        fn, how, reps = fns[leg]
        t0, warm = time.perf_counter(), 0
        while warm < 1 or time.perf_counter() - t0 < MIN_WARM_S:
            fn()
            L.bcnn_hip_sync()
            warm += 1
        if how == "kernel":
            times = []
            for _ in range(reps):
                fn()
                times.append(L.bcnn_hip_label_maps_kernel_ms(1))
            ms = sorted(times)[len(times) // 2]
        elif how == "events":
            L.bcnn_hip_event_record(e0)
            for _ in range(reps):
                fn()
            L.bcnn_hip_event_record(e1)
            L.bcnn_hip_event_sync(e1)
            ms = L.bcnn_hip_event_elapsed_ms(e0, e1) / reps
        else:
            L.bcnn_hip_sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            L.bcnn_hip_sync()
            ms = (time.perf_counter() - t0) * 1e3 / reps
        rec = {"case": name, "tensor": [n, c, h, w], "images": sizes, "leg": leg, "clock": how, "iters": reps, "ms": ms,
               "pixels": pixels, "min_bytes": min_bytes}
        if how == "kernel":
            rec["min_gbps"] = min_bytes / ms * 1e-6
        print(json.dumps(rec), flush=True)


def _child(name, iters, parent_iters):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--iters", str(iters), "--parent-iters",
                        str(parent_iters)], capture_output=True, text=True, cwd=ROOT, timeout=300)  # a hung child ends the run
    if r.returncode != 0:
        raise SystemExit("case %s failed (%d):\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return [json.loads(line) for line in r.stdout.strip().splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent-iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the raw record as JSON here")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        _case(a.case, a.iters, a.parent_iters)
        return
    runs = []
    for rep in range(a.repeats):   # alternating: every case once per round
        for name in CASES:
            for r in _child(name, a.iters, a.parent_iters):
                r["repeat"] = rep
                runs.append(r)
                print("%-9s %-13s rep %d  %10.4f ms  (%s)" % (name, r["leg"], rep, r["ms"], r["clock"]), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    summary = {}
    for name in CASES:
        for leg in LEGS:
            mine = [r for r in runs if r["case"] == name and r["leg"] == leg]
            s = {"tensor": mine[0]["tensor"], "pixels": mine[0]["pixels"], "clock": mine[0]["clock"],
                 "ms": med([r["ms"] for r in mine]), "ms_spread": [min(r["ms"] for r in mine), max(r["ms"] for r in mine)]}
            if "min_gbps" in mine[0]:
                s["min_bytes"] = mine[0]["min_bytes"]
                s["min_gbps"] = med([r["min_gbps"] for r in mine])
            summary[name + "_" + leg] = s
        ms = lambda leg: summary[name + "_" + leg]["ms"]   # noqa: E731
        summary[name + "_ratios"] = {"parent_route_over_call": ms("parent_route") / ms("call"),
                                     "parent_route_over_eval_call": ms("parent_route") / ms("eval_call"),
                                     "interp_fwd_over_kernel": ms("interp_fwd") / ms("kernel")}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/label_maps_time.py", "iters": a.iters, "parent_iters": a.parent_iters,
                       "repeats": a.repeats, "summary": summary, "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
