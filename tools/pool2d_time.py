#!/usr/bin/env python
"""Time per call of the pool2d kernels (bcnn_amd/csrc/pool2d.hip) at the shapes real nets use,
forward and overwrite backward, between device events, with the algorithmic bytes each call has to move:

  stem_pool2d    (128, 64, 112, 112)  max 3x3 / s2 / p1      the torchvision / Caffe ResNet stem pool
  stem_maxpool   (128, 64, 112, 112)  the existing unfused bcnn_hip_maxpool_forward / _backward, 3x3 / s2 / SAME: the same
                                      output extent and the same bytes, the yardstick of the leg above
  dense_avg      (128, 256, 56, 56)   average 2x2 / s2         a DenseNet transition
  spp5 / 9 / 13  (128, 512, 13, 13)   max 5, 9, 13 / s1 / centred   the SPP block of YOLOv3-SPP / YOLOv4

bytes: forward x + y (+ indexes), backward dy (+ indexes) + dx (the overwrite form reads no dx). GB/s = bytes / time;
the SPP tensors (44 MB) fit the 256 MB last-level cache, so their rate is not an HBM rate.

Every leg runs in a process of its own, the legs alternate and each is repeated --repeats times; a measurement warms up
for at least 80 ms and 3 calls, then times --iters calls between two device events. A leg that finds no device fails.

    python tools/pool2d_time.py [--out profiles/pool2d.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08

# leg -> (n, c, h, w), kind, size, stride, pad
LEGS = {
    "stem_pool2d": ((128, 64, 112, 112), "max", 3, 2, 1),
    "stem_maxpool": ((128, 64, 112, 112), "maxpool", 3, 2, 0),
    "dense_avg": ((128, 256, 56, 56), "avg", 2, 2, 0),
    "spp5": ((128, 512, 13, 13), "max", 5, 1, 2),
    "spp9": ((128, 512, 13, 13), "max", 9, 1, 4),
    "spp13": ((128, 512, 13, 13), "max", 13, 1, 6),
}


def _leg(name, iters):
    sys.path.insert(0, ROOT)
    import ctypes
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    shape, kind, k, s, p = LEGS[name]
    n, c, h, w = shape
    if kind == "maxpool":
        oh, ow = (h + s - 1) // s, (w + s - 1) // s   # BCNN_PADDING_SAME
    else:
        oh, ow = ops.pool2d_out_hw(kind, h, w, k, s, p)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(shape, generator=gen).to("cuda:0")
    dy = torch.randn((n, c, oh, ow), generator=gen).to("cuda:0")
    y = torch.empty((n, c, oh, ow), device="cuda:0")
    dx = torch.empty(shape, device="cuda:0")
    idx = torch.empty((n, c, oh, ow), dtype=torch.int32, device="cuda:0") if kind != "avg" else None
    if kind == "maxpool":
        fwd = lambda: ops.maxpool_forward(x, y, idx, k, s)
        bwd = lambda: ops.maxpool_backward(dy, idx, dx, k, s, overwrite=True)
    else:
        fwd = lambda: ops.pool2d_forward(x, y, idx, kind, k, s, p)
        bwd = lambda: ops.pool2d_backward(dy, idx, dx, kind, k, s, p, overwrite=True)
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()

    def timed(fn):
        t0, warm = time.perf_counter(), 0
        while warm < 3 or time.perf_counter() - t0 < MIN_WARM_S:
            fn()
            L.bcnn_hip_sync()
            warm += 1
        L.bcnn_hip_event_record(e0)
        for _ in range(iters):
            fn()
        L.bcnn_hip_event_record(e1)
        L.bcnn_hip_event_sync(e1)
        return L.bcnn_hip_event_elapsed_ms(e0, e1) / iters

    L.bcnn_hip_trace_enable(1)
    fwd()
    bwd()
    L.bcnn_hip_sync()
    tl = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(tl + 1)
    L.bcnn_hip_trace_read(buf, tl + 1)
    L.bcnn_hip_trace_enable(0)
    in_b, out_b = 4.0 * n * c * h * w, 4.0 * n * c * oh * ow
    has_idx = 1 if idx is not None else 0
    fwd_bytes, bwd_bytes = in_b + (1 + has_idx) * out_b, (1 + has_idx) * out_b + in_b
    fwd_ms, bwd_ms = timed(fwd), timed(bwd)
    print(json.dumps({"leg": name, "shape": list(shape), "out": [oh, ow], "kind": kind, "size": k, "stride": s, "pad": p,
                      "kernels": buf.value.decode().split(), "iters": iters,
                      "fwd_ms": fwd_ms, "fwd_bytes": fwd_bytes, "fwd_gbs": fwd_bytes / fwd_ms * 1e-6,
                      "bwd_ms": bwd_ms, "bwd_bytes": bwd_bytes, "bwd_gbs": bwd_bytes / bwd_ms * 1e-6}))


def _child(name, iters):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--iters", str(iters)],
                       capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("leg %s failed (%d):\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the raw record as JSON here")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        _leg(a.leg, a.iters)
        return
    runs = []
    for rep in range(a.repeats):   # alternating: every leg once per round
        for name in LEGS:
            r = _child(name, a.iters)
            r["repeat"] = rep
            runs.append(r)
            print("%-13s rep %d  fwd %7.3f ms %7.1f GB/s   bwd %7.3f ms %7.1f GB/s   %s" % (
                name, rep, r["fwd_ms"], r["fwd_gbs"], r["bwd_ms"], r["bwd_gbs"], " ".join(r["kernels"])), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {}
    for name in LEGS:
        mine = [r for r in runs if r["leg"] == name]
        summary[name] = {k: med([r[k] for r in mine]) for k in ("fwd_ms", "fwd_gbs", "bwd_ms", "bwd_gbs")}
        summary[name]["fwd_ms_spread"] = [min(r["fwd_ms"] for r in mine), max(r["fwd_ms"] for r in mine)]
        summary[name]["bwd_ms_spread"] = [min(r["bwd_ms"] for r in mine), max(r["bwd_ms"] for r in mine)]
    new, old = summary["stem_pool2d"], summary["stem_maxpool"]
    summary["stem_ratio_new_over_old"] = {"fwd": new["fwd_ms"] / old["fwd_ms"], "bwd": new["bwd_ms"] / old["bwd_ms"],
                                          "fwd_plus_bwd": (new["fwd_ms"] + new["bwd_ms"]) / (old["fwd_ms"] + old["bwd_ms"])}
    result = {"tool": "tools/pool2d_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary, "runs": runs}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
