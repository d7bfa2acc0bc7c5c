#!/usr/bin/env python
"""Time per call of the self-gated activation kernels (bcnn_amd/csrc/activation.hip) and the scale-channels kernels
(bcnn_amd/csrc/scale_channels.hip) at a MobileNetV3-class squeeze-and-excitation shape,
(64, 72, 56, 56), between device events, with the algorithmic bytes each call has to move:

  keep_<act>   bcnn_hip_activation_forward_keep          x read, x_saved and y written           12 bytes / element
  back_<act>   bcnn_hip_activation_backward_from_input   x_saved and dy read, dx written         12 bytes / element
  scale_fwd    bcnn_hip_scale_channels_forward           x read, y written (+ N C gates)          8 bytes / element
  scale_bwd    bcnn_hip_scale_channels_backward          x, dy, dx read, dx written (+ gates)    16 bytes / element

GB/s = bytes / time. One tensor is 58 MB, so the two or three tensors of a call fit the 256 MB last-level cache when the
same call repeats: the rate of a repeated call is not an HBM rate, and bytes / 8 TB/s is the floor a cold call has.

Every leg runs in a process of its own, the legs alternate and each is repeated --repeats times; a measurement warms up for
at least 80 ms and 3 calls, then times --iters calls between two device events. A leg that finds no device fails.

    python tools/gated_se_time.py [--out profiles/gated_se.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
SHAPE = (64, 72, 56, 56)
ACTS = ("hard_swish", "swish", "mish")
LEGS = ["keep_" + a for a in ACTS] + ["back_" + a for a in ACTS] + ["scale_fwd", "scale_bwd"]


def _leg(name, iters):
    sys.path.insert(0, ROOT)
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    n, c, h, w = SHAPE
    elems = n * c * h * w
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(SHAPE, generator=gen).to("cuda:0")
    dy = torch.randn(SHAPE, generator=gen).to("cuda:0")
    if name.startswith("keep_"):
        act, saved = ops.ACT_ALL[name[5:]], torch.empty_like(x)
        fn, per_elem = (lambda: ops.activation_forward_keep(x, saved, act)), 12   # in place: x drifts, the time does not
    elif name.startswith("back_"):
        act = ops.ACT_ALL[name[5:]]
        fn, per_elem = (lambda: ops.activation_backward_from_input(x, dy, act)), 12
    else:
        gate = torch.rand((n, c, 1, 1), generator=gen).to("cuda:0")
        y, dgate = torch.empty_like(x), torch.zeros((n, c, 1, 1), device="cuda:0")
        if name == "scale_fwd":
            fn, per_elem = (lambda: ops.scale_channels_forward(x, gate, y)), 8
        else:
            fn, per_elem = (lambda: ops.scale_channels_backward(x, gate, dy, y, dgate)), 16
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
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
    ms = L.bcnn_hip_event_elapsed_ms(e0, e1) / iters
    nbytes = float(per_elem) * elems
    print(json.dumps({"leg": name, "shape": list(SHAPE), "iters": iters, "ms": ms, "bytes": nbytes,
                      "gbs": nbytes / ms * 1e-6, "floor_ms_at_8TBs": nbytes / 8e12 * 1e3}))


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
            print("%-16s rep %d  %7.4f ms %7.1f GB/s   (floor at 8 TB/s %6.4f ms)" % (name, rep, r["ms"], r["gbs"],
                                                                                     r["floor_ms_at_8TBs"]), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {}
    for name in LEGS:
        mine = [r for r in runs if r["leg"] == name]
        summary[name] = {"ms": med([r["ms"] for r in mine]), "gbs": med([r["gbs"] for r in mine]),
                         "ms_spread": [min(r["ms"] for r in mine), max(r["ms"] for r in mine)],
                         "floor_ms_at_8TBs": mine[0]["floor_ms_at_8TBs"]}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/gated_se_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary,
                       "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
