#!/usr/bin/env python
"""Time per call of the patch-merging kernels (bcnn_amd/csrc/patch_merge.hip) between device events,
next to the two routes the fused node replaces:

  shape  N    C    H x W       path     4C
  swin1  64   96   56 x 56     split    384    Swin-T stage 1 -> 2
  swin2  64   192  28 x 28     split    768    stage 2 -> 3
  swin3  64   384  14 x 14     stream   1536   stage 3 -> 4
  focus  16   3    640 x 640   column   12     YOLOv5's Focus with a norm behind it

  fused_fwd / fused_bwd   bcnn_hip_patch_merge_forward / _backward with the norm, all gradients (overwrite)
  split_fwd / split_bwd   this build's own norm = 0 launch followed by the channel-norm kernels on the rearranged tensor
                          (backward: channel-norm backward, then the norm = 0 backward): what the fusion replaces
  torch_fwd / torch_bwd   torch-ROCm: cat of the four strided views of the [N,H,W,C] tensor + aten.native_layer_norm, and
                          autograd through the same (a yardstick printed next to ours: no test or threshold depends on it)

bytes: what each route has to move at least, in floats of 4 bytes per element of the source: fused forward 2 (read x, write
y), fused backward 3 (x, dy, dx); the split route 4 (x, r, r, y) and 5 (r, dy, dr, dr, dx); torch as the split route. floor =
bytes / 8 TB/s. A repeated call whose tensors fit the 256 MB last-level cache is not running at an HBM rate: the record says
which working sets fit.

Every (shape, leg, repeat) runs in a fresh process; the leg warms up for at least 80 ms and 3 calls, then times --iters calls
between two device events. The summary is the median over the processes, with the spread. A process that finds no device fails.

    python tools/patch_merge_time.py [--out profiles/patch_merge.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
SHAPES = {"swin1": (64, 96, 56, 56), "swin2": (64, 192, 28, 28), "swin3": (64, 384, 14, 14), "focus": (16, 3, 640, 640)}
LEGS = {"fused_fwd": 2, "fused_bwd": 3, "split_fwd": 4, "split_bwd": 5, "torch_fwd": 4, "torch_bwd": 5}   # floats / element
LLC_BYTES = 256e6


def _shape(name, leg, iters):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    n, c, h, w = SHAPES[name]
    out, rows = (n, 4 * c, h // 2, w // 2), n * (h // 2) * (w // 2)
    gen, dev = torch.Generator().manual_seed(1), "cuda:0"
    x = (torch.randn((n, c, h, w), generator=gen) + 0.5).to(dev)
    dy = torch.randn(out, generator=gen).to(dev)
    scales, b = (torch.rand(4 * c, generator=gen) + 0.5).to(dev), torch.randn(4 * c, generator=gen).to(dev)
    y, r, dr, dx = torch.empty(out, device=dev), torch.empty(out, device=dev), torch.empty(out, device=dev), torch.empty_like(x)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    dscales, db = torch.zeros(4 * c, device=dev), torch.zeros(4 * c, device=dev)
    ops.patch_merge_forward(x, scales, b, y, mean, rstd, 1e-5)
    ops.patch_merge_forward(x, None, None, r, None, None)

    def split_fwd():
        ops.patch_merge_forward(x, None, None, r, None, None)
        ops.channel_norm_forward(r, scales, b, y, mean, rstd, 1e-5)

    def split_bwd():
        ops.channel_norm_backward(r, scales, mean, rstd, dy, dr, dscales, db, True)
        ops.patch_merge_backward(None, None, None, None, dr, dx, None, None, True)

    xt = x.permute(0, 2, 3, 1).contiguous().requires_grad_(True)   # torch's (and Swin's) layout: channels last
    dyt = dy.permute(0, 2, 3, 1).contiguous()

    def torch_fwd():
        m = torch.cat([xt[:, 0::2, 0::2], xt[:, 1::2, 0::2], xt[:, 0::2, 1::2], xt[:, 1::2, 1::2]], -1)
        return F.layer_norm(m, (4 * c,), scales, b, 1e-5)

    graph = torch_fwd()

    def torch_bwd():
        torch.autograd.grad(graph, xt, dyt, retain_graph=True)

    fns = {"fused_fwd": lambda: ops.patch_merge_forward(x, scales, b, y, mean, rstd, 1e-5),
           "fused_bwd": lambda: ops.patch_merge_backward(x, scales, mean, rstd, dy, dx, dscales, db, True),
           "split_fwd": split_fwd, "split_bwd": split_bwd, "torch_fwd": torch_fwd, "torch_bwd": torch_bwd}
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    fn = fns[leg]
    t0, warm = time.perf_counter(), 0
    while warm < 3 or time.perf_counter() - t0 < MIN_WARM_S:
        fn()
        torch.cuda.synchronize()
        L.bcnn_hip_sync()
        warm += 1
    L.bcnn_hip_event_record(e0)
    for _ in range(iters):
        fn()
    L.bcnn_hip_event_record(e1)
    L.bcnn_hip_event_sync(e1)
    ms = L.bcnn_hip_event_elapsed_ms(e0, e1) / iters
    nbytes = 4.0 * LEGS[leg] * n * c * h * w
    print(json.dumps({"shape": name, "dims": list(SHAPES[name]), "leg": leg, "path": ops.PATCH_MERGE_PATHS[ops.patch_merge_path(n, c, h, w)],
                      "iters": iters, "ms": ms, "bytes": nbytes, "gbs": nbytes / ms * 1e-6,
                      "floor_ms_at_8TBs": nbytes / 8e12 * 1e3, "fits_llc": nbytes <= LLC_BYTES}), flush=True)


def _child(name, leg, iters):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name + ":" + leg, "--iters", str(iters)],
                       capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("shape %s failed (%d):\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return [json.loads(line) for line in r.stdout.strip().splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the raw record as JSON here")
    ap.add_argument("--shape", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.shape:
        _shape(*a.shape.split(":"), a.iters)
        return
    runs = []
    for rep in range(a.repeats):   # alternating: every shape and leg once per round
        for name, leg in ((n, l) for n in SHAPES for l in LEGS):
            for r in _child(name, leg, a.iters):
                r["repeat"] = rep
                runs.append(r)
                print("%-5s %-10s %-7s rep %d  %8.4f ms %7.1f GB/s   (floor at 8 TB/s %7.4f ms)" % (
                    name, r["leg"], r["path"], rep, r["ms"], r["gbs"], r["floor_ms_at_8TBs"]), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {}
    for name in SHAPES:
        for leg in LEGS:
            mine = [r for r in runs if r["shape"] == name and r["leg"] == leg]
            summary[name + "_" + leg] = {"dims": mine[0]["dims"], "path": mine[0]["path"], "ms": med([r["ms"] for r in mine]),
                                         "gbs": med([r["gbs"] for r in mine]),
                                         "ms_spread": [min(r["ms"] for r in mine), max(r["ms"] for r in mine)],
                                         "floor_ms_at_8TBs": mine[0]["floor_ms_at_8TBs"], "fits_llc": mine[0]["fits_llc"]}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/patch_merge_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary,
                       "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
