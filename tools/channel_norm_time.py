#!/usr/bin/env python
"""Time per call of the channel-norm kernels (bcnn_amd/csrc/channel_norm.hip) on their three paths,
between device events, next to torch-ROCm's own layer norm on the permuted ([N,H,W,C], contiguous) tensor in the same process:

  shape  N    C    H x W     path (forward / backward)
  mvit   32   144  16 x 16   resident / stream    a MobileViT stage
  detr   2    256  25 x 34   stream               a DETR encoder layer
  cnx1   32   96   56 x 56   resident / stream    ConvNeXt stage 1
  cnx4   32   768  7 x 7     stream               ConvNeXt stage 4 (three passes of per-channel sums in the backward)
  c8     32   8    28 x 28   column               either side of the backward's column limit
  c9     32   9    28 x 28   column / stream
  c16    32   16   28 x 28   column / stream      either side of the forward's column limit
  c17    32   17   28 x 28   resident / stream
  f238   32   238  28 x 28   resident / stream    either side of the forward's resident limit
  f239   32   239  28 x 28   stream

  ours_fwd   bcnn_hip_channel_norm_forward, mean and rstd stored       8 bytes / element (stream: the second sweep re-reads x,
  ours_bwd   bcnn_hip_channel_norm_backward, overwrite, all gradients  12 bytes / element  expected from cache, not counted)
  torch_fwd  aten.native_layer_norm on the permuted tensor             (a yardstick printed next to ours: no test or
  torch_bwd  aten.native_layer_norm_backward, all three gradients       threshold depends on it)

floor = bytes / 8 TB/s, what a cold call has to take. A repeated call whose tensors fit the 256 MB last-level cache is not
running at an HBM rate: the record says which working sets fit.

Every (shape, leg, repeat) runs in a fresh process; the leg warms up for at least 80 ms and 3 calls, then times --iters calls
between two device events. The summary is the median over the processes, with
the spread. A process that finds no device fails.

    python tools/channel_norm_time.py [--out profiles/channel_norm.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
SHAPES = {"mvit": (32, 144, 16, 16), "detr": (2, 256, 25, 34), "cnx1": (32, 96, 56, 56), "cnx4": (32, 768, 7, 7),
          "c8": (32, 8, 28, 28), "c9": (32, 9, 28, 28), "c16": (32, 16, 28, 28), "c17": (32, 17, 28, 28),
          "f238": (32, 238, 28, 28), "f239": (32, 239, 28, 28)}
LEGS = ("ours_fwd", "ours_bwd", "torch_fwd", "torch_bwd")
LLC_BYTES = 256e6


def _shape(name, leg, iters):
    sys.path.insert(0, ROOT)
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    n, c, h, w = SHAPES[name]
    elems = n * c * h * w
    gen = torch.Generator().manual_seed(1)
    dev = "cuda:0"
    x = (torch.randn((n, c, h, w), generator=gen) + 0.5).to(dev)
    dy = torch.randn((n, c, h, w), generator=gen).to(dev)
    scales, b = (torch.rand(c, generator=gen) + 0.5).to(dev), torch.randn(c, generator=gen).to(dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(n * h * w, device=dev), torch.empty(n * h * w, device=dev)
    dscales, db = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
    ops.channel_norm_forward(x, scales, b, y, mean, rstd, 1e-5)
    xt, dyt = x.permute(0, 2, 3, 1).contiguous(), dy.permute(0, 2, 3, 1).contiguous()   # torch's layout: channels last
    aten = torch.ops.aten
    fns = {
        "ours_fwd": (lambda: ops.channel_norm_forward(x, scales, b, y, mean, rstd, 1e-5), 8),
        "ours_bwd": (lambda: ops.channel_norm_backward(x, scales, mean, rstd, dy, dx, dscales, db, True), 12),
        "torch_fwd": (lambda: aten.native_layer_norm(xt, [c], scales, b, 1e-5), 8),
        "torch_bwd": (lambda: aten.native_layer_norm_backward(dyt, xt, [c], mean.view(n, h, w, 1), rstd.view(n, h, w, 1),
                                                              scales, b, [True, True, True]), 12),
    }
    paths = {"ours_fwd": ops.CHANNEL_NORM_PATHS[ops.channel_norm_path(n, c, h * w, False)],
             "ours_bwd": ops.CHANNEL_NORM_PATHS[ops.channel_norm_path(n, c, h * w, True)]}
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    fn, per_elem = fns[leg]
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
    print(json.dumps({"shape": name, "dims": list(SHAPES[name]), "leg": leg, "path": paths.get(leg), "iters": iters,
                      "ms": ms, "bytes": nbytes, "gbs": nbytes / ms * 1e-6, "floor_ms_at_8TBs": nbytes / 8e12 * 1e3,
                      "fits_llc": nbytes <= LLC_BYTES}), flush=True)


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
    for rep in range(a.repeats):   # alternating: every shape once per round
        for name, leg in ((n, l) for n in SHAPES for l in LEGS):
            for r in _child(name, leg, a.iters):
                r["repeat"] = rep
                runs.append(r)
                print("%-5s %-10s %-9s rep %d  %8.4f ms %7.1f GB/s   (floor at 8 TB/s %7.4f ms)" % (
                    name, r["leg"], r["path"] or "", rep, r["ms"], r["gbs"], r["floor_ms_at_8TBs"]), flush=True)
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
            json.dump({"tool": "tools/channel_norm_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary,
                       "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
