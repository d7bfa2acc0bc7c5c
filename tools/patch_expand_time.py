#!/usr/bin/env python
"""Time per call of the patch-expanding kernels (bcnn_amd/csrc/patch_expand.hip) between device events:

  shape  N    c_in      H x W      block  order     norm  c    out           path
  up2    32   4 x 96    28 x 28    2      blocks    yes   96   96 x 56 x 56   split    Swin-UNet's PatchExpand
  up4    32   16 x 96   56 x 56    4      blocks    yes   96   96 x 224 x 224 split    Swin-UNet's FinalPatchExpand_X4
  pshuf  64   4 x 64    64 x 64    2      channels  no    64   64 x 128 x 128 copy     a sub-pixel convolution head

  fwd / bwd               bcnn_hip_patch_expand_forward / _backward, with the norm all gradients (overwrite)
  torch_fwd / torch_bwd   torch-ROCm: pixel_shuffle (on the channels permuted to its order where the shape's is `blocks`,
                          done once outside the timed region) followed by layer_norm over the channels of the NHWC view, and
                          autograd through the same (a yardstick printed next to ours: no test or threshold depends on it)

bytes: what the node has to move at least, in floats of 4 bytes per element: forward 2 (read x, write y), backward with the
norm 3 (x, dy, dx), without 2. sweep = bytes / 6.7 TB/s, the memset-class sweep rate of DESIGN.md section 4; frac = sweep / ms.
A repeated call whose tensors fit the 256 MB last-level cache is not running at an HBM rate: the record says which fit.

Every (shape, leg, repeat) runs in a fresh process; the leg warms up for at least 80 ms and 3 calls, times --iters calls
between two device events as a pilot, and then times as many calls as fill a window of at least 0.25 s (never fewer than
--iters); the record holds that count. The summary is the median over the processes, with the spread. A process that finds no device fails.

    python tools/patch_expand_time.py [--out profiles/patch_expand.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
MIN_WINDOW_S = 0.25   # a window of a millisecond measures the clock and the scheduler as much as the kernel
# name: (N, c, H, W, block, order, norm)
SHAPES = {"up2": (32, 96, 28, 28, 2, "blocks", True), "up4": (32, 96, 56, 56, 4, "blocks", True),
          "pshuf": (64, 64, 64, 64, 2, "channels", False)}
LEGS = ("fwd", "bwd", "torch_fwd", "torch_bwd")
LLC_BYTES = 256e6
SWEEP_BYTES_PER_S = 6.7e12


def _shape(name, leg, iters):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    n, c, h, w, p, order, norm = SHAPES[name]
    src, out, rows = (n, p * p * c, h, w), (n, c, p * h, p * w), n * p * h * p * w
    gen, dev = torch.Generator().manual_seed(1), "cuda:0"
    x = (torch.randn(src, generator=gen) + 0.5).to(dev)
    dy = torch.randn(out, generator=gen).to(dev)
    scales, b = (torch.rand(c, generator=gen) + 0.5).to(dev), torch.randn(c, generator=gen).to(dev)
    y, dx = torch.empty(out, device=dev), torch.empty_like(x)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    dscales, db = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
    ops.patch_expand_forward(x, scales if norm else None, b if norm else None, y, mean if norm else None, rstd if norm else None, p, order)
    xt = x if order == "channels" else x.reshape(n, p * p, c, h, w).transpose(1, 2).reshape(src).contiguous()
    xt.requires_grad_(True)
    st, bt = scales.clone().requires_grad_(True), b.clone().requires_grad_(True)
    wrt = [xt, st, bt] if norm else [xt]

    def torch_fwd():
        r = F.pixel_shuffle(xt, p)
        return F.layer_norm(r.permute(0, 2, 3, 1), (c,), st, bt, 1e-5).permute(0, 3, 1, 2) if norm else r

    graph = torch_fwd()
    if norm and leg.startswith("torch"):   # the yardstick computes what the node computes
        torch.cuda.synchronize()
        assert (graph.detach() - y).abs().max().item() < 1e-4

    def bwd():
        if norm:
            ops.patch_expand_backward(x, scales, mean, rstd, dy, dx, dscales, db, p, order, True)
        else:
            ops.patch_expand_backward(None, None, None, None, dy, dx, None, None, p, order, True)

    fns = {"fwd": lambda: ops.patch_expand_forward(x, scales if norm else None, b if norm else None, y, mean if norm else None,
                                                   rstd if norm else None, p, order),
           "bwd": bwd, "torch_fwd": torch_fwd, "torch_bwd": lambda: torch.autograd.grad(graph, wrt, dy, retain_graph=True)}
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    fn = fns[leg]
    t0, warm = time.perf_counter(), 0
    while warm < 3 or time.perf_counter() - t0 < MIN_WARM_S:
        fn()
        torch.cuda.synchronize()
        L.bcnn_hip_sync()
        warm += 1

    def timed(calls):
        L.bcnn_hip_event_record(e0)
        for _ in range(calls):
            fn()
        L.bcnn_hip_event_record(e1)
        L.bcnn_hip_event_sync(e1)
        return L.bcnn_hip_event_elapsed_ms(e0, e1) / calls

    pilot = timed(iters)
    iters = max(iters, int(MIN_WINDOW_S * 1e3 / pilot) + 1)
    ms = timed(iters)
    nbytes = 4.0 * (3 if leg.endswith("bwd") and norm else 2) * x.numel()
    sweep_ms = nbytes / SWEEP_BYTES_PER_S * 1e3
    path = ops.PATCH_EXPAND_PATHS[ops.patch_expand_path(n, p * p * c, h, w, p)] if norm else "copy"
    print(json.dumps({"shape": name, "dims": list(src), "block": p, "order": order, "norm": norm, "leg": leg, "path": path,
                      "iters": iters, "ms": ms, "bytes": nbytes, "gbs": nbytes / ms * 1e-6, "sweep_ms_at_6.7TBs": sweep_ms,
                      "fraction_of_sweep_rate": sweep_ms / ms, "fits_llc": nbytes <= LLC_BYTES}), flush=True)


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
                print("%-5s %-9s %-6s rep %d  %8.4f ms %7.1f GB/s   (%.2f of the 6.7 TB/s sweep rate)" % (
                    name, r["leg"], r["path"], rep, r["ms"], r["gbs"], r["fraction_of_sweep_rate"]), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {}
    for name in SHAPES:
        for leg in LEGS:
            mine = [r for r in runs if r["shape"] == name and r["leg"] == leg]
            summary[name + "_" + leg] = {"dims": mine[0]["dims"], "path": mine[0]["path"], "ms": med([r["ms"] for r in mine]),
                                         "gbs": med([r["gbs"] for r in mine]),
                                         "ms_spread": [min(r["ms"] for r in mine), max(r["ms"] for r in mine)],
                                         "fraction_of_sweep_rate": med([r["fraction_of_sweep_rate"] for r in mine]),
                                         "fits_llc": mine[0]["fits_llc"]}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/patch_expand_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary,
                       "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
