#!/usr/bin/env python
"""Time per call of the group-normalisation kernels (bcnn_amd/csrc/group_norm.hip) on the three paths,
between device events, next to torch-ROCm's own group norm on the same tensors in the same process:

  shape  N    C    H x W    G    path
  a      32   256  56 x 56  32   split     (rows of 25088 floats)
  b      32   512  14 x 14  32   resident  (rows of 3136 floats)
  c      2    256  56 x 56  1    split     (two rows of 802816 floats: layer norm at N = 2)
  d      64   72   7 x 7    72   lanes     (instance norm on 7 x 7 planes)
  e      2    63   16 x 16  1    forward resident, backward split (two rows of 16128 floats)
  f      2    64   16 x 16  1    split                            (two rows of 16384 floats)
  g      2    63   8 x 16   1    resident                         (two rows of 8064 floats)
  h      2    64   8 x 16   1    forward resident, backward split (two rows of 8192 floats)
  (e - h: layer norm at N = 2 on either side of the resident limits, e against f forward and g against h backward: what two
  workgroups cost against the split path's extra launches)

  ours_fwd   bcnn_hip_group_norm_forward, mean and rstd stored       x read, y written              8 bytes / element
  ours_bwd   bcnn_hip_group_norm_backward, overwrite, all gradients  x, dy read, dx written        12 bytes / element
  torch_fwd  aten.native_group_norm                                  (a yardstick printed next to ours: no test or
  torch_bwd  aten.native_group_norm_backward, all three gradients     threshold depends on it)

floor = bytes / 8 TB/s, what a cold call has to take. A repeated call whose tensors fit the 256 MB last-level cache is not
running at an HBM rate: the record says which working sets fit.

Every (shape, repeat) runs in a fresh process that measures the four legs one after the other; a leg warms up for at least
80 ms and 3 calls, then times --iters calls between two device events. The summary is the median over the processes. A
process that finds no device fails.

    python tools/group_norm_time.py [--out profiles/group_norm.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
SHAPES = {"a": (32, 256, 56, 56, 32), "b": (32, 512, 14, 14, 32), "c": (2, 256, 56, 56, 1), "d": (64, 72, 7, 7, 72),
          "e": (2, 63, 16, 16, 1), "f": (2, 64, 16, 16, 1), "g": (2, 63, 8, 16, 1), "h": (2, 64, 8, 16, 1)}
LEGS = ("ours_fwd", "ours_bwd", "torch_fwd", "torch_bwd")
LLC_BYTES = 256e6


def _shape(name, iters):
    sys.path.insert(0, ROOT)
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    n, c, h, w, g = SHAPES[name]
    elems = n * c * h * w
    gen = torch.Generator().manual_seed(1)
    dev = "cuda:0"
    x = (torch.randn((n, c, h, w), generator=gen) + 0.5).to(dev)
    dy = torch.randn((n, c, h, w), generator=gen).to(dev)
    gamma, beta = (torch.rand(c, generator=gen) + 0.5).to(dev), torch.randn(c, generator=gen).to(dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(n * g, device=dev), torch.empty(n * g, device=dev)
    dgamma, dbeta = torch.zeros(c, device=dev), torch.zeros(c, device=dev)
    ops.group_norm_forward(x, gamma, beta, y, mean, rstd, g, 1e-5)
    aten = torch.ops.aten
    fns = {
        "ours_fwd": (lambda: ops.group_norm_forward(x, gamma, beta, y, mean, rstd, g, 1e-5), 8),
        "ours_bwd": (lambda: ops.group_norm_backward(x, gamma, mean, rstd, dy, dx, dgamma, dbeta, g, True), 12),
        "torch_fwd": (lambda: aten.native_group_norm(x, gamma, beta, n, c, h * w, g, 1e-5), 8),
        "torch_bwd": (lambda: aten.native_group_norm_backward(dy, x, mean.view(n, g), rstd.view(n, g), gamma, n, c, h * w, g,
                                                              [True, True, True]), 12),
    }
    paths = {"ours_fwd": ops.GROUP_NORM_PATHS[ops.group_norm_path(n, c, h * w, g, False)],
             "ours_bwd": ops.GROUP_NORM_PATHS[ops.group_norm_path(n, c, h * w, g, True)]}
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    for leg in LEGS:
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


def _child(name, iters):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--iters", str(iters)],
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
        _shape(a.shape, a.iters)
        return
    runs = []
    for rep in range(a.repeats):   # alternating: every shape once per round
        for name in SHAPES:
            for r in _child(name, a.iters):
                r["repeat"] = rep
                runs.append(r)
                print("%s %-10s %-9s rep %d  %8.4f ms %7.1f GB/s   (floor at 8 TB/s %7.4f ms)" % (
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
            json.dump({"tool": "tools/group_norm_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary,
                       "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
