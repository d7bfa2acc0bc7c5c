#!/usr/bin/env python
"""Time per call of the dice-loss kernels (bcnn_amd/csrc/dice_loss.hip) between device events:

  shape       N    C     H x W        path
  swin_unet   24   9     224 x 224    register   Swin-UNet on Synapse
  voc         8    21    513 x 513    register   (hw is odd: one pixel per lane)
  cityscapes  4    19    512 x 1024   register
  ade20k      8    150   128 x 128    wide

  fwd / bwd         bcnn_hip_dice_loss_forward (p, sums, finalize: loss and coefficients) / _backward (overwrite),
                    0.4 CE + 0.6 Dice, squared, reduce batch, ignore label 255 on 5 % of the pixels
  sl_fwd / sl_bwd   the softmax-loss node's forward with the label / backward at the same shape: the nearest path the
                    project had before this node (cross-entropy alone)
  torch_fwd_bwd     torch-ROCm: cross_entropy + the same Dice expression, and autograd through it, as one leg (a
                    yardstick printed next to ours: no test or threshold depends on it)

bytes: what a pass has to move at least: x (or p) read, p (or dx) written, the label read. The wide path reads p once more
to form the sums; that read is not in `bytes`, so its GB/s is the rate of the useful traffic. A repeated call whose
tensors fit the 256 MB last-level cache is not running at an HBM rate: the record says which fit.

Every (shape, leg, repeat) runs in a fresh process; the leg warms up for at least 80 ms and 3 calls, times --iters calls
between two device events as a pilot, and then times as many calls as fill a window of at least 0.25 s (never fewer than
--iters). The summary is the median over the processes, with the spread. A process that finds no device fails.

    python tools/dice_loss_time.py [--out profiles/dice_loss.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
MIN_WINDOW_S = 0.25
SHAPES = {"swin_unet": (24, 9, 224, 224), "voc": (8, 21, 513, 513), "cityscapes": (4, 19, 512, 1024), "ade20k": (8, 150, 128, 128)}
LEGS = ("fwd", "bwd", "sl_fwd", "sl_bwd", "torch_fwd_bwd")
IGNORE = 255
LLC_BYTES = 256e6


def _shape(name, leg, iters):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    n, c, h, w = SHAPES[name]
    hw, dev, gen = h * w, "cuda:0", torch.Generator().manual_seed(1)
    x = (torch.rand((n, c, hw), generator=gen) * 12 - 6).to(dev)
    lab = torch.randint(0, c, (n, 1, hw), generator=gen).float()
    lab[torch.rand((n, 1, hw), generator=gen) < 0.05] = IGNORE
    lab = lab.to(dev)
    p, dx = torch.empty_like(x), torch.empty_like(x)
    ws, rec = ops.dice_loss_workspace(n, c, hw), ops.softmax_loss_record()
    kw = dict(ignore_label=IGNORE, normalize="valid")
    ops.dice_loss_forward(x, lab, p, ws, ignore_label=IGNORE)   # p, the record and the coefficients exist before a backward leg
    ops.softmax_loss_forward(x, lab, p, rec, **kw)
    xt, t = x.clone().requires_grad_(True), lab[:, 0].long()

    def torch_fwd_bwd():
        valid = (t != IGNORE).unsqueeze(1)
        q = xt.softmax(1) * valid
        onehot = F.one_hot(torch.where(t == IGNORE, 0, t), c).permute(0, 2, 1) * valid
        i, z, y = (q * onehot).sum((0, 2)), (q * q).sum((0, 2)), onehot.sum((0, 2))
        loss = 0.4 * F.cross_entropy(xt, t, ignore_index=IGNORE) + 0.6 * (1 - (2 * i + 1e-5) / (z + y + 1e-5)).mean()
        return torch.autograd.grad(loss, xt)

    if leg == "torch_fwd_bwd":   # the yardstick computes what the node computes
        ops.dice_loss_backward(p, lab, ws, dx, ignore_label=IGNORE, overwrite=True)
        torch.cuda.synchronize()
        assert (torch_fwd_bwd()[0] - dx).abs().max().item() <= 1e-5 * dx.abs().max().item() + 1e-12
    fns = {"fwd": lambda: ops.dice_loss_forward(x, lab, p, ws, ignore_label=IGNORE),
           "bwd": lambda: ops.dice_loss_backward(p, lab, ws, dx, ignore_label=IGNORE, overwrite=True),
           "sl_fwd": lambda: ops.softmax_loss_forward(x, lab, p, rec, **kw),
           "sl_bwd": lambda: ops.softmax_loss_backward(p, lab, rec, dx, overwrite=True, **kw), "torch_fwd_bwd": torch_fwd_bwd}
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
    nbytes = 4.0 * (2 * x.numel() + lab.numel()) * (2 if leg == "torch_fwd_bwd" else 1)
    print(json.dumps({"shape": name, "dims": [n, c, h, w], "leg": leg, "path": ("register", "wide")[ops.dice_loss_path(n, c, hw)],
                      "iters": iters, "ms": ms, "bytes": nbytes, "gbs": nbytes / ms * 1e-6, "fits_llc": nbytes <= LLC_BYTES}), flush=True)


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
                print("%-10s %-13s %-8s rep %d  %8.4f ms %7.1f GB/s" % (name, r["leg"], r["path"], rep, r["ms"], r["gbs"]), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {}
    for name in SHAPES:
        for leg in LEGS:
            mine = [r for r in runs if r["shape"] == name and r["leg"] == leg]
            summary[name + "_" + leg] = {"dims": mine[0]["dims"], "path": mine[0]["path"], "ms": med([r["ms"] for r in mine]),
                                         "gbs": med([r["gbs"] for r in mine]),
                                         "ms_spread": [min(r["ms"] for r in mine), max(r["ms"] for r in mine)],
                                         "fits_llc": mine[0]["fits_llc"]}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/dice_loss_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary, "runs": runs},
                      fh, indent=1)


if __name__ == "__main__":
    main()
