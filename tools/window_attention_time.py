#!/usr/bin/env python
"""Time per call of the window-attention kernels (bcnn_amd/csrc/attention_window.hip), forward and
forward + backward with the bias table and its gradient, between device events, at Swin-T shapes (N = 32, d = c = 32), each
with shift 0 and shift ws / 2:

  shape    heads  H x W    ws
  stage1   3      56 x 56  7
  stage3   12     14 x 14  7
  stage4   24     7 x 7    7
  ws8      3      64 x 64  8

next to two outside yardsticks that no test or threshold depends on:

  global_*  the project's own ops.attention_forward / _backward on a pre-partitioned copy (N * windows images of ws x ws); the
            partition and reverse copies are not timed, and it has no bias and no mask (timed once, it knows no shift)
  torch_*   torch-ROCm fp32: roll, partition, bmm + bias + mask, softmax, bmm, reverse, roll back; autograd's backward

Every (shape, shift, leg, repeat) runs in a fresh process: a warm-up of at least 80 ms and 3 calls, then --iters calls between
two device events. The summary is the median over the repeats with the spread. A process that finds no device fails.

    python tools/window_attention_time.py [--out profiles/window_attention.json]

--bf16 times the bf16 inference forward (attention_window_bf16.hip) instead: the legs ours_fwd (the
unchanged fp32 forward, the yardstick) and ours_fwd_bf16, alternating, under the same protocol:

    python tools/window_attention_time.py --bf16 [--out profiles/window_attention_bf16.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
N, DIM = 32, 32
SHAPES = {"stage1": (3, 56, 56, 7), "stage3": (12, 14, 14, 7), "stage4": (24, 7, 7, 7), "ws8": (3, 64, 64, 8)}
LEGS = ("ours_fwd", "ours_fwdbwd", "global_fwd", "global_fwdbwd", "torch_fwd", "torch_fwdbwd")
BF16_LEGS = ("ours_fwd", "ours_fwd_bf16")


def _leg(name, shift, leg, iters):
    sys.path.insert(0, ROOT)
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    heads, h, w, ws = SHAPES[name]
    dev, length, nwin = "cuda:0", ws * ws, (h // ws) * (w // ws)
    gen = torch.Generator().manual_seed(1)
    q, k, v, do = [torch.randn((N, heads * DIM, h, w), generator=gen).to(dev) for _ in range(4)]
    table = torch.randn(heads * (2 * ws - 1) ** 2, generator=gen).to(dev)
    backward = leg.endswith("bwd")

    if leg.startswith("ours"):
        o, dq, dk, dv, dtable = [torch.zeros_like(x) for x in (v, q, k, v, table)]

        forward = ops.window_attention_forward_bf16 if leg.endswith("bf16") else ops.window_attention_forward

        def fn():
            forward(q, k, v, table, o, heads, ws, shift)
            if backward:
                ops.window_attention_backward(q, k, v, table, do, dq, dk, dv, dtable, heads, ws, shift, overwrite=(True,) * 3)
    elif leg.startswith("global"):
        pq, pk, pv, pdo = [torch.randn((N * nwin, heads * DIM, ws, ws), generator=gen).to(dev) for _ in range(4)]
        o, lse = torch.empty_like(pv), torch.empty(N * nwin * heads * length, device=dev)
        dq, dk, dv = [torch.empty_like(x) for x in (pq, pk, pv)]

        def fn():
            ops.attention_forward(pq, pk, pv, o, lse, heads)
            if backward:
                ops.attention_backward(pq, pk, pv, o, lse, pdo, dq, dk, dv, heads, overwrite=(True, True, True))
    else:
        ys, xs = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        rel = ((ys[:, None] - ys[None, :] + ws - 1) * (2 * ws - 1) + xs[:, None] - xs[None, :] + ws - 1).to(dev)
        mask = None
        if shift:
            region = lambda e: (torch.arange(e) >= e - ws).int() + (torch.arange(e) >= e - shift).int()
            code = (3 * region(h)[:, None] + region(w)[None, :]).reshape(h // ws, ws, w // ws, ws).permute(0, 2, 1, 3)
            code = code.reshape(nwin, length)
            mask = torch.zeros(nwin, length, length).masked_fill(code[:, :, None] != code[:, None, :], float("-inf")).to(dev)
        tq, tk, tv, tt = [x.clone().requires_grad_(backward) for x in (q, k, v, table)]

        def windows(x):
            x = torch.roll(x, (-shift, -shift), (2, 3)) if shift else x
            return x.reshape(N, heads, DIM, h // ws, ws, w // ws, ws).permute(0, 3, 5, 1, 2, 4, 6).reshape(-1, DIM, length)

        def fn():
            s = torch.bmm(windows(tq).transpose(1, 2), windows(tk)) * DIM ** -0.5
            s = s.view(N, nwin, heads, length, length) + tt.view(heads, -1)[:, rel][None, None]
            if mask is not None:
                s = s + mask[None, :, None]
            p = torch.softmax(s, -1).view(-1, length, length)
            out = torch.bmm(windows(tv), p.transpose(1, 2)).view(N, h // ws, w // ws, heads, DIM, ws, ws)
            out = out.permute(0, 3, 4, 1, 5, 2, 6).reshape(N, heads * DIM, h, w)
            out = torch.roll(out, (shift, shift), (2, 3)) if shift else out
            if backward:
                tq.grad = tk.grad = tv.grad = tt.grad = None
                out.backward(do)

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
    print(json.dumps({"shape": name, "dims": [N, heads, DIM, DIM, h, w, ws], "shift": shift, "leg": leg, "iters": iters,
                      "ms": ms}), flush=True)


def _child(name, shift, leg, iters):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--shift", str(shift), "--leg", leg,
                        "--iters", str(iters)], capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("%s %s failed (%d):\n%s\n%s" % (name, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return [json.loads(line) for line in r.stdout.strip().splitlines() if line.startswith("{")][0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bf16", action="store_true", help="time the bf16 forward against the fp32 forward")
    ap.add_argument("--out", default=None, help="also write the raw record as JSON here")
    ap.add_argument("--shape", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--shift", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.shape:
        _leg(a.shape, a.shift, a.leg, a.iters)
        return
    cases = [(name, shift, leg) for name in SHAPES for shift in (0, SHAPES[name][3] // 2) for leg in (BF16_LEGS if a.bf16 else LEGS)
             if shift == 0 or not leg.startswith("global")]
    runs = []
    for rep in range(a.repeats):   # alternating: every case once per round
        for name, shift, leg in cases:
            r = _child(name, shift, leg, a.iters)
            r["repeat"] = rep
            runs.append(r)
            print("%-7s shift %d %-14s rep %d  %8.4f ms" % (name, shift, leg, rep, r["ms"]), flush=True)
    summary = {}
    for name, shift, leg in cases:
        mine = sorted(r["ms"] for r in runs if (r["shape"], r["shift"], r["leg"]) == (name, shift, leg))
        summary["%s_shift%d_%s" % (name, shift, leg)] = {"ms": mine[len(mine) // 2], "ms_spread": [mine[0], mine[-1]]}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/window_attention_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary,
                       "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
