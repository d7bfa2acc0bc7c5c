#!/usr/bin/env python
"""Time per call of the attention kernels (bcnn_amd/csrc/attention.hip), forward and forward + backward,
between device events, next to torch-ROCm's own fp32 softmax(q^T k) v on the same device as an outside yardstick:

  shape      N   heads  d    c    Lq = Lk
  danet      8   1      64   128  64 x 64   (position attention of a segmentation head; its c = 512 is above the node's limit)
  botnet     32  4      128  128  14 x 14
  mobilevit  32  4      36   36   16 x 16

  ours_fwd      bcnn_hip_attention_forward, log-sum-exp stored
  ours_fwdbwd   ... and bcnn_hip_attention_backward, the three gradients assigned
  torch_fwd     torch.softmax(q^T k * scale, -1) and the product with v (S and P go through memory)
  torch_fwdbwd  ... and autograd's backward          (a yardstick printed next to ours: no test or threshold depends on it)

flops: what the matrix instructions of our kernels execute, 2 nh Lq Lk (d + c) forward and 2 nh Lq Lk (4 d + 3 c) backward (the
two-pass backward forms S and dP twice), against the 157 TFLOP/s fp32-MFMA peak. bytes: q, k, v and o once (and dO and the three
gradients in the backward), what a call has to move whatever it does inside.

--bf16 times two legs only, in the same session: ours_fwd and ours_fwd_bf16, bcnn_hip_attention_forward_bf16
(bcnn_amd/csrc/attention_bf16.hip, DESIGN.md section 36: the same flops on v_mfma_f32_32x32x16_bf16, against the 2517 TFLOP/s
bf16-MFMA peak), and adds the ratio of their medians to the summary.

Every (shape, leg, repeat) runs in a fresh process: a warm-up of at least 80 ms and 3 calls, then --iters calls between two
device events. The summary is the median over the repeats. A process that finds no device fails.

    python tools/attention_time.py [--out profiles/attention.json]
    python tools/attention_time.py --bf16 [--out profiles/attention_bf16.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
PEAK_TFLOPS = 157.0
PEAK_BF16_TFLOPS = 2517.0
SHAPES = {"danet": (8, 1, 64, 128, 64, 64), "botnet": (32, 4, 128, 128, 14, 14), "mobilevit": (32, 4, 36, 36, 16, 16)}
LEGS = ("ours_fwd", "ours_fwdbwd", "torch_fwd", "torch_fwdbwd")
BF16_LEGS = ("ours_fwd", "ours_fwd_bf16")


def _leg(name, leg, iters):
    sys.path.insert(0, ROOT)
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    n, heads, d, c, h, w = SHAPES[name]
    length, nh, dev = h * w, n * heads, "cuda:0"
    gen = torch.Generator().manual_seed(1)
    q, k = [torch.randn((n, heads * d, h, w), generator=gen).to(dev) for _ in range(2)]
    v, do = [torch.randn((n, heads * c, h, w), generator=gen).to(dev) for _ in range(2)]
    o, lse = torch.empty_like(v), torch.empty(nh * length, device=dev)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    scale = d ** -0.5
    backward = leg.endswith("bwd")

    forward = ops.attention_forward_bf16 if leg.endswith("bf16") else ops.attention_forward
    peak = PEAK_BF16_TFLOPS if leg.endswith("bf16") else PEAK_TFLOPS

    def ours():
        forward(q, k, v, o, lse, heads)
        if backward:
            ops.attention_backward(q, k, v, o, lse, do, dq, dk, dv, heads, overwrite=(True, True, True))

    tq, tk, tv = [x.view(nh, -1, length).requires_grad_(backward) for x in (q, k, v)]
    tdo = do.view(nh, c, length)

    def theirs():
        p = torch.softmax(torch.bmm(tq.transpose(1, 2), tk) * scale, -1)
        out = torch.bmm(tv, p.transpose(1, 2))
        if backward:
            tq.grad = tk.grad = tv.grad = None
            out.backward(tdo)

    fn = ours if leg.startswith("ours") else theirs
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
    pairs = 2.0 * nh * length * length
    flops = pairs * (d + c) + (pairs * (4 * d + 3 * c) if backward else 0.0)
    nbytes = 4.0 * nh * length * (2 * d + 2 * c) * (2 if backward else 1) + (4.0 * nh * length * c if backward else 0.0)
    print(json.dumps({"shape": name, "dims": list(SHAPES[name]), "leg": leg, "iters": iters, "ms": ms, "flops": flops,
                      "tflops": flops / ms * 1e-9, "of_peak": flops / ms * 1e-9 / peak, "peak_tflops": peak, "bytes": nbytes,
                      "gbs": nbytes / ms * 1e-6}), flush=True)


def _child(name, leg, iters):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--leg", leg, "--iters", str(iters)],
                       capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("%s %s failed (%d):\n%s\n%s" % (name, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return [json.loads(line) for line in r.stdout.strip().splitlines() if line.startswith("{")][0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bf16", action="store_true", help="time ours_fwd and ours_fwd_bf16 only")
    ap.add_argument("--out", default=None, help="also write the raw record as JSON here")
    ap.add_argument("--shape", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.shape:
        _leg(a.shape, a.leg, a.iters)
        return
    legs = BF16_LEGS if a.bf16 else LEGS
    runs = []
    for rep in range(a.repeats):   # alternating: every (shape, leg) once per round
        for name in SHAPES:
            for leg in legs:
                r = _child(name, leg, a.iters)
                r["repeat"] = rep
                runs.append(r)
                print("%-9s %-12s rep %d  %8.4f ms %6.1f TFLOP/s (%4.1f %% of %g) %7.1f GB/s" % (
                    name, leg, rep, r["ms"], r["tflops"], 100 * r["of_peak"], r["peak_tflops"], r["gbs"]), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {}
    for name in SHAPES:
        for leg in legs:
            mine = [r for r in runs if r["shape"] == name and r["leg"] == leg]
            summary[name + "_" + leg] = {"dims": mine[0]["dims"], "ms": med([r["ms"] for r in mine]),
                                         "tflops": med([r["tflops"] for r in mine]), "gbs": med([r["gbs"] for r in mine]),
                                         "ms_spread": [min(r["ms"] for r in mine), max(r["ms"] for r in mine)]}
    if a.bf16:
        for name in SHAPES:
            summary[name + "_fp32_over_bf16"] = summary[name + "_ours_fwd"]["ms"] / summary[name + "_ours_fwd_bf16"]["ms"]
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/attention_time.py", "iters": a.iters, "repeats": a.repeats, "peak_tflops": PEAK_TFLOPS,
                       "summary": summary, "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
