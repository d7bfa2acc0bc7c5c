#!/usr/bin/env python
"""Time per call of the softmax-loss kernels (bcnn_amd/csrc/softmax_loss.hip) between device
events, next to the chain the node replaces, measured in the same process on the same logits. fp32:

  case      logits (N, C, H, W)      what it is
  voc       (8, 21, 513, 513)        a DeepLab batch on VOC: the register path, scalar form (513 * 513 is odd)
  ade       (8, 150, 129, 129)       ADE20K's 150 classes at the decoder's stride: the streaming path, scalar form
  imagenet  (256, 1000, 1, 1)        a classifier: the rows path

  new_fwd / new_bwd / new_confusion   bcnn_hip_softmax_loss_forward (with the label: probabilities, loss, counts and the
                                      finalize launch), _backward in its overwrite form, _confusion
  new_upload                          the class-index label map, host to device (bcnn_hip_memcpy_h2d, pageable memory)
  chain_softmax / chain_grad /        what the softmax and cost nodes launch in a TRAIN forward, one leg each:
  chain_metric                        softmax_kernel; copy and axpy(-1, label); the metric kernels
                                      (BCNN_METRIC_ERROR_RATE: one argmax over C * H * W values per image). The cost
                                      node's 4-byte read-back and the wait it implies are NOT included. The summary's
                                      chain_fwd is the sum of the three medians
  chain_bwd                           their backward: two axpys
  chain_upload                        the dense one-hot label, host to device

About one pixel in eight carries the ignore label 255 (the chain has no such thing: its label stays one-hot there).
Each record carries the trace names of one call's launches and the least bytes the leg must move -- forward: read x and
the label map, write p; backward: read p and the label map, write dx; confusion: read p and the label map; the chain's
forward legs their own minimum (softmax: x and p; gradient: p, y and p - y; metric: p), its backward the same minimum as
the new backward. Every (case, repeat) runs in a fresh process that measures the legs one after the other; a leg warms
up for at least 80 ms and 3 calls, then times --iters calls between two device events. The summary is the median over
the processes with the spread (min, max), and the ratios chain / new per direction and for a whole step (upload +
forward + backward). A process that finds no device fails.

    python tools/softmax_loss_time.py [--out profiles/softmax_loss.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
CASES = {"voc": (8, 21, 513, 513), "ade": (8, 150, 129, 129), "imagenet": (256, 1000, 1, 1)}
LEGS = ("new_fwd", "new_bwd", "new_confusion", "new_upload", "chain_softmax", "chain_grad", "chain_metric", "chain_bwd",
        "chain_upload")
CHAIN_FWD = ("chain_softmax", "chain_grad", "chain_metric")
IGNORE = 255


def _case(name, iters):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from bcnn_amd import _lib, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    n, c, h, w = CASES[name]
    hw, total = h * w, n * c * h * w
    gen = torch.Generator().manual_seed(1)
    dev = "cuda:0"
    x = (4 * torch.randn((n, c, hw), generator=gen)).to(dev)
    cls = torch.randint(0, c, (n, 1, hw), generator=gen)
    lab_host = cls.float()
    lab_host[torch.rand((n, 1, hw), generator=gen) < 0.125] = IGNORE
    lab_host = lab_host.numpy()
    onehot_host = np.zeros((n, c, hw), np.float32)
    np.put_along_axis(onehot_host, cls.numpy(), 1.0, axis=1)
    lab = torch.from_numpy(lab_host).to(dev)
    onehot = torch.from_numpy(onehot_host).to(dev)
    p, dx = torch.empty_like(x), torch.empty_like(x)
    rec = ops.softmax_loss_record()
    y, gcost, gprob, gx = torch.empty_like(x), torch.empty_like(x), torch.zeros_like(x), torch.zeros_like(x)
    metric = torch.zeros(1, device=dev)
    kw = dict(ignore_label=IGNORE, normalize="valid_per_image", scale=1.0)
    P = lambda t: t.data_ptr()   # noqa: E731

    def chain_grad():   # bcnn_forward_cost_layer (bcnn_layers_next.c): the gradient p - y
        L.bcnn_hip_copy_f32(total, P(y), P(gcost))
        L.bcnn_hip_axpy(total, -1.0, P(onehot), P(gcost))

    def chain_bwd():   # bcnn_backward_cost_layer, bcnn_backward_softmax_layer
        L.bcnn_hip_axpy(total, 1.0, P(gcost), P(gprob))
        L.bcnn_hip_axpy(total, 1.0, P(gprob), P(gx))

    fwd_bytes, conf_bytes = 4 * (2 * total + n * hw), 4 * (total + n * hw)
    fns = {
        "new_fwd": (lambda: ops.softmax_loss_forward(x, lab, p, rec, **kw), fwd_bytes),
        "new_bwd": (lambda: ops.softmax_loss_backward(p, lab, rec, dx, overwrite=True, **kw), fwd_bytes),
        "new_confusion": (lambda: ops.softmax_loss_confusion(p, lab, ignore_label=IGNORE), conf_bytes),
        "new_upload": (lambda: L.bcnn_hip_memcpy_h2d(P(lab), lab_host.ctypes.data, lab_host.nbytes), lab_host.nbytes),
        "chain_softmax": (lambda: L.bcnn_hip_softmax_forward(P(x), P(y), n, c, hw), 8 * total),   # bcnn_forward_softmax_layer
        "chain_grad": (chain_grad, 12 * total),   # read p and y, write p - y
        "chain_metric": (lambda: L.bcnn_hip_cost_metric(0, P(y), P(onehot), P(gcost), n, c * hw, P(metric)), 4 * total),
        "chain_bwd": (chain_bwd, fwd_bytes),
        "chain_upload": (lambda: L.bcnn_hip_memcpy_h2d(P(onehot), onehot_host.ctypes.data, onehot_host.nbytes),
                         onehot_host.nbytes),
    }
    ops.softmax_loss_forward(x, lab, p, rec, **kw)   # p and the record exist before the backward leg runs
    stats = ops.softmax_loss_read_record(rec)
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    for leg in LEGS:
        fn, nbytes = fns[leg]
        t0, warm = time.perf_counter(), 0
        while warm < 3 or time.perf_counter() - t0 < MIN_WARM_S:
            fn()
            L.bcnn_hip_sync()
            warm += 1
        L.bcnn_hip_trace_enable(1)
        fn()
        L.bcnn_hip_sync()
        size = L.bcnn_hip_trace_read(None, 0)
        buf = ctypes.create_string_buffer(size + 1)
        L.bcnn_hip_trace_read(buf, size + 1)
        L.bcnn_hip_trace_enable(0)
        L.bcnn_hip_event_record(e0)
        for _ in range(iters):
            fn()
        L.bcnn_hip_event_record(e1)
        L.bcnn_hip_event_sync(e1)
        ms = L.bcnn_hip_event_elapsed_ms(e0, e1) / iters
        print(json.dumps({"case": name, "logits": [n, c, h, w], "leg": leg, "kernels": buf.value.decode().split(),
                          "iters": iters, "ms": ms, "min_bytes": nbytes, "gbps": nbytes / ms * 1e-6,
                          "valid": stats["valid"], "ignored": stats["ignored"]}), flush=True)


def _child(name, iters):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--iters", str(iters)],
                       capture_output=True, text=True, cwd=ROOT, timeout=240)   # a hung child ends the whole run
    if r.returncode != 0:
        raise SystemExit("case %s failed (%d):\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return [json.loads(line) for line in r.stdout.strip().splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the raw record as JSON here")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        _case(a.case, a.iters)
        return
    runs = []
    for rep in range(a.repeats):   # alternating: every case once per round
        for name in CASES:
            for r in _child(name, a.iters):
                r["repeat"] = rep
                runs.append(r)
                print("%-9s %-14s rep %d  %9.4f ms %7.0f GB/s   %s" % (name, r["leg"], rep, r["ms"], r["gbps"],
                                                                       " ".join(r["kernels"])), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    summary = {}
    for name in CASES:
        for leg in LEGS:
            mine = [r for r in runs if r["case"] == name and r["leg"] == leg]
            summary[name + "_" + leg] = {"logits": mine[0]["logits"], "kernels": mine[0]["kernels"],
                                         "ms": med([r["ms"] for r in mine]),
                                         "ms_spread": [min(r["ms"] for r in mine), max(r["ms"] for r in mine)],
                                         "min_bytes": mine[0]["min_bytes"], "gbps": med([r["gbps"] for r in mine])}
        ms = lambda leg: summary[name + "_" + leg]["ms"]   # noqa: E731
        summary[name + "_chain_fwd"] = {"logits": summary[name + "_new_fwd"]["logits"], "ms": sum(ms(leg) for leg in CHAIN_FWD),
                                        "sum_of": list(CHAIN_FWD)}
        summary[name + "_ratios"] = {
            "chain_over_new_fwd": ms("chain_fwd") / ms("new_fwd"), "chain_over_new_bwd": ms("chain_bwd") / ms("new_bwd"),
            "chain_over_new_upload": ms("chain_upload") / ms("new_upload"),
            "chain_over_new_step": (ms("chain_upload") + ms("chain_fwd") + ms("chain_bwd")) /
                                   (ms("new_upload") + ms("new_fwd") + ms("new_bwd"))}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/softmax_loss_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary,
                       "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
