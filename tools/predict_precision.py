#!/usr/bin/env python
"""What the inference-precision switch (bcnn_set_inference_precision) buys: the PREDICT-mode forward of
the benchmark's ResNet-18 graph (bench.py: build_resnet18) at 224 x 224, N = 128, timed three ways --

  parent_fp32   a built checkout of the parent commit (--parent-tree DIR; left out when not given)
  fp32          this tree, default precision: has to match the parent within the run-to-run spread
  bf16          this tree, BCNN_PRECISION_BF16

-- and, layer by layer, the bf16 kernel next to the fp32 family it displaces (the library's own per-class kernel timers,
bcnn_hip_profile_*; the family's name comes from the dispatch trace).

Every leg runs in a process of its own (the parent tree brings its own bcnn_amd package), the legs alternate, and each
is repeated --repeats times: the spread of the repeats is what a difference has to exceed. A leg warms up for at least
80 ms and 3 passes like bench.py, then times --steps forwards between two device events.

    python tools/predict_precision.py [--parent-tree DIR] [--out profiles/predict_precision.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08


def resnet18_conv_layers(n, base=64):
    """(name, (N, C, H, W, F, k, s, p, g), batch_norm, act) of every distinct convolution shape of build_resnet18 at 224 x 224"""
    layers = [("conv0 7x7/s2", (n, 3, 224, 224, base, 7, 2, 3, 1))]
    c, hw = base, 56
    for stage, width in enumerate((base, 2 * base, 4 * base, 8 * base), start=1):
        if stage > 1:
            layers.append(("s%d 3x3/s2" % stage, (n, c, hw, hw, width, 3, 2, 1, 1)))
            layers.append(("s%d proj 1x1/s2" % stage, (n, c, hw, hw, width, 1, 2, 0, 1)))
            hw //= 2
        layers.append(("s%d 3x3" % stage, (n, width, hw, hw, width, 3, 1, 1, 1)))
        c = width
    return layers


def _forward_leg(tree, precision, batch, steps):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import bench
    from bcnn_amd import capi
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    net = capi.Net(mode=capi.MODE_PREDICT, n=batch, w=224, h=224, c=3)
    bench.build_resnet18(net, capi)
    net.compile()
    rs = np.random.RandomState(0)
    net.data(0)[...] = rs.uniform(-1, 1, net.shape(0)).astype(np.float32)
    net.upload(0)
    if precision == "bf16":
        assert net.set_inference_precision(capi.PRECISION_BF16) == 0
    t0, warm = time.perf_counter(), 0
    while warm < 3 or time.perf_counter() - t0 < MIN_WARM_S:
        net.forward()
        net.sync()
        warm += 1
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        net.forward()
    b.record()
    torch.cuda.synchronize()
    prob = net.index("prob")
    net.download(prob, with_grad=False)
    out = net.data(prob)
    print(json.dumps(dict(ms=a.elapsed_time(b) / steps, warm=warm, top1=[int(v) for v in out.reshape(batch, -1).argmax(1)[:16]],
                          pmax=[round(float(v), 6) for v in out.reshape(batch, -1).max(1)[:4]])))


def _trace(L, fn):
    L.bcnn_hip_trace_enable(1)
    fn()
    n = L.bcnn_hip_trace_read(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return buf.value.decode().split()


def _conv_kernel_ms(L, fn, reps):
    """mean time per call of the convolution-forward kernel classes (batch-norm and activation sweeps are other classes)"""
    L.bcnn_hip_profile_reset()
    L.bcnn_hip_profile_enable(1)
    for _ in range(reps):
        fn()
    L.bcnn_hip_profile_enable(0)
    total = 0.0
    for cls in range(L.bcnn_hip_profile_num_classes()):
        if not L.bcnn_hip_profile_class_name(cls).decode().startswith("conv_fwd"):
            continue
        ms, n, fl, by = C.c_double(), C.c_longlong(), C.c_double(), C.c_double()
        L.bcnn_hip_profile_read(cls, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by))
        total += ms.value
    L.bcnn_hip_profile_reset()
    return total / reps


def _layers_leg(batch, reps):
    sys.path.insert(0, ROOT)
    import torch
    from bcnn_amd import _lib, ops
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    L = _lib.load()
    dev = "cuda:0"
    rows = []
    for name, shape in resnet18_conv_layers(batch):
        n, c, h, w, f, k, s, p, g = shape
        gen = torch.Generator(device=dev).manual_seed(sum(shape))
        x = torch.rand((n, c, h, w), device=dev, generator=gen) * 2 - 1
        wt = (torch.rand((f, c // g, k, k), device=dev, generator=gen) * 2 - 1) * (3.0 / (c // g * k * k)) ** 0.5
        oh, ow = ops.conv_out_hw(h, w, k, s, p)
        y = torch.empty((n, f, oh, ow), device=dev)
        bn = dict(run_mean=torch.zeros(f, device=dev), run_var=torch.ones(f, device=dev), scales=torch.ones(f, device=dev),
                  saved_mean=torch.zeros(f, device=dev), saved_var=torch.zeros(f, device=dev))
        bias = torch.zeros(f, device=dev)
        # every convolution of the graph carries a fused batch-norm: the kernel runs with its raw epilogue
        fp32 = lambda: ops.conv_forward(x, wt, bias, y, k, s, p, g, 0, bn=bn, mode=ops.MODE_PREDICT)
        bf16 = lambda: ops.conv_forward_bf16(x, wt, bias, y, k, s, p, g, 0, bn=bn, mode=ops.MODE_PREDICT)
        family = [t for t in _trace(L, fp32) if "tail" not in t]
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < MIN_WARM_S:
            fp32()
            bf16()
            torch.cuda.synchronize()
        t32a = _conv_kernel_ms(L, fp32, reps)
        t16a = _conv_kernel_ms(L, bf16, reps)
        t32b = _conv_kernel_ms(L, fp32, reps)
        t16b = _conv_kernel_ms(L, bf16, reps)
        flops = 2.0 * n * oh * ow * f * (c // g) * k * k
        bytes_ = 4.0 * (x.numel() + wt.numel() + y.numel())
        rows.append(dict(layer=name, shape=list(shape), fp32_family=family[0] if family else "?",
                         fp32_ms=[round(t32a, 4), round(t32b, 4)], bf16_ms=[round(t16a, 4), round(t16b, 4)],
                         bf16_tflops=round(flops / (min(t16a, t16b) * 1e-3) / 1e12, 1),
                         bf16_gbs=round(bytes_ / (min(t16a, t16b) * 1e-3) / 1e9, 0)))
    print(json.dumps(rows))


def _child(args_list):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args_list, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("leg %s failed (%d):\n%s\n%s" % (args_list, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-tree", default=None, help="a BUILT checkout of the parent commit")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layer-reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the result as JSON here")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg == "layers":
        return _layers_leg(args.batch, args.layer_reps)
    if args.leg:
        return _forward_leg(args.tree, args.leg, args.batch, args.steps)

    legs = [("fp32", ROOT, "fp32"), ("bf16", ROOT, "bf16")]
    if args.parent_tree:
        legs.insert(0, ("parent_fp32", os.path.abspath(args.parent_tree), "fp32"))
    runs = {name: [] for name, _, _ in legs}
    for _ in range(args.repeats):          # alternating: whatever else the machine does hits every leg alike
        for name, tree, prec in legs:
            runs[name].append(_child(["--leg", prec, "--tree", tree, "--batch", str(args.batch), "--steps", str(args.steps)]))
    result = dict(workload="resnet18 PREDICT forward, 224x224, N=%d" % args.batch, steps=args.steps, forward_ms={})
    for name, rs in runs.items():
        ms = sorted(r["ms"] for r in rs)
        result["forward_ms"][name] = dict(runs=[round(m, 4) for m in ms], median=round(ms[len(ms) // 2], 4),
                                          spread=round(ms[-1] - ms[0], 4))
    result["top1_agree_bf16_vs_fp32"] = sum(int(a == b) for a, b in zip(runs["bf16"][0]["top1"], runs["fp32"][0]["top1"]))
    result["layers"] = _child(["--leg", "layers", "--batch", str(args.batch), "--layer-reps", str(args.layer_reps)])
    print("%-14s %10s %10s   runs" % ("forward", "median ms", "spread ms"))
    for name, v in result["forward_ms"].items():
        print("%-14s %10.3f %10.3f   %s" % (name, v["median"], v["spread"], v["runs"]))
    print("\n%-18s %-34s %-28s %16s %16s %8s %8s" % ("layer", "shape", "fp32 family", "fp32 ms", "bf16 ms", "TFLOP/s", "GB/s"))
    for r in result["layers"]:
        slower = " SLOWER" if min(r["bf16_ms"]) > min(r["fp32_ms"]) else ""
        print("%-18s %-34s %-28s %16s %16s %8.1f %8.0f%s" % (r["layer"], "x".join(map(str, r["shape"])), r["fp32_family"],
                                                            r["fp32_ms"], r["bf16_ms"], r["bf16_tflops"], r["bf16_gbs"], slower))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
