#!/usr/bin/env python
"""What the device route of the segmentation-list loader buys, at DeepLab's shape: batches of
8 x 3 x 513 x 513 with flip, shift (40, 40), scale (0.75, 1.25) and rotation 20 all on.

  case    leg            what it is
  label   host           libbip's bip_warp_label_map over the 8 masks of a batch, one after the other: wall clock
          device         bcnn_hip_augment_label_batch, the copy of its staging block included: between device events
          copy           a pinned host-to-device copy of as many bytes as that block holds, alone: between device events
                         (device - copy estimates the kernel alone; its bytes/s are over the minimum traffic of 1 byte
                         read and 4 bytes written per pixel)
  next    host / device  a whole bcnn_loader_next + bcnn_synchronize on a conv -> softmax-loss net fed from 16 PPM / PGM
                         pairs of 513 x 513 (no crop, cheap decode: the routes differ in the pixel and label work), with
                         bcnn_set_loader_on_device off / on: wall clock

Every (case, leg, repeat) runs in a fresh process; a leg warms up for at least 80 ms and 3 calls, then times --iters calls.
The summary is the median over the processes with the spread (min, max). A process that finds no device fails.

    python tools/loader_segmentation_time.py [--out profiles/loader_segmentation.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
N, H, W = 8, 513, 513
LEGS = (("label", "host"), ("label", "device"), ("label", "copy"), ("next", "host"), ("next", "device"))
SEG = 6


def _records(np, L):
    """8 records with all four stages and their taps, from the loader's own fill_record"""
    fn = L.bcnn_loader_fill_record
    fn.restype = None
    fn.argtypes = [C.c_int] * 5 + [C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rs = np.random.RandomState(3)
    recs, taps = np.zeros((N, 8), np.int32), np.zeros((N, (W + H) * 2), np.int32)
    for b in range(N):
        fn(1, 1, int(rs.randint(-20, 21)), int(rs.randint(-20, 21)), 1, float(rs.uniform(0.75, 1.25)), 1,
           float(rs.uniform(-0.17, 0.17)), W, H, recs[b].ctypes.data, taps[b].ctypes.data)
    return recs, taps


def _timed(fn, iters, sync):
    t0, warm = time.perf_counter(), 0
    while warm < 3 or time.perf_counter() - t0 < MIN_WARM_S:
        fn()
        sync()
        warm += 1
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / iters


def _label(leg, iters):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from bcnn_amd import _lib, capi, ops
    L = _lib.load()
    assert L.bcnn_hip_device_count() > 0, "no device"
    recs, taps = _records(np, capi.lib())
    maps = np.random.RandomState(1).randint(0, 21, (N, H, W)).astype(np.uint8)
    label = torch.zeros((N, 1, H, W), device="cuda:0")
    block = recs.nbytes + taps.nbytes + maps.nbytes
    out = {"case": "label", "leg": leg, "shape": [N, 1, H, W], "iters": iters, "block_bytes": block,
           "min_bytes": 5 * N * H * W}
    if leg == "host":
        out["ms"] = _timed(lambda: [ops.warp_label_map(maps[b], recs[b], taps[b], 255) for b in range(N)], iters, lambda: None)
        out["clock"] = "wall"
    else:
        if leg == "device":
            fn = lambda: ops.augment_label_batch(label, maps, recs, taps, 255)   # noqa: E731
        else:
            src = torch.empty(block, dtype=torch.uint8).pin_memory()
            dst = torch.empty(block, dtype=torch.uint8, device="cuda:0")
            fn = lambda: dst.copy_(src, non_blocking=True)   # noqa: E731
        _timed(fn, 3, torch.cuda.synchronize)
        if leg == "device":
            L.bcnn_hip_trace_enable(1)
            assert fn() == 0
            torch.cuda.synchronize()
            size = L.bcnn_hip_trace_read(None, 0)
            buf = C.create_string_buffer(size + 1)
            L.bcnn_hip_trace_read(buf, size + 1)
            L.bcnn_hip_trace_enable(0)
            out["kernels"] = buf.value.decode().split()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out["ms"] = e0.elapsed_time(e1) / iters
        out["clock"] = "device events"
    print(json.dumps(out), flush=True)


def _next(leg, iters):
    sys.path.insert(0, ROOT)
    import numpy as np
    from bcnn_amd import capi
    with tempfile.TemporaryDirectory() as d:
        rs = np.random.RandomState(2)
        rows = []
        for k in range(16):
            pi, pm = os.path.join(d, "im%d.ppm" % k), os.path.join(d, "mask%d.pgm" % k)
            with open(pi, "wb") as f:
                f.write(b"P6\n%d %d\n255\n" % (W, H) + rs.randint(0, 256, (H, W, 3)).astype(np.uint8).tobytes())
            with open(pm, "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (W, H) + rs.randint(0, 21, (H, W)).astype(np.uint8).tobytes())
            rows.append("%s %s" % (pi, pm))
        lst = os.path.join(d, "seg.txt")
        with open(lst, "w") as f:
            f.write("\n".join(rows) + "\n")
        cfg = os.path.join(d, "seg.cfg")
        with open(cfg, "w") as f:
            f.write("[net]\ninput_width=%d\ninput_height=%d\ninput_channels=3\nbatch_size=%d\nflip_h=1\nrange_shift_x=40\n"
                    "range_shift_y=40\nmin_scale=0.75\nmax_scale=1.25\nrotation_range=20\n\n[conv]\nfilters=21\nsize=1\nstride=1\n"
                    "pad=0\nactivation=linear\nsrc=input\ndst=c1\n\n[softmax_loss]\nignore_label=255\nsrc=c1\ndst=prob\n" % (W, H, N))
        net = capi.Net.load_net(cfg, None, mode=capi.MODE_TRAIN)
        assert net.set_loader_on_device(leg == "device") == 0
        net.compile()
        assert net.set_data_loader(SEG, lst) == 0
        net.L.bcnn_augment_data_with_flip.argtypes = [C.c_void_p, C.c_int, C.c_int]
        net.L.bcnn_augment_data_with_flip(net.net, 1, 0)
        capi._libc.srand(1)

        def fn():
            assert net.loader_next() == 0

        ms = _timed(fn, iters, net.sync)
        print(json.dumps({"case": "next", "leg": leg, "shape": [N, 3, H, W], "iters": iters, "ms": ms, "clock": "wall",
                          "device_labels": net.loader_device_labels()}), flush=True)
        net.close()


def _child(case, leg, iters):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--leg", leg, "--iters", str(iters)],
                       capture_output=True, text=True, cwd=ROOT, timeout=240)   # a hung child ends the whole run
    if r.returncode != 0:
        raise SystemExit("%s %s failed (%d):\n%s\n%s" % (case, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return [json.loads(line) for line in r.stdout.strip().splitlines() if line.startswith("{")][-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the raw record as JSON here")
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        (_label if a.case == "label" else _next)(a.leg, a.iters)
        return
    runs = []
    for rep in range(a.repeats):   # alternating: every leg once per round
        for case, leg in LEGS:
            r = _child(case, leg, a.iters)
            r["repeat"] = rep
            runs.append(r)
            print("%-6s %-7s rep %d  %9.4f ms" % (case, leg, rep, r["ms"]), flush=True)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    summary = {}
    for case, leg in LEGS:
        mine = [r["ms"] for r in runs if r["case"] == case and r["leg"] == leg]
        summary["%s_%s" % (case, leg)] = {"ms": med(mine), "ms_spread": [min(mine), max(mine)]}
    first = [r for r in runs if r["case"] == "label" and r["leg"] == "device"][0]
    kernel_ms = summary["label_device"]["ms"] - summary["label_copy"]["ms"]
    summary["label_device"]["kernels"] = first.get("kernels")
    summary["label_kernel_estimate"] = {"ms": kernel_ms, "min_bytes": first["min_bytes"],
                                        "gbps": first["min_bytes"] / kernel_ms * 1e-6 if kernel_ms > 0 else None,
                                        "is": "label_device - label_copy"}
    summary["ratios"] = {"label_host_over_device": summary["label_host"]["ms"] / summary["label_device"]["ms"],
                         "next_host_over_device": summary["next_host"]["ms"] / summary["next_device"]["ms"]}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/loader_segmentation_time.py", "iters": a.iters, "repeats": a.repeats, "summary": summary,
                       "runs": runs}, fh, indent=1)


if __name__ == "__main__":
    main()
