#!/usr/bin/env python3
"""yolov3-tiny PREDICT forward at 416 x 416 (N = 1 and N = 32, random Darknet weights) and the achieved HBM bandwidth of
the detector-graph kernels on large memory-bound cases: concat of two 64 x 128 x 104 x 104 sources and upsample
64 x 128 x 52 x 52 -> 104 x 104, forward and backward. Device events on the library's stream, after warm-up.
    python tools/exp/yolo_tiny_time.py [--reps 20]
Under rocprofv3:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/exp/yolo_tiny_time.py"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: one HIP runtime for torch and the library)

from bcnn_amd import _lib, capi  # noqa: E402
from tests.test_yolov3_tiny import tiny_cfg, write_tiny_weights  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X


def timed(L, fn, reps, warm=3):
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    for _ in range(warm):
        fn()
    L.bcnn_hip_sync()
    L.bcnn_hip_event_record(e0)
    for _ in range(reps):
        fn()
    L.bcnn_hip_event_record(e1)
    L.bcnn_hip_event_sync(e1)
    ms = L.bcnn_hip_event_elapsed_ms(e0, e1) / reps
    L.bcnn_hip_event_destroy(e0)
    L.bcnn_hip_event_destroy(e1)
    return ms


def tiny_forward(L, n, reps, tmp):
    cfg = os.path.join(tmp, "tiny%d.cfg" % n)
    with open(cfg, "w") as fp:
        fp.write(tiny_cfg(batch=n))
    model = os.path.join(tmp, "tiny.weights")
    if not os.path.exists(model):
        write_tiny_weights(model)
    net = capi.Net.load_net(cfg, model, capi.MODE_PREDICT)
    net.compile()
    net.data(0)[...] = np.random.RandomState(0).uniform(0, 1, net.shape(0)).astype(np.float32)
    net.upload(0)
    ms = timed(L, net.forward, reps)
    net.close()
    return ms


def bandwidth(L, reps):
    f4 = 4
    out = {}
    n, c, h, w = 64, 128, 104, 104
    s = n * c * h * w
    a, b = torch.randn(s, device="cuda"), torch.randn(s, device="cuda")
    y = torch.empty(2 * s, device="cuda")
    ga, gb = torch.randn(s, device="cuda"), torch.randn(s, device="cuda")
    src = (C.c_void_p * 2)(a.data_ptr(), b.data_ptr())
    grd = (C.c_void_p * 2)(ga.data_ptr(), gb.data_ptr())
    sizes = (C.c_int * 2)(c * h * w, c * h * w)
    ms = timed(L, lambda: L.bcnn_hip_concat_forward(2, src, sizes, y.data_ptr(), 2 * c * h * w, n), reps)
    out["concat_fwd"] = dict(ms=ms, bytes=4 * s * f4)              # read 2 s, write 2 s
    ms = timed(L, lambda: L.bcnn_hip_concat_backward(2, grd, sizes, y.data_ptr(), 2 * c * h * w, n), reps)
    out["concat_bwd"] = dict(ms=ms, bytes=6 * s * f4)              # read dy 2 s, read + write dx 2 s each
    del a, b, y, ga, gb
    uh, uw = 52, 52
    su = n * c * uh * uw
    x, yu = torch.randn(su, device="cuda"), torch.empty(4 * su, device="cuda")
    ms = timed(L, lambda: L.bcnn_hip_upsample_forward(x.data_ptr(), yu.data_ptr(), n, c, uh, uw, 2), reps)
    out["upsample_fwd"] = dict(ms=ms, bytes=5 * su * f4)           # read s, write 4 s
    ms = timed(L, lambda: L.bcnn_hip_upsample_backward(x.data_ptr(), yu.data_ptr(), n, c, uh, uw, 2), reps)
    out["upsample_bwd"] = dict(ms=ms, bytes=6 * su * f4)           # read dy 4 s, read + write dx
    for v in out.values():
        v["GBps"] = v["bytes"] / (v["ms"] * 1e-3) / 1e9
        v["of_peak"] = v["GBps"] * 1e9 / HBM_PEAK
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    L = _lib.load()
    res = {"device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        for n in (1, 32):
            ms = tiny_forward(L, n, args.reps, tmp)
            res["yolov3_tiny_416_N%d_ms" % n] = ms
            print("yolov3-tiny 416x416 PREDICT forward  N=%-3d %8.3f ms  (%.1f img/s)" % (n, ms, n / ms * 1e3))
    bw = bandwidth(L, args.reps)
    for k, v in bw.items():
        print("%-13s %8.3f ms  %7.1f GB/s  %.2f of 8 TB/s" % (k, v["ms"], v["GBps"], v["of_peak"]))
    res["bandwidth"] = bw
    print(json.dumps(res))


if __name__ == "__main__":
    main()
