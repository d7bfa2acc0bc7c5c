#!/usr/bin/env python3
"""LRN and dropout (lrn_dropout.hip): time per call and the fraction of the 8 TB/s HBM peak, counting the algorithmic
bytes -- LRN forward reads x and writes y (2 passes), LRN backward reads x and dy and writes dx (overwrite, 3 passes),
dropout reads and writes x in place (2 passes). AlexNet's LRN shapes (N = 128, n = 5) and a 4096-wide fc dropout at
N = 128, plus small shapes where the channels are split into chunks. Device events on the library's stream after
warm-up.
    python tools/exp/lrn_dropout_time.py [--reps 50]
Under rocprofv3:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/exp/lrn_dropout_time.py --reps 10"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: one HIP runtime for torch and the library)

from bcnn_amd import _lib, ops  # noqa: E402

PEAK = 8.0e12
LRN_SHAPES = [  # name, n, c, h, w, local_size
    ("alexnet_norm1_96x55x55", 128, 96, 55, 55, 5),
    ("alexnet_norm2_256x27x27", 128, 256, 27, 27, 5),
    ("n32_256x28x28_vec", 32, 256, 28, 28, 5),
    ("n8_256x13x13_chunked", 8, 256, 13, 13, 5),
]
DROP_SHAPES = [("fc_4096_n128", 128 * 4096), ("conv_256x27x27_n128", 128 * 256 * 27 * 27)]


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


def row(name, what, ms, nbytes):
    bw = nbytes / (ms * 1e-3)
    print("%-28s %-8s %9.3f %9.2f %7.3f" % (name, what, ms, bw / 1e12, bw / PEAK), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    L = _lib.load()
    print("%-28s %-8s %9s %9s %7s" % ("shape", "pass", "ms", "TB/s", "of pk"))
    for name, n, c, h, w, ls in LRN_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.rand((n, c, h, w), device="cuda", generator=g) * 2 - 1
        dy = torch.rand((n, c, h, w), device="cuda", generator=g) - 0.5
        y, dx = torch.empty_like(x), torch.empty_like(x)
        b = x.numel() * 4
        row(name, "lrn_fwd", timed(L, lambda: ops.lrn_forward(x, y, ls, 1e-4, 0.75, 1.0), a.reps), 2 * b)
        row(name, "lrn_bwd", timed(L, lambda: ops.lrn_backward(x, dy, dx, ls, 1e-4, 0.75, 1.0, 1), a.reps), 3 * b)
        del x, dy, y, dx
    for name, size in DROP_SHAPES:
        x = torch.rand(size, device="cuda") - 0.5
        step = [0]

        def fwd():
            ops.dropout_forward(x, 0.5, 12345, step[0])
            step[0] += 1
        row(name, "dropout", timed(L, fwd, a.reps), 2 * size * 4)
        del x


if __name__ == "__main__":
    main()
