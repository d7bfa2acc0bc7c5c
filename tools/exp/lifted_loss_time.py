#!/usr/bin/env python3
"""Lifted-structure loss (lifted_loss.hip): time of forward + backward of the cost node's device work (7 + 1 launches) per
(B, K), and beside it the floor any implementation of the closed form pays on this library: the two bcnn_hip_gemm calls
of the same shapes, x x^T (B x B x K) and A x (B x K x B). Device events on the library's stream after warm-up; the
repetitions are sized so that every timed window holds at least ~50 ms of work.
    python tools/exp/lifted_loss_time.py [--min-ms 50]
Under rocprofv3 (kernel and copy trace, no counters in the same run):
    rocprofv3 --kernel-trace --memory-copy-trace --stats -d <dir> -- python tools/exp/lifted_loss_time.py --net-steps 5
--net-steps N runs N TRAIN steps of an fc -> lifted cost net (B = 512, K = 128) instead of the table, so that the trace
shows every copy a step makes."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime for torch and the library)

from bcnn_amd import _lib, capi, ops  # noqa: E402

BS = (64, 128, 256, 512, 1024, 2048)
KS = (64, 128, 512)


def timed(L, fn, min_ms, warm=3):
    e0, e1 = L.bcnn_hip_event_create(), L.bcnn_hip_event_create()
    for _ in range(warm):
        fn()
    L.bcnn_hip_sync()
    reps, ms = 20, 0.0
    while True:
        L.bcnn_hip_event_record(e0)
        for _ in range(reps):
            fn()
        L.bcnn_hip_event_record(e1)
        L.bcnn_hip_event_sync(e1)
        ms = L.bcnn_hip_event_elapsed_ms(e0, e1)
        if ms >= min_ms or reps >= 20000:
            break
        reps = int(reps * max(2.0, 1.2 * min_ms / max(ms, 1e-3)))
    L.bcnn_hip_event_destroy(e0)
    L.bcnn_hip_event_destroy(e1)
    return ms / reps


def table(L, min_ms):
    print("%5s %5s %10s %10s %10s %7s" % ("B", "K", "node ms", "gram gemm", "A.x gemm", "ratio"), flush=True)
    for B in BS:
        for K in KS:
            g = torch.Generator(device="cuda").manual_seed(B + K)
            x = torch.randn((B, K), device="cuda", generator=g)
            cls = torch.randint(0, 8, (B,), device="cuda", generator=g)
            lab = torch.zeros((B, K), device="cuda")
            lab[torch.arange(B, device="cuda"), cls] = 1
            grad = torch.zeros((B, K), device="cuda")
            rec = torch.zeros(2, dtype=torch.int32, device="cuda")
            ws = torch.empty(ops.lifted_struct_workspace_size(B, K), device="cuda")
            gram = torch.empty((B, B), device="cuda")
            amat = torch.randn((B, B), device="cuda", generator=g)
            torch.cuda.synchronize()

            def node():
                ops.lifted_struct_forward(x, lab, grad, rec, ws, 1.0, False)
                ops.lifted_struct_backward(grad, rec, 1.0)
            t_node = timed(L, node, min_ms)
            t_gram = timed(L, lambda: ops.gemm(0, 1, B, B, K, 1.0, x, K, x, K, 0.0, gram, B), min_ms)
            t_ax = timed(L, lambda: ops.gemm(0, 0, B, K, B, 1.0, amat, B, x, K, 0.0, grad, K), min_ms)
            print("%5d %5d %10.4f %10.4f %10.4f %7.2f" % (B, K, t_node, t_gram, t_ax, t_node / (t_gram + t_ax)),
                  flush=True)


def net_steps(n, B=512, K=128):
    net = capi.Net(mode=capi.MODE_TRAIN, w=1, h=1, c=K, n=B)
    net.fullc(K, src="input", dst="fc")
    net.cost("fc", dst="out", loss=capi.LOSS_LIFTED_STRUCT)
    net.compile()
    net.set_sgd(0.01, 0.9)
    rs = np.random.RandomState(0)
    net.data(0)[...] = rs.randn(B, K, 1, 1)
    lab = np.zeros((B, K), np.float32)
    lab[np.arange(B), rs.randint(0, 8, B)] = 1
    net.data(1)[...] = lab.reshape(B, K, 1, 1)
    net.upload(0)
    net.upload(1)
    for _ in range(n):
        net.forward()
        net.backward()
        net.update()
    net.sync()
    print("loss %.6f pairs %d after %d steps" % (net.lifted_struct_loss() + (n,)))
    net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-ms", type=float, default=50.0)
    ap.add_argument("--net-steps", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lifted_loss_time.py measures on the GPU; none found")
    if a.net_steps:
        net_steps(a.net_steps)
    else:
        table(_lib.load(), a.min_ms)


if __name__ == "__main__":
    main()
