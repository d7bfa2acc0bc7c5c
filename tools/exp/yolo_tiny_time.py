#!/usr/bin/env python3
"""yolov3-tiny PREDICT forward at 416 x 416 (N = 1 and N = 32, random Darknet weights) and the achieved HBM bandwidth of
the detector-graph kernels on large memory-bound cases: concat of two 64 x 128 x 104 x 104 sources and upsample
64 x 128 x 52 x 52 -> 104 x 104, forward and backward. Device events on the library's stream, after warm-up.
    python tools/exp/yolo_tiny_time.py [--reps 20]
--post: instead, the cost of getting a batch's boxes out after the N = 32 forward: 32 calls of bcnn_yolo_get_detections
against one bcnn_yolo_get_detections_batch, wall clock around the calls (their synchronisation included), three
alternating repeats; the raw record goes to --out (default profiles/detect_postprocess_n32.json).
    python tools/exp/yolo_tiny_time.py --post [--candidates 300]
--pre: instead, the cost of getting a batch's frames in before the N = 32 forward: per image a host resize, a canvas paste
and bcnn_fill_tensor_with_image (which uploads the whole tensor each time) against one bcnn_fill_tensor_with_images, both
ended by bcnn_synchronize, wall clock, three alternating repeats; the raw record goes to --out (default
profiles/input_fill_n32.json).
    python tools/exp/yolo_tiny_time.py --pre
--train: instead, one training step of yolov3-tiny at N = 32 with detector training on (bcnn_set_detector_training): eight
truths per image, forward + backward + SGD update on device events, and the TRAIN forward of the two heads alone
(bcnn_forward_node); the raw record goes to --out (default profiles/detect_train_step_n32.json).
    python tools/exp/yolo_tiny_time.py --train
Under rocprofv3:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/exp/yolo_tiny_time.py"""
import argparse
import json
import os
import sys
import statistics
import tempfile
import time

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


class YoloHead(C.Structure):
    """struct bcnn_hip_yolo_head (include/bcnn_hip.h)"""
    _fields_ = [("out_d", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("num", C.c_int), ("coords", C.c_int),
                ("classes", C.c_int), ("anchor_w", C.c_float * 16), ("anchor_h", C.c_float * 16)]


def post(L, reps, tmp, n, want, out_path):
    """after one forward of yolov3-tiny at N = n: (i) n calls of bcnn_yolo_get_detections, (ii) one
    bcnn_yolo_get_detections_batch; `want` candidates per image on average set the threshold"""
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
    fwd_ms = timed(L, net.forward, reps)
    net.forward()
    net.sync()
    _, _, neth, netw = net.shape(0)
    # the heads: their activated objectness (read back once, outside every timed region) sets the threshold
    heads, objectness, head_bytes = [], [], 0
    for k in range(net.num_nodes):
        y, src = net.node_dst(k), net.node_src(k, 0)
        if y == src or net.shape(y)[1] != 255 or net.shape(src) != net.shape(y):
            continue  # a head copies its 255-channel source (the convolution in front reads 512 / 256 channels)
        net.download(y, with_grad=False)
        nn, c, h, w = net.shape(y)
        num = 3
        per = c // num
        objectness.append(net.data(y).reshape(nn, num, per, h * w)[:, :, 4].reshape(nn, -1).copy())
        head_bytes += 4 * nn * c * h * w
        heads.append((net.tensor(y).data_gpu, h, w, num, 4, per - 5))
    assert len(heads) == 2, "yolov3-tiny has two heads"
    obj = np.concatenate(objectness, 1)
    thresh = float(np.sort(obj.reshape(-1))[::-1][min(obj.size - 1, want * n)])
    counts = (obj > thresh).sum(1)
    print("threshold %.6f: candidates per image %s" % (thresh, " ".join(str(int(v)) for v in counts)))
    sizes = [(640 + 8 * (b % 5), 480 - 8 * (b % 3)) for b in range(n)]
    ws, hs = (C.c_int * n)(*[s[0] for s in sizes]), (C.c_int * n)(*[s[1] for s in sizes])
    NL = net.L

    def per_image():
        res = []
        t0 = time.perf_counter()
        for b in range(n):
            cnt = C.c_int(0)
            res.append((NL.bcnn_yolo_get_detections(net.net, b, sizes[b][0], sizes[b][1], netw, neth, thresh, 0,
                                                    C.byref(cnt)), cnt))
        dt = time.perf_counter() - t0
        got = [c.value for _, c in res]
        for d, c in res:
            NL.bcnn_free_detections(d, c.value)
        return dt * 1e3, got

    def batch():
        dets, cnts = (C.POINTER(capi.Detection) * n)(), (C.c_int * n)()
        t0 = time.perf_counter()
        st = NL.bcnn_yolo_get_detections_batch(net.net, ws, hs, netw, neth, thresh, 0, dets, cnts)
        dt = time.perf_counter() - t0
        assert st == 0, st
        got = list(cnts)
        for b in range(n):
            NL.bcnn_free_detections(dets[b], cnts[b])
        return dt * 1e3, got

    for _ in range(3):  # warm-up (the batch call also settles its record capacity here)
        per_image()
        batch()
    rec_i, rec_ii = [], []
    for _ in range(3):
        ms, got_i = per_image()
        rec_i.append(ms)
        ms, got_ii = batch()
        rec_ii.append(ms)
        assert got_i == got_ii == [int(v) for v in counts], (got_i, got_ii)
    # device events around the C-ABI entry alone: the two kernels and the copy of the result block
    anchors = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
    tab = (YoloHead * 2)()
    for k, (ptr, h, w, num, coords, classes) in enumerate(heads):
        mask = (3, 4, 5) if k == 0 else (0, 1, 2)
        tab[k].out_d, tab[k].h, tab[k].w, tab[k].num, tab[k].coords, tab[k].classes = ptr, h, w, num, coords, classes
        for a, m in enumerate(mask):
            tab[k].anchor_w[a], tab[k].anchor_h[a] = anchors[2 * m], anchors[2 * m + 1]
    # the record capacity the timed batch calls ran with (bcnn_layers_detect.c: 256, or 1.25 x the largest count of the
    # net's previous call -- the warm-up calls, with these same counts)
    cap = max(256, int(max(counts)) + int(max(counts)) // 4)
    classes = heads[0][5]
    words = L.bcnn_hip_yolo_detect_result_words(n, cap, classes)
    result = (C.c_int * words)()
    geom = (C.c_int * (4 * n))()
    for b, (w, h) in enumerate(sizes):
        new_w, new_h = (netw, (h * netw) // w) if netw / w < neth / h else ((w * neth) // h, neth)
        geom[4 * b:4 * b + 4] = [w, h, new_w, new_h]
    dev_ms = timed(L, lambda: L.bcnn_hip_yolo_detect_batch(tab, 2, n, geom, netw, neth, netw, neth, thresh, 0, 0.45, cap,
                                                           0, result), reps)
    assert list(result[:n]) == [int(v) for v in counts]
    # what the copy of the result block alone costs: the same bytes, device to pageable host memory, synchronised
    block = L.bcnn_hip_malloc_f32(words)
    for _ in range(3):
        L.bcnn_hip_memcpy_d2h(result, block, 4 * words)
    t0 = time.perf_counter()
    for _ in range(reps):
        L.bcnn_hip_memcpy_d2h(result, block, 4 * words)
    copy_ms = (time.perf_counter() - t0) * 1e3 / reps
    L.bcnn_hip_free(block)
    net.close()
    res = dict(device=torch.cuda.get_device_name(0), workload="yolov3-tiny 416x416 N=%d, random Darknet weights" % n,
               threshold=thresh, candidates_per_image=[int(v) for v in counts], forward_ms=fwd_ms,
               per_image_calls_ms=rec_i, batch_call_ms=rec_ii,
               per_image_calls_median_ms=statistics.median(rec_i), batch_call_median_ms=statistics.median(rec_ii),
               per_image_calls_spread_ms=max(rec_i) - min(rec_i), batch_call_spread_ms=max(rec_ii) - min(rec_ii),
               kernels_and_copy_device_ms=dev_ms, result_copy_alone_wall_ms=copy_ms,
               pcie_bytes_per_image_calls=n * head_bytes, pcie_bytes_batch_call=4 * (words + 4 * n),
               record_capacity=cap)
    print("forward %.3f ms | %d per-image calls: median %.3f ms (spread %.3f) | one batch call: median %.3f ms "
          "(spread %.3f) | kernels + copy on the device %.3f ms | the copy alone %.3f ms wall" %
          (fwd_ms, n, res["per_image_calls_median_ms"], res["per_image_calls_spread_ms"], res["batch_call_median_ms"],
           res["batch_call_spread_ms"], dev_ms, copy_ms))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fp:
        json.dump(res, fp, indent=1)
        fp.write("\n")
    print(json.dumps(res))


def pre(L, reps, tmp, n, out_path, fw=640, fh=480):
    """n random fw x fh x 3 frames into the input of yolov3-tiny at N = n, letterbox fit: (A) the host path, per image
    bip_resize_bilinear, paste onto a canvas of 128, bcnn_fill_tensor_with_image; (B) one bcnn_fill_tensor_with_images"""
    cfg = os.path.join(tmp, "tiny%d.cfg" % n)
    with open(cfg, "w") as fp:
        fp.write(tiny_cfg(batch=n))
    model = os.path.join(tmp, "tiny.weights")
    if not os.path.exists(model):
        write_tiny_weights(model)
    net = capi.Net.load_net(cfg, model, capi.MODE_PREDICT)
    net.compile()
    NL = net.L
    _, c, H, W = net.shape(0)
    u8p = C.POINTER(C.c_uint8)
    bip = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libbip.so"))
    bip.bip_resize_bilinear.argtypes = [u8p] + [C.c_size_t] * 3 + [u8p] + [C.c_size_t] * 4
    NL.bcnn_fill_tensor_with_image.argtypes = [C.c_void_p, u8p] + [C.c_int] * 3 + [C.c_float, C.c_int] + [C.c_float] * 3 + \
        [C.c_int] * 2
    NL.bcnn_fill_tensor_with_image.restype = C.c_int
    rs = np.random.RandomState(0)
    frames = [rs.randint(0, 256, (fh, fw, c)).astype(np.uint8) for _ in range(n)]
    new_w, new_h = (W, (fh * W) // fw) if np.float32(W) / np.float32(fw) < np.float32(H) / np.float32(fh) else \
        ((fw * H) // fh, H)
    xo, yo = (W - new_w) // 2, (H - new_h) // 2
    norm = 1.0 / 255.0
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
    ws, hs = (C.c_int * n)(*[fw] * n), (C.c_int * n)(*[fh] * n)

    def host_path():
        t0 = time.perf_counter()
        for b in range(n):
            small = np.empty((new_h, new_w, c), np.uint8)
            bip.bip_resize_bilinear(frames[b].ctypes.data_as(u8p), fw, fh, fw * c, small.ctypes.data_as(u8p), new_w, new_h,
                                    new_w * c, c)
            canvas = np.full((H, W, c), 128, np.uint8)
            canvas[yo:yo + new_h, xo:xo + new_w] = small
            st = NL.bcnn_fill_tensor_with_image(net.net, canvas.ctypes.data_as(u8p), W, H, c, norm, 1, 0.0, 0.0, 0.0, 0, b)
            assert st == 0, st
        net.sync()
        return (time.perf_counter() - t0) * 1e3

    def device_path():
        t0 = time.perf_counter()
        st = NL.bcnn_fill_tensor_with_images(net.net, 0, n, ptrs, ws, hs, None, c, capi.IMAGE_FIT_LETTERBOX, norm, 1,
                                             0.0, 0.0, 0.0)
        net.sync()
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0, st
        return dt

    def device_tensor():
        net.download(0, with_grad=False)
        return net.data(0).copy()

    for _ in range(3):  # warm-up: code objects, the pinned and the device staging blocks at their final size
        host_path()
        device_path()
    rec_a, rec_b = [], []
    for _ in range(3):
        rec_a.append(host_path())
        x_a = device_tensor()
        rec_b.append(device_path())
        x_b = device_tensor()
        assert np.array_equal(x_a.view(np.uint32), x_b.view(np.uint32)), "the two legs fill the tensor differently"
    # device events around the C-ABI entry alone: the staging copy and the kernel (the host packing overlaps neither)
    x_d = net.tensor(0).data_gpu
    dev_ms = timed(L, lambda: L.bcnn_hip_fill_images(x_d, n, c, H, W, n, ptrs, ws, hs, None, capi.IMAGE_FIT_LETTERBOX,
                                                     norm, 1, 0.0, 0.0, 0.0), reps)
    fwd_ms = timed(L, net.forward, reps)
    net.close()
    align = lambda v: (v + 15) // 16 * 16  # noqa: E731
    staged = align(n * 36) + n * (W + H) * 8 + n * align(fw * fh * c)   # descriptors, tap tables, pixels (image_fill.hip)
    res = dict(device=torch.cuda.get_device_name(0),
               workload="yolov3-tiny %dx%d N=%d, random %dx%dx%d frames, letterbox" % (W, H, n, fw, fh, c),
               forward_ms=fwd_ms, host_path_ms=rec_a, device_path_ms=rec_b,
               host_path_median_ms=statistics.median(rec_a), device_path_median_ms=statistics.median(rec_b),
               host_path_spread_ms=max(rec_a) - min(rec_a), device_path_spread_ms=max(rec_b) - min(rec_b),
               copy_and_kernel_device_ms=dev_ms, pcie_bytes_host_path=n * n * c * H * W * 4, pcie_bytes_device_path=staged,
               results_bit_identical=True)
    print("forward %.3f ms | host path (%d fills): median %.3f ms (spread %.3f) | one device fill: median %.3f ms "
          "(spread %.3f) | its copy + kernel on the device %.3f ms" %
          (fwd_ms, n, res["host_path_median_ms"], res["host_path_spread_ms"], res["device_path_median_ms"],
           res["device_path_spread_ms"], dev_ms))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fp:
        json.dump(res, fp, indent=1)
        fp.write("\n")
    print(json.dumps(res))


def train(L, reps, tmp, n, out_path):
    """one SGD step of yolov3-tiny at N = n, and the share of the heads' TRAIN forward in it"""
    cfg = os.path.join(tmp, "tiny_train%d.cfg" % n)
    with open(cfg, "w") as fp:
        fp.write(tiny_cfg(batch=n).replace("[net]\n", "[net]\ntrain_detector=1\n", 1))
    model = os.path.join(tmp, "tiny.weights")
    if not os.path.exists(model):
        write_tiny_weights(model)
    net = capi.Net.load_net(cfg, model, capi.MODE_TRAIN)
    net.compile()
    net.set_sgd(1e-5, 0.9, 5e-4)
    rs = np.random.RandomState(0)
    net.data(0)[...] = rs.uniform(0, 1, net.shape(0)).astype(np.float32)
    net.upload(0)
    lab = np.zeros((n, 50, 5), np.float32)
    lab[:, :8, 0:2] = rs.uniform(0.05, 0.95, (n, 8, 2))
    lab[:, :8, 2:4] = rs.uniform(0.03, 0.6, (n, 8, 2))
    lab[:, :8, 4] = rs.randint(0, 80, (n, 8))
    net.data(1)[...] = lab.reshape(net.shape(1))
    net.upload(1)
    heads = []
    stats = capi.YoloTrainStats()
    for node in range(net.num_nodes):
        if net.L.bcnn_yolo_get_train_stats(net.net, node, C.byref(stats)) == 0:
            heads.append(node)

    def step():
        net.forward()
        net.backward()
        net.update()

    step_ms = timed(L, step, reps)
    fwd_ms = timed(L, net.forward, reps)
    heads_ms = timed(L, lambda: [net.forward_node(h) for h in heads], reps)
    got = [net.yolo_train_stats(h) for h in heads]
    net.close()
    rec = dict(device=torch.cuda.get_device_name(0), n=n, reps=reps, step_ms=step_ms, forward_ms=fwd_ms,
               heads_train_forward_ms=heads_ms, heads=len(heads), truths_assigned=[g["count"] for g in got])
    print("yolov3-tiny 416x416 TRAIN N=%d: step %.3f ms (%.0f img/s), forward %.3f ms, TRAIN forward of the %d heads %.3f ms"
          % (n, step_ms, n / step_ms * 1e3, fwd_ms, len(heads), heads_ms))
    with open(out_path, "w") as fp:
        json.dump(rec, fp, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--post", action="store_true", help="time the detection post-processing after the N = 32 forward")
    ap.add_argument("--candidates", type=int, default=300, help="--post: candidates per image the threshold leaves")
    ap.add_argument("--pre", action="store_true", help="time the input fill before the N = 32 forward")
    ap.add_argument("--train", action="store_true", help="time one training step of yolov3-tiny at N = 32")
    ap.add_argument("--out", default=None, help="--post / --pre / --train: where the raw record goes")
    args = ap.parse_args()
    L = _lib.load()
    if args.pre:
        with tempfile.TemporaryDirectory() as tmp:
            pre(L, args.reps, tmp, 32, args.out or os.path.join(ROOT, "profiles", "input_fill_n32.json"))
        return
    if args.train:
        with tempfile.TemporaryDirectory() as tmp:
            train(L, args.reps, tmp, 32, args.out or os.path.join(ROOT, "profiles", "detect_train_step_n32.json"))
        return
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "detect_postprocess_n32.json")
    if args.post:
        with tempfile.TemporaryDirectory() as tmp:
            post(L, args.reps, tmp, 32, args.candidates, args.out)
        return
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
