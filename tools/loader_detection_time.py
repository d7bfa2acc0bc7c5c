#!/usr/bin/env python
"""What bcnn_set_loader_detection_on_device buys on a detection list of JPEG files:
bcnn_loader_next + bcnn_synchronize per batch, host clock, under the protocol of tools/loader_jpeg_time.py.

  workload  a detection list of 640 x 480 JPEGs (4:2:0, quality 90, encoded here by PIL as in tools/jpeg_fill_time.py),
            three boxes each, net input 416 x 416 x 3, N = 32, TRAIN mode, flip (INI key flip_h) + colour adjustment
            (-20, 20, 0.8, 1.2), the yolov3-tiny pattern of tests/test_yolo_train_graph.py (two heads) behind it
  legs      parent    a built checkout of the parent commit (--parent-tree DIR; left out when not given): the host path
            off       this tree, the new switch off: has to match the parent within the spread of the repeats
            on_t1     this tree, loader_on_device and loader_detection_on_device on, bcnn_set_num_threads(1)
            on_t16    the same with 16 host threads
  and, end to end with no bar, bcnn_train_on_batch images/s of the same graph: parent against on_t16 (--train-steps 0
  leaves it out; without a parent tree, off against on_t16).

Every leg runs in a process of its own (the parent tree brings its own bcnn_amd package), the legs alternate, and each is
repeated --repeats times: the spread of the repeats is what a difference has to exceed. A measurement warms up for at
least 80 ms and 3 batches, then times --batches batches. Bytes uploaded per batch are computed from the shapes: the float
input tensor on the host legs, the staging block of bcnn_hip_augment_letterbox_batch (records, sums, descriptors,
letterbox taps, the decoded images) on the others; the label tensor goes up on every leg alike.

    python tools/loader_detection_time.py [--parent-tree DIR] [--out profiles/loader_detection.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_fill_time import write_images  # noqa: E402  (the same files as the inference-side measurement)

MIN_WARM_S = 0.08
N, SIDE, CLASSES = 32, 416, 2
ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169]
LEGS = {"parent": (False, 1), "off": (False, 1), "on_t1": (True, 1), "on_t16": (True, 16)}
NET = """[net]
input_width=%d
input_height=%d
input_channels=3
batch_size=%d
train_detector=1
flip_h=1
min_contrast=0.8
max_contrast=1.2
min_brightness=-20
max_brightness=20
learning_rate=0.001
momentum=0.9
""" % (SIDE, SIDE, N)


def _leg(tree, device, threads, data, batches, train_steps):
    sys.path.insert(0, tree)
    import torch
    from bcnn_amd import capi
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    libc = C.CDLL(None)
    vp, i, f, cp = C.c_void_p, C.c_int, C.c_float, C.c_char_p
    lst = os.path.join(data, "list.txt")

    def build():
        net = capi.Net.load_net(os.path.join(data, "net.cfg"), None, mode=capi.MODE_TRAIN)   # the [net] section alone
        L = net.L
        L.bcnn_set_data_loader.argtypes = [vp, i, cp, cp, cp, cp]
        L.bcnn_loader_next.argtypes = [vp]
        L.bcnn_train_on_batch.argtypes = [vp]
        L.bcnn_train_on_batch.restype = f
        lrelu = capi.ACT_LRELU
        net.conv(8, 3, 1, 1, 1, 1, lrelu, "input", "c1")
        net.maxpool(2, 2, capi.PADDING_SAME, "c1", "p1")
        net.conv(16, 3, 1, 1, 1, 1, lrelu, "p1", "c2")
        net.maxpool(2, 2, capi.PADDING_SAME, "c2", "p2")
        net.conv(16, 3, 1, 1, 1, 1, lrelu, "p2", "c3")
        net.conv(16, 3, 1, 1, 1, 1, lrelu, "c3", "c4")
        net.conv(2 * (5 + CLASSES), 1, 1, 0, 1, 0, capi.ACT_NONE, "c4", "h1")
        net.yolo(2, CLASSES, [3, 4], ANCHORS, "h1", "yolo1")
        net.concat(["c3"], "r1")
        net.conv(8, 1, 1, 0, 1, 1, lrelu, "r1", "c5")
        net.upsample(2, "c5", "up")
        net.concat(["up", "c2"], "cat")
        net.conv(16, 3, 1, 1, 1, 1, lrelu, "cat", "c6")
        net.conv(3 * (5 + CLASSES), 1, 1, 0, 1, 0, capi.ACT_NONE, "c6", "h2")
        net.yolo(3, CLASSES, [0, 1, 2], ANCHORS, "h2", "yolo2")
        assert L.bcnn_set_data_loader(net.net, 4, lst.encode(), None, lst.encode(), None) == 0
        if device:
            assert net.set_loader_on_device(True) == 0 and net.set_loader_detection_on_device(True) == 0
        assert net.set_num_threads(threads) == 0
        net.compile()
        libc.srand(1)
        return net

    def timed(fn, count):
        t0, warm = time.perf_counter(), 0
        while warm < 3 or time.perf_counter() - t0 < MIN_WARM_S:
            fn()
            warm += 1
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        return (time.perf_counter() - t0) / count

    out = {}
    net = build()

    def one_batch():
        assert net.L.bcnn_loader_next(net.net) == 0
        net.sync()
    out["batch_ms"] = timed(one_batch, batches) * 1e3
    out["device_letterboxed"] = net.loader_device_letterboxed() if device else 0
    assert out["device_letterboxed"] == (N if device else 0), out
    if train_steps > 0:
        losses = []

        def one_step():
            losses.append(net.L.bcnn_train_on_batch(net.net))   # returns the loss: the step has finished on the device
        out["train_img_s"] = N / timed(one_step, train_steps)
        out["last_loss"] = losses[-1]
    net.close()
    print(json.dumps(out))


def upload_bytes():
    """bytes of the input's host-to-device copy of a batch, per leg kind (640 x 480 sources letterbox to 416 x 312)"""
    al = lambda v: (v + 15) // 16 * 16
    host = N * 3 * SIDE * SIDE * 4
    device = al(N * 32) + N * 16 + al(N * 36) + al(N * (416 + 312) * 8) + N * al(640 * 480 * 3)
    return {"host_letterbox": host, "device_letterbox": device}


def _child(args_list):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args_list, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("leg %s failed (%d):\n%s\n%s" % (args_list, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-tree", default=None, help="a BUILT checkout of the parent commit")
    ap.add_argument("--images", type=int, default=64, help="files in the list")
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result as JSON here")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--data", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        device, threads = LEGS[args.leg]
        return _leg(args.tree, device, threads, args.data, args.batches, args.train_steps)

    import numpy as np
    legs = [("off", ROOT), ("on_t1", ROOT), ("on_t16", ROOT)]
    if args.parent_tree:
        legs.insert(0, ("parent", os.path.abspath(args.parent_tree)))
    train_legs = ("parent", "on_t16") if args.parent_tree else ("off", "on_t16")
    runs = {name: [] for name, _ in legs}
    with tempfile.TemporaryDirectory() as data:
        source = write_images(data, args.images)
        rs = np.random.RandomState(0)
        with open(os.path.join(data, "list.txt"), "w") as fh:
            for k in range(args.images):
                boxes = " ".join("%d %.4f %.4f %.4f %.4f" % (rs.randint(CLASSES), *rs.uniform(0.2, 0.8, 2), *rs.uniform(0.05, 0.4, 2))
                                 for _ in range(3))
                fh.write("%s %s\n" % (os.path.join(data, "%03d.jpg" % k), boxes))
        with open(os.path.join(data, "net.cfg"), "w") as fh:
            fh.write(NET)
        for _ in range(args.repeats):          # alternating: whatever else the machine does hits every leg alike
            for name, tree in legs:
                train = args.train_steps if name in train_legs else 0
                runs[name].append(_child(["--leg", name, "--tree", tree, "--data", data, "--batches", str(args.batches),
                                          "--train-steps", str(train)]))
    uploaded = upload_bytes()
    result = dict(images=source, files=args.images, batch=N, input=SIDE, batches=args.batches, train_steps=args.train_steps,
                  upload_bytes_per_batch=uploaded, raw=runs, summary={})
    print("upload per batch: %s" % uploaded)
    print("%-14s %-8s %12s %12s   runs" % ("measurement", "leg", "median", "spread"))
    for key in ("batch_ms", "train_img_s"):
        result["summary"][key] = {}
        for name, _ in legs:
            v = sorted(r[key] for r in runs[name] if key in r)
            if not v:
                continue
            result["summary"][key][name] = dict(runs=[round(x, 4) for x in v], median=round(v[len(v) // 2], 4),
                                                spread=round(v[-1] - v[0], 4))
            s = result["summary"][key][name]
            print("%-14s %-8s %12.3f %12.3f   %s" % (key, name, s["median"], s["spread"], s["runs"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
