#!/usr/bin/env python
"""What bcnn_set_loader_decode_on_device buys on a classification list of JPEG files:
bcnn_loader_next + bcnn_synchronize per batch, host clock, under the protocol of tools/loader_time.py.

  workload  a list of 640 x 480 JPEGs (4:2:0, quality 90, encoded here by PIL as in tools/jpeg_fill_time.py), net input
            224 x 224 x 3, N = 32, TRAIN mode, flip + shift (8, 8) + colour adjustment (-20, 20, 0.8, 1.2)
  legs      parent    a built checkout of the parent commit (--parent-tree DIR; left out when not given) with
                      loader_on_device = 1: decoding on the host, one file after the other
            off       this tree, loader_on_device = 1, the new switch off: has to match the parent within the spread
            on_t1     this tree, both switches on, bcnn_set_num_threads(1)
            on_t16    the same with 16 host threads
  and, end to end with no bar, bcnn_train_on_batch images/s of the ResNet-18 graph of bench.py at 224 x 224 fed from the
  same list: parent against on_t16 (--train-steps 0 leaves it out).

Every leg runs in a process of its own (the parent tree brings its own bcnn_amd package), the legs alternate, and each is
repeated --repeats times: the spread of the repeats is what a difference has to exceed. A measurement warms up for at
least 80 ms and 3 batches, then times --batches batches. Bytes uploaded per batch are computed from the frame headers:
the raw cropped samples and their records on the host-decoding legs, the staging block of
bcnn_hip_augment_jpeg_begin (records, sums, taps, windows, tables, coefficients) on the others.

    python tools/loader_jpeg_time.py [--parent-tree DIR] [--out profiles/loader_decode_jpeg.json]
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
N, SIDE = 32, 224
LEGS = {"parent": (False, 1), "off": (False, 1), "on_t1": (True, 1), "on_t16": (True, 16)}


def _leg(tree, decode, threads, data, batches, train_steps):
    sys.path.insert(0, tree)
    import torch
    from bcnn_amd import capi
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    libc = C.CDLL(None)
    vp, i, f, cp = C.c_void_p, C.c_int, C.c_float, C.c_char_p
    lst = os.path.join(data, "list.txt")

    def prepare(net):
        L = net.L
        L.bcnn_set_data_loader.argtypes = [vp, i, cp, cp, cp, cp]
        L.bcnn_loader_next.argtypes = [vp]
        L.bcnn_train_on_batch.argtypes = [vp]
        L.bcnn_train_on_batch.restype = f
        L.bcnn_augment_data_with_shift.argtypes = [vp, i, i]
        L.bcnn_augment_data_with_flip.argtypes = [vp, i, i]
        L.bcnn_augment_data_with_color_adjustment.argtypes = [vp, i, i, f, f]
        assert L.bcnn_set_data_loader(net.net, 2, lst.encode(), None, lst.encode(), None) == 0
        L.bcnn_augment_data_with_shift(net.net, 8, 8)
        L.bcnn_augment_data_with_flip(net.net, 1, 0)
        L.bcnn_augment_data_with_color_adjustment(net.net, -20, 20, 0.8, 1.2)
        assert net.set_loader_on_device(True) == 0
        if decode:
            assert net.set_loader_decode_on_device(True) == 0
        assert net.set_num_threads(threads) == 0
        net.compile()
        libc.srand(1)

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
    net = capi.Net(mode=capi.MODE_TRAIN, w=SIDE, h=SIDE, c=3, n=N)
    net.fullc(10, capi.ACT_NONE, "input", "fc")
    net.softmax("fc", "prob")
    net.cost("prob", "label", "cost", 1.0)
    prepare(net)

    def one_batch():
        assert net.L.bcnn_loader_next(net.net) == 0
        net.sync()
    out["batch_ms"] = timed(one_batch, batches) * 1e3
    out["device_decoded"] = net.loader_device_decoded() if decode else 0
    assert out["device_decoded"] == (N if decode else 0), out
    net.close()
    if train_steps > 0:
        sys.path.append(ROOT)
        from bench import build_resnet18
        net = capi.Net(mode=capi.MODE_TRAIN, w=SIDE, h=SIDE, c=3, n=N)
        build_resnet18(net, capi, classes=10)
        net.L.bcnn_set_sgd_optimizer(net.net, 0.005, 0.9)
        prepare(net)
        losses = []

        def one_step():
            losses.append(net.L.bcnn_train_on_batch(net.net))   # returns the loss: the step has finished on the device
        out["train_img_s"] = N / timed(one_step, train_steps)
        out["last_loss"] = losses[-1]
        net.close()
    print(json.dumps(out))


def upload_bytes(data, count):
    """bytes of the one host-to-device copy of a batch, per leg kind, from the frame headers of the first N files"""
    from jpeg_fill_time import _Info
    bip = C.CDLL(os.path.join(ROOT, "bcnn_amd", "lib", "libbip.so"))
    bip.bip_jpeg_frame_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(_Info)]
    al = lambda v: (v + 15) // 16 * 16
    coeff = planes = 0
    for k in range(N):
        blob = open(os.path.join(data, "%03d.jpg" % (k % count)), "rb").read()
        info = _Info()
        assert bip.bip_jpeg_frame_info(blob, len(blob), C.byref(info)) == 0
        coeff += 2 * info.num_coefficients
        planes += info.ncomp
    records, sums, raw = al(N * 32), N * 16, al(N * SIDE * SIDE * 3)
    host = records + sums + raw                                   # bcnn_hip_augment_batch without a scale stage
    device = records + sums + al(N * 2 * SIDE * 8) + al(N * 20) + al((planes + 1) * 24) + al((N + 1) * 96) + coeff
    return {"host_decoding": host, "device_decoding": device}


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
        decode, threads = LEGS[args.leg]
        return _leg(args.tree, decode, threads, args.data, args.batches, args.train_steps)

    legs = [("off", ROOT), ("on_t1", ROOT), ("on_t16", ROOT)]
    if args.parent_tree:
        legs.insert(0, ("parent", os.path.abspath(args.parent_tree)))
    runs = {name: [] for name, _ in legs}
    with tempfile.TemporaryDirectory() as data:
        source = write_images(data, args.images)
        with open(os.path.join(data, "list.txt"), "w") as fh:
            for k in range(args.images):
                fh.write("%s %d\n" % (os.path.join(data, "%03d.jpg" % k), k % 10))
        uploaded = upload_bytes(data, args.images)
        for _ in range(args.repeats):          # alternating: whatever else the machine does hits every leg alike
            for name, tree in legs:
                train = args.train_steps if name in ("parent", "on_t16") else 0
                runs[name].append(_child(["--leg", name, "--tree", tree, "--data", data, "--batches", str(args.batches),
                                          "--train-steps", str(train)]))
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
