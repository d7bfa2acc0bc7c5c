#!/usr/bin/env python
"""What the device loader path (bcnn_set_loader_on_device) buys: bcnn_loader_next + bcnn_synchronize
per batch, host clock, on two synthetic datasets with the augmentation of the reference's examples --

  cifar10   10,000 records, N = 128, flip + colour adjustment (-20, 20, 0.8, 1.2) + shift (4, 4)
  mnist     10,000 samples, N = 256, shift (5, 5) + rotation 30

-- and end to end, bcnn_train_on_batch images/s on the ResNet-18 graph of examples/cifar10 (32 x 32, N = 128) fed by the
CIFAR-10 loader above. Three legs:

  parent    a built checkout of the parent commit (--parent-tree DIR; left out when not given): the host path
  off       this tree, switch off: has to match the parent within the run-to-run spread
  on        this tree, switch on

Every leg runs in a process of its own (the parent tree brings its own bcnn_amd package), the legs alternate, and each
is repeated --repeats times: the spread of the repeats is what a difference has to exceed. A measurement warms up for at
least 80 ms and 3 batches, then times --batches batches. The list loaders are not timed: decoding stays on the host on
both paths and dominates them.

    python tools/loader_time.py [--parent-tree DIR] [--out profiles/loader_device.json]

--effects times the effects switch instead (bcnn_set_loader_effects): two legs of this tree with the
switch on, the host path (fx_host) and the device path (fx_device), ms per batch on the CIFAR-10 loader (N = 128) and on a
list of 160 x 160 x 3 PPM files (N = 32).

    python tools/loader_time.py --effects [--out profiles/loader_effects.json]
"""
import argparse
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08


def write_datasets(d, samples):
    import numpy as np
    rs = np.random.RandomState(0)
    with open(os.path.join(d, "cifar.bin"), "wb") as f:
        rec = rs.randint(0, 256, (samples, 3073)).astype(np.uint8)
        rec[:, 0] %= 10
        f.write(rec.tobytes())
    with open(os.path.join(d, "mnist-images"), "wb") as f:
        f.write(struct.pack(">IIII", 2051, samples, 28, 28) + rs.randint(0, 256, (samples, 28, 28)).astype(np.uint8).tobytes())
    with open(os.path.join(d, "mnist-labels"), "wb") as f:
        f.write(struct.pack(">II", 2049, samples) + rs.randint(0, 10, samples).astype(np.uint8).tobytes())


def cifar_resnet18(net, A):
    """examples/cifar10/cifar10_example.c:65-143"""
    def conv(f, k, s, p, act, src, dst):
        net.conv(f, k, s, p, 1, 1, act, src, dst)
    conv(64, 3, 1, 1, A.ACT_RELU, "input", "conv1")
    prev, width = "conv1", 64
    for stage in range(1, 5):
        for block in (1, 2):
            a, b, out = "conv%d_%d" % (stage, 2 * block - 1), "conv%d_%d" % (stage, 2 * block), "conv%d_add%d" % (stage, block)
            down = stage > 1 and block == 1
            if down:
                width *= 2
            conv(width, 3, 2 if down else 1, 1, A.ACT_RELU, prev, a)
            conv(width, 3, 1, 1, A.ACT_NONE, a, b)
            skip = prev
            if down:
                skip = "conv%d_res1" % stage
                conv(width, 1, 2, 0, A.ACT_NONE, prev, skip)
            net.eltwise(A.ACT_RELU, skip, b, out)
            prev = out
    net.avgpool(prev, "pool")
    net.fullc(10, A.ACT_NONE, "pool", "fc")
    net.softmax("fc", "softmax")
    net.cost("softmax", "label", "cost", 1.0)


def _leg(tree, on, data, batches, train_steps):
    sys.path.insert(0, tree)
    import torch
    from bcnn_amd import capi
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    libc = C.CDLL(None)
    vp, i, f, cp = C.c_void_p, C.c_int, C.c_float, C.c_char_p

    def prepare(net, kind, paths, **aug):
        L = net.L
        L.bcnn_set_data_loader.argtypes = [vp, i, cp, cp, cp, cp]
        L.bcnn_loader_next.argtypes = [vp]
        L.bcnn_train_on_batch.argtypes = [vp]
        L.bcnn_train_on_batch.restype = f
        L.bcnn_augment_data_with_shift.argtypes = [vp, i, i]
        L.bcnn_augment_data_with_rotation.argtypes = [vp, f]
        L.bcnn_augment_data_with_flip.argtypes = [vp, i, i]
        L.bcnn_augment_data_with_color_adjustment.argtypes = [vp, i, i, f, f]
        assert L.bcnn_set_data_loader(net.net, kind, *[p.encode() if p else None for p in paths]) == 0
        if "shift" in aug: L.bcnn_augment_data_with_shift(net.net, *aug["shift"])
        if "rotation" in aug: L.bcnn_augment_data_with_rotation(net.net, aug["rotation"])
        if "flip" in aug: L.bcnn_augment_data_with_flip(net.net, *aug["flip"])
        if "color" in aug: L.bcnn_augment_data_with_color_adjustment(net.net, *aug["color"])
        if on:
            assert net.set_loader_on_device(True) == 0
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

    cifar = (os.path.join(data, "cifar.bin"), None, os.path.join(data, "cifar.bin"), None)
    mnist = (os.path.join(data, "mnist-images"), os.path.join(data, "mnist-labels")) * 2
    cifar_aug = dict(flip=(1, 0), color=(-20, 20, 0.8, 1.2), shift=(4, 4))
    out = {}
    for name, kind, paths, shape, aug in (("cifar10", 1, cifar, (32, 3, 128), cifar_aug),
                                          ("mnist", 0, mnist, (28, 1, 256), dict(shift=(5, 5), rotation=30.0))):
        side, c, n = shape
        net = capi.Net(mode=capi.MODE_TRAIN, w=side, h=side, c=c, n=n)
        net.fullc(10, capi.ACT_NONE, "input", "fc")
        net.softmax("fc", "prob")
        net.cost("prob", "label", "cost", 1.0)
        prepare(net, kind, paths, **aug)

        def one_batch():
            assert net.L.bcnn_loader_next(net.net) == 0
            net.sync()
        out[name + "_batch_ms"] = timed(one_batch, batches) * 1e3
        net.close()
    net = capi.Net(mode=capi.MODE_TRAIN, w=32, h=32, c=3, n=128)
    cifar_resnet18(net, capi)
    net.L.bcnn_set_sgd_optimizer(net.net, 0.005, 0.9)
    prepare(net, 1, cifar, **cifar_aug)
    losses = []

    def one_step():
        losses.append(net.L.bcnn_train_on_batch(net.net))   # returns the loss: the step has finished on the device
    sec = timed(one_step, train_steps)
    out["train_img_s"] = 128 / sec
    out["last_loss"] = losses[-1]
    net.close()
    print(json.dumps(out))


FX_CONF = """[net]
batch=%d
width=%d
height=%d
channels=3
max_distortion=0.3
max_spots=3
range_shift_x=4
range_shift_y=4
min_contrast=0.8
max_contrast=1.2
loader_effects=1
loader_on_device=%d
[connected]
output=10
src=input
dst=fc
[softmax]
src=fc
dst=prob
[cost]
src=prob
dst=out
loss=euclidean
metric=error
"""


def _effects_leg(tree, device, data, batches):
    """--effects: bcnn_set_loader_effects on, host path against device path, ms per batch: the
    CIFAR-10 loader at N = 128 and a classification list of 160 x 160 x 3 PPM files at N = 32 (PPM: reading a file is a
    copy, so the list leg times the augmentation and not a decoder). The nets come from config files, which is how
    max_distortion reaches a net."""
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from bcnn_amd import capi
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    libc = C.CDLL(None)
    rs = np.random.RandomState(1)
    lines = []
    for k in range(64):
        p = os.path.join(data, "fx%d.ppm" % k)
        with open(p, "wb") as f:
            f.write(b"P6\n160 160\n255\n" + rs.randint(0, 256, (160, 160, 3)).astype(np.uint8).tobytes())
        lines.append("%s %d" % (p, k % 10))
    lst = os.path.join(data, "fx_list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(lines) + "\n")
    cifar = os.path.join(data, "cifar.bin")
    out = {}
    for name, kind, path, side, n in (("cifar10_fx_batch_ms", 1, cifar, 32, 128), ("list160_fx_batch_ms", 2, lst, 160, 32)):
        cfg = os.path.join(data, "fx_%d_%d.conf" % (side, device))
        with open(cfg, "w") as f:
            f.write(FX_CONF % (n, side, side, device))
        net = capi.Net.load_net(cfg, None, mode=capi.MODE_TRAIN)
        assert net.get_loader_effects() == 1 and net.get_loader_on_device() == device
        net.L.bcnn_set_data_loader.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
        net.L.bcnn_loader_next.argtypes = [C.c_void_p]
        assert net.L.bcnn_set_data_loader(net.net, kind, path.encode(), None, path.encode(), None) == 0
        net.compile()
        libc.srand(1)
        t0, warm = time.perf_counter(), 0
        while warm < 3 or time.perf_counter() - t0 < MIN_WARM_S:
            assert net.L.bcnn_loader_next(net.net) == 0
            net.sync()
            warm += 1
        t0 = time.perf_counter()
        for _ in range(batches):
            assert net.L.bcnn_loader_next(net.net) == 0
            net.sync()
        out[name] = (time.perf_counter() - t0) / batches * 1e3
        net.close()
    print(json.dumps(out))


def _child(args_list):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args_list, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("leg %s failed (%d):\n%s\n%s" % (args_list, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-tree", default=None, help="a BUILT checkout of the parent commit")
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--train-steps", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result as JSON here")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--data", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--effects", action="store_true",
                    help="time bcnn_set_loader_effects instead: host path (fx_host) against device path (fx_device)")
    args = ap.parse_args()
    if args.leg in ("fx_host", "fx_device"):
        return _effects_leg(args.tree, 1 if args.leg == "fx_device" else 0, args.data, args.batches)
    if args.leg:
        return _leg(args.tree, args.leg == "on", args.data, args.batches, args.train_steps)

    legs = [("off", ROOT), ("on", ROOT)]
    if args.parent_tree:
        legs.insert(0, ("parent", os.path.abspath(args.parent_tree)))
    keys = ("cifar10_batch_ms", "mnist_batch_ms", "train_img_s")
    if args.effects:
        legs, keys = [("fx_host", ROOT), ("fx_device", ROOT)], ("cifar10_fx_batch_ms", "list160_fx_batch_ms")
    runs = {name: [] for name, _ in legs}
    with tempfile.TemporaryDirectory() as data:
        write_datasets(data, args.samples)
        for _ in range(args.repeats):          # alternating: whatever else the machine does hits every leg alike
            for name, tree in legs:
                leg = name if args.effects else ("on" if name == "on" else "off")
                runs[name].append(_child(["--leg", leg, "--tree", tree, "--data", data,
                                          "--batches", str(args.batches), "--train-steps", str(args.train_steps)]))
    result = dict(samples=args.samples, batches=args.batches, train_steps=args.train_steps, raw=runs, summary={})
    print("%-18s %-8s %12s %12s   runs" % ("measurement", "leg", "median", "spread"))
    for key in keys:
        result["summary"][key] = {}
        for name, _ in legs:
            v = sorted(r[key] for r in runs[name])
            result["summary"][key][name] = dict(runs=[round(x, 4) for x in v], median=round(v[len(v) // 2], 4),
                                                spread=round(v[-1] - v[0], 4))
            s = result["summary"][key][name]
            print("%-18s %-8s %12.3f %12.3f   %s" % (key, name, s["median"], s["spread"], s["runs"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
