#!/usr/bin/env python
"""What bcnn_fill_tensor_with_jpegs buys: the input tensor of a batch of N = 32 JPEG images in a
416 x 416 letterbox, from compressed bytes to the finished tensor on the device, host clock around work that ends in
bcnn_synchronize. Four legs:

  parent    a built checkout of the parent commit (--parent-tree DIR; left out when not given): the composition
            available there -- bip_load_image_from_memory per image, one bcnn_fill_tensor_with_images, bcnn_synchronize
  host      this tree, the same composition: has to match the parent within the run-to-run spread
  jpegs1    this tree, one bcnn_fill_tensor_with_jpegs + bcnn_synchronize, bcnn_set_num_threads(net, 1)
  jpegs16   the same with 16 host threads for the entropy decoding

Every leg runs in a process of its own (the parent tree brings its own bcnn_amd package), the legs alternate, and each
is repeated --repeats times: the spread of the repeats is what a difference has to exceed. A measurement warms up for at
least 80 ms and 3 calls, then times --calls calls. The images are 640 x 480, 4:2:0, quality 90, encoded with PIL when it
imports, otherwise the committed fixtures of tests/golden/jpeg repeated to N; the record says which.

    python tools/jpeg_fill_time.py [--parent-tree DIR] [--out profiles/jpeg_fill.json]

--host-split needs no GPU: it times the two halves of the split host decoder on one such image, single thread -- entropy
decoding (bip_jpeg_read_coefficients) against the pixel stage (bip_jpeg_pixels_from_coefficients) -- which bounds what
moving the pixel stage to the device can remove from the host.
"""
import argparse
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_WARM_S = 0.08
N, SIDE = 32, 416
u8p = C.POINTER(C.c_uint8)


def write_images(d, count):
    """count JPEG files in d; returns where they came from"""
    import numpy as np
    try:
        from PIL import Image
    except ImportError:
        names = sorted(p for p in glob.glob(os.path.join(ROOT, "tests", "golden", "jpeg", "*.jpg"))
                       if "grey" not in os.path.basename(p))
        for k in range(count):
            with open(os.path.join(d, "%03d.jpg" % k), "wb") as f:
                f.write(open(names[k % len(names)], "rb").read())
        return "fixtures of tests/golden/jpeg, repeated"
    rs = np.random.RandomState(0)
    y, x = np.mgrid[0:480, 0:640]
    for k in range(count):       # smooth structure + texture: the bit rate of a photograph, not of noise
        base = np.stack([127 + 120 * np.sin(x / (23.0 + k) + k), 127 + 120 * np.cos(y / (17.0 + k)),
                         127 + 120 * np.sin((x + y) / (41.0 + k))], -1)
        img = np.clip(base + rs.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(d, "%03d.jpg" % k), "JPEG", quality=90, subsampling=2)
    return "PIL %s, 640 x 480, 4:2:0, quality 90" % __import__("PIL").__version__


def timed(fn, count):
    t0, warm = time.perf_counter(), 0
    while warm < 3 or time.perf_counter() - t0 < MIN_WARM_S:
        fn()
        warm += 1
    t0 = time.perf_counter()
    for _ in range(count):
        fn()
    return (time.perf_counter() - t0) / count


class _Component(C.Structure):      # bip_jpeg_component / bip_jpeg_info of include/bip/bip.h
    _fields_ = [(k, C.c_int32) for k in ("h", "v", "width", "height", "pitch", "rows", "blocks_w", "blocks_h", "idct_w",
                                         "idct_h")]


class _Info(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("width", "height", "ncomp", "hmax", "vmax", "progressive")] + \
               [("num_coefficients", C.c_size_t), ("comp", _Component * 3)]


def _bip(tree):
    bip = C.CDLL(os.path.join(tree, "bcnn_amd", "lib", "libbip.so"))
    bip.bip_load_image_from_memory.argtypes = [C.c_char_p, C.c_int, C.POINTER(u8p)] + [C.POINTER(C.c_int32)] * 3
    bip.bip_load_image_from_memory.restype = C.c_int
    if tree == ROOT:         # the split decoder: this tree only
        bip.bip_jpeg_frame_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(_Info)]
        bip.bip_jpeg_read_coefficients.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(_Info), C.POINTER(C.c_int16)]
        bip.bip_jpeg_pixels_from_coefficients.argtypes = [C.POINTER(_Info), C.POINTER(C.c_int16), u8p]
        for fn in (bip.bip_jpeg_frame_info, bip.bip_jpeg_read_coefficients, bip.bip_jpeg_pixels_from_coefficients):
            fn.restype = C.c_int
    return bip


def _frame_info(bip, data):
    info = _Info()
    assert bip.bip_jpeg_frame_info(data, len(data), C.byref(info)) == 0
    return info


def _leg(tree, leg, data, calls):
    sys.path.insert(0, tree)
    import torch
    from bcnn_amd import capi
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    files = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(data, "*.jpg")))]
    n = len(files)
    net = capi.Net(mode=capi.MODE_PREDICT, w=SIDE, h=SIDE, c=3, n=n)
    net.conv(8, 3, 1, 1, src="input", dst="conv")
    net.compile()
    L = net.L
    out = {}
    if leg == "host":
        bip, free = _bip(tree), C.CDLL(None).free
        free.argtypes = [C.c_void_p]
        ptrs, ws, hs = (C.c_void_p * n)(), (C.c_int * n)(), (C.c_int * n)()

        def one_call():
            keep = []
            for b, d in enumerate(files):
                p, w, h, c = u8p(), C.c_int32(), C.c_int32(), C.c_int32()
                assert bip.bip_load_image_from_memory(d, len(d), C.byref(p), C.byref(w), C.byref(h), C.byref(c)) == 0
                assert c.value == 3
                keep.append(p)
                ptrs[b], ws[b], hs[b] = C.cast(p, C.c_void_p), w.value, h.value
            assert L.bcnn_fill_tensor_with_images(net.net, 0, n, ptrs, ws, hs, None, 3, capi.IMAGE_FIT_LETTERBOX,
                                                  1 / 255.0, 1, 0.0, 0.0, 0.0) == 0
            for p in keep:
                free(C.cast(p, C.c_void_p))
            net.sync()
        out["bytes_uploaded"] = None
    else:
        threads = int(leg[len("jpegs"):])
        assert net.set_num_threads(threads) == 0

        def one_call():
            assert net.fill_jpegs(files, fit=capi.IMAGE_FIT_LETTERBOX, norm_coeff=1 / 255.0, swap_to_bgr=True) == (0, -1)
            net.sync()
    out["call_ms"] = timed(one_call, calls) * 1e3
    net.download(0, with_grad=False)
    out["checksum"] = float(abs(net.data(0)).sum())     # the legs fill the same tensor
    net.close()
    print(json.dumps(out))


def upload_bytes(data):
    """(decoded pixel bytes, coefficient bytes) of the batch: what the composition / the new call copies to the device
    on top of descriptors and tap tables"""
    bip = _bip(ROOT)
    pixels = coeff = 0
    for p in sorted(glob.glob(os.path.join(data, "*.jpg"))):
        info = _frame_info(bip, open(p, "rb").read())
        pixels += info.width * info.height * info.ncomp
        coeff += 2 * info.num_coefficients
    return pixels, coeff


def host_split(repeats):
    import numpy as np
    with tempfile.TemporaryDirectory() as d:
        source = write_images(d, 1)
        data = open(os.path.join(d, "000.jpg"), "rb").read()
    bip, free = _bip(ROOT), C.CDLL(None).free
    free.argtypes = [C.c_void_p]
    info = _frame_info(bip, data)
    coeff = np.zeros(info.num_coefficients, np.int16)
    img = np.zeros((info.height, info.width, info.ncomp), np.uint8)
    cp, ip = coeff.ctypes.data_as(C.POINTER(C.c_int16)), img.ctypes.data_as(u8p)

    def whole():
        p, w, h, c = u8p(), C.c_int32(), C.c_int32(), C.c_int32()
        assert bip.bip_load_image_from_memory(data, len(data), C.byref(p), C.byref(w), C.byref(h), C.byref(c)) == 0
        free(C.cast(p, C.c_void_p))
    rows = []
    for _ in range(repeats):
        e = timed(lambda: bip.bip_jpeg_read_coefficients(data, len(data), C.byref(info), cp), 50) * 1e3
        p = timed(lambda: bip.bip_jpeg_pixels_from_coefficients(C.byref(info), cp, ip), 50) * 1e3
        w = timed(whole, 50) * 1e3
        rows.append(dict(entropy_ms=round(e, 3), pixels_ms=round(p, 3), whole_ms=round(w, 3)))
    result = dict(image=source, bytes=len(data), extent=[info.width, info.height], runs=rows)
    print(json.dumps(result, indent=1))
    return result


def _child(args_list):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args_list, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("leg %s failed (%d):\n%s\n%s" % (args_list, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-tree", default=None, help="a BUILT checkout of the parent commit")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result as JSON here")
    ap.add_argument("--host-split", action="store_true", help="time the two halves of the host decoder (no GPU)")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--data", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return _leg(args.tree, args.leg, args.data, args.calls)
    if args.host_split:
        result = host_split(args.repeats)
    else:
        legs = [("host", ROOT, "host"), ("jpegs1", ROOT, "jpegs1"), ("jpegs16", ROOT, "jpegs16")]
        if args.parent_tree:
            legs.insert(0, ("parent", os.path.abspath(args.parent_tree), "host"))
        runs = {name: [] for name, _, _ in legs}
        with tempfile.TemporaryDirectory() as data:
            source = write_images(data, N)
            pixels, coeff = upload_bytes(data)
            for _ in range(args.repeats):      # alternating: whatever else the machine does hits every leg alike
                for name, tree, leg in legs:
                    runs[name].append(_child(["--leg", leg, "--tree", tree, "--data", data, "--calls", str(args.calls)]))
        result = dict(images=source, n=N, plane=[SIDE, SIDE], calls=args.calls, pixel_bytes_uploaded=pixels,
                      coefficient_bytes_uploaded=coeff, raw=runs, summary={})
        print("%-10s %12s %12s   runs (ms per call)" % ("leg", "median", "spread"))
        for name, _, _ in legs:
            v = sorted(r["call_ms"] for r in runs[name])
            s = dict(runs=[round(x, 3) for x in v], median=round(v[len(v) // 2], 3), spread=round(v[-1] - v[0], 3))
            result["summary"][name] = s
            print("%-10s %12.3f %12.3f   %s" % (name, s["median"], s["spread"], s["runs"]))
        sums = {r["checksum"] for rs in runs.values() for r in rs}
        result["same_tensor"] = len(sums) == 1
        print("bytes uploaded per batch: pixels %d (host legs), coefficients %d (jpegs legs); same tensor: %s"
              % (pixels, coeff, result["same_tensor"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
