"""bcnn_yolo_get_detections_batch (threshold, box decode, ordered compaction and NMS in detect.hip) against this build's
per-image bcnn_yolo_get_detections and the unmodified reference, on the small awkward extents of tests/test_yolo_head.py
(grid 9 x 11, 3 of 5 anchors, 4 classes) with inputs that keep every decision away from its threshold
(tests/_detect_inputs.py). x, y, objectness and prob must be bit-equal to the per-image call: the same IEEE operations on
the same device values with contraction off; w and h go through expf, which is not libm's on the device: 1e-5."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (first, so that one HIP runtime serves torch and libbcnn_hip.so)

from oracle import ref_bind as rb
from tests import _detect_inputs as I
from tests import _detect_ref as D

pytestmark = pytest.mark.gpu

N = 3
SIZES = [(640, 480), (300, 500), (416, 416)]   # original (w, h) of the three images
NETW, NETH = 416, 416
CHANNELS = I.NUM * (I.COORDS + 1 + I.CLASSES)
INVALID_PARAMETER = 1


def _graph(net, is_ref=False, two_heads=False):
    """input -> concat(input) -> yolo (an identity upsample first: neither concat nor the head may be a net's first
    node); with two heads also input -> upsample x2 -> yolo with another mask. Returns the head nodes."""
    if is_ref:
        D.ref_upsample(net, 1, "input", "u0")
        D.ref_concat(net, ["input"], "cat")
        return [D.ref_yolo(net, I.NUM, I.CLASSES, I.MASK, I.ANCHORS, "cat", "yolo")]
    net.upsample(1, "input", "u0")
    net.concat(["input"], "cat")
    nodes = [net.yolo(I.NUM, I.CLASSES, I.MASK, I.ANCHORS, "cat", "yolo")]
    if two_heads:
        net.upsample(2, "input", "up")
        nodes.append(net.yolo(I.NUM, I.CLASSES, I.MASK2, I.ANCHORS, "up", "yolo2"))
    return nodes


def _hip_net(x, two_heads=False):
    from bcnn_amd import capi
    net = capi.Net(mode=capi.MODE_PREDICT, w=I.W, h=I.H, c=CHANNELS, n=N)
    nodes = _graph(net, two_heads=two_heads)
    net.compile()
    net.data(0)[...] = x
    net.upload(0)
    net.forward()
    return net, nodes


def _per_image(net, relative, thresh=I.THRESH):
    return [net.get_detections(b, SIZES[b][0], SIZES[b][1], NETW, NETH, thresh, relative) for b in range(N)]


def _worker(net):
    """the batched call with its two capacities as arguments (bcnn_layers_detect.c)"""
    from bcnn_amd import capi
    fn = net.L.bcnn_yolo_detections_batch_worker
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                   C.c_int, C.POINTER(C.POINTER(capi.Detection)), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return fn


def _batch_with_capacities(net, relative, record_cap, nms_cap):
    from bcnn_amd import capi
    ws, hs = (C.c_int * N)(*[s[0] for s in SIZES]), (C.c_int * N)(*[s[1] for s in SIZES])
    dets, counts, passes = (C.POINTER(capi.Detection) * N)(), (C.c_int * N)(), C.c_int(0)
    st = _worker(net)(net.net, ws, hs, NETW, NETH, I.THRESH, relative, record_cap, nms_cap, dets, counts,
                      C.byref(passes))
    assert st == 0, st
    return capi.detections_batch_to_lists(net.L, dets, counts), passes.value


def _bits(v):
    return np.asarray(v, np.float32).tobytes()


def _assert_same_as_per_image(got, want):
    """one image: same length; x, y, objectness, prob bit-equal; w, h within 1e-5 relative"""
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, r) in enumerate(zip(got, want)):
        for key in ("x", "y", "objectness"):
            assert _bits(g[key]) == _bits(r[key]), (k, key, g[key], r[key])
        assert g["prob"].shape == r["prob"].shape and _bits(g["prob"]) == _bits(r["prob"]), (k, g["prob"], r["prob"])
        for key in ("w", "h"):
            assert abs(g[key] - r[key]) <= 1e-5 * abs(r[key]), (k, key, g[key], r[key])


def _assert_identical(got, want):
    assert len(got) == len(want)
    for k, (g, r) in enumerate(zip(got, want)):
        for key in ("x", "y", "w", "h", "objectness", "prob"):
            assert _bits(g[key]) == _bits(r[key]), (k, key, g[key], r[key])


@pytest.fixture(scope="module")
def single():
    """one head, N = 3: the net after its forward, and the per-image results for relative = 0, 1"""
    x = I.first_admissible(N)
    net, nodes = _hip_net(x)
    y = net.node_dst(nodes[0])
    net.download(y, with_grad=False)
    for b in range(N):   # the third input condition, on the values the device computed
        o = I.candidate_objectness(net.data(y), b)
        assert len(np.unique(o)) == len(o), "image %d: two candidates share an objectness" % b
    want = {rel: _per_image(net, rel) for rel in (0, 1)}
    yield dict(net=net, x=x, want=want)
    net.close()


@pytest.mark.parametrize("relative", [0, 1])
def test_single_head_matches_per_image_call(single, relative):
    net, want = single["net"], single["want"][relative]
    got = net.get_detections_batch(SIZES, NETW, NETH, I.THRESH, relative)
    assert len(got) == N
    for b in range(N):
        _assert_same_as_per_image(got[b], want[b])
        for d in got[b]:
            assert d["prob"].shape == (I.CLASSES,)
    assert any(d["objectness"] == 0 for img in got for d in img)   # NMS suppressed something: the count includes it
    assert any(len(img) > 5 for img in got)


@pytest.mark.parametrize("relative", [0, 1])
def test_single_head_matches_reference(single, relative):
    D.need_ref()
    D.ref_lib()
    x = single["x"]
    ref = rb.RefNet(mode=rb.MODE_PREDICT, w=I.W, h=I.H, c=CHANNELS, n=N)
    _graph(ref, is_ref=True)
    ref.compile()
    ref.data(0)[...] = x
    ref.forward()
    got = single["net"].get_detections_batch(SIZES, NETW, NETH, I.THRESH, relative)
    suppressed, most = 0, 0
    for b in range(N):
        want = D.ref_detections(ref, b, SIZES[b][0], SIZES[b][1], NETW, NETH, I.THRESH, relative)
        D.assert_same_detections(got[b], want, 1e-5)
        suppressed += sum(d["objectness"] == 0 for d in want)
        most = max(most, len(want))
    assert suppressed >= 1 and most > 5
    ref.close()


def test_image_without_candidates_is_null(single):
    """image 1's objectness inputs far negative: dets[1] == NULL, num_dets[1] == 0, the other images as per image"""
    from bcnn_amd import capi
    x = I.first_admissible(N, quiet=1)
    net, _ = _hip_net(x)
    want = _per_image(net, 1)
    assert want[1] == [] and len(want[0]) > 5 and len(want[2]) > 5
    ws, hs = (C.c_int * N)(*[s[0] for s in SIZES]), (C.c_int * N)(*[s[1] for s in SIZES])
    dets, counts = (C.POINTER(capi.Detection) * N)(), (C.c_int * N)(-1, -1, -1)
    assert net.L.bcnn_yolo_get_detections_batch(net.net, ws, hs, NETW, NETH, I.THRESH, 1, dets, counts) == 0
    assert not dets[1] and counts[1] == 0
    assert dets[0] and dets[2]
    got = capi.detections_batch_to_lists(net.L, dets, counts)
    for b in (0, 2):
        _assert_same_as_per_image(got[b], want[b])
    net.close()


def _sorted_inside_tie_groups(dets, obj_ranked):
    """`dets` with every run of equal (original) objectness re-ordered by the bits of (x, y): the per-image call leaves
    the order inside such a run to qsort"""
    out, r = [], 0
    while r < len(dets):
        e = r + 1
        while e < len(dets) and obj_ranked[e] == obj_ranked[r]:
            e += 1
        out += sorted(dets[r:e], key=lambda d: (_bits(d["x"]), _bits(d["y"])))
        r = e
    return out


def test_two_heads_of_different_grids():
    """head 1 on the 9 x 11 input, head 2 on its upsample x2 (18 x 22) with another mask. Every objectness of head 1
    appears four times in head 2, so the order among equal boxes matters: candidate index, i.e. head 1 first. That
    order is checked against a numpy decode (stable sort); the comparison with the per-image call, whose order inside
    a run of equal objectness is qsort's, is made with both lists re-ordered alike inside every such run."""
    x = I.first_admissible(N, two_heads=True, shift=2.0)
    net, _ = _hip_net(x, two_heads=True)
    x5 = x.reshape(N, I.NUM, I.COORDS + 1 + I.CLASSES, I.H, I.W).astype(np.float64)
    heads = [I.decode(x5, I.MASK), I.decode(I.upsampled(x5), I.MASK2)]
    both_at_equal_rank = False
    for relative in (0, 1):
        got = net.get_detections_batch(SIZES, NETW, NETH, I.THRESH, relative)
        want = _per_image(net, relative)
        for b in range(N):
            # the expected order from the numpy decode: by objectness, equal ones in candidate order (a stable sort)
            obj = np.concatenate([hd[b][0] for hd in heads])
            box = np.concatenate([hd[b][1] for hd in heads])
            head = np.concatenate([np.full(len(hd[b][0]), k) for k, hd in enumerate(heads)])
            assert len(heads[0][b][0]) > 5 and len(heads[1][b][0]) == 4 * len(heads[0][b][0])
            assert len(got[b]) == len(obj) == len(want[b])
            order = np.argsort(-obj, kind="stable")
            ranked_obj = obj[order]
            _assert_same_as_per_image(_sorted_inside_tie_groups(got[b], ranked_obj),
                                      _sorted_inside_tie_groups(want[b], ranked_obj))
            w, h = SIZES[b]
            if NETW / w < NETH / h:
                new_w, new_h = NETW, (h * NETW) // w
            else:
                new_w, new_h = (w * NETH) // h, NETH
            for r, k in enumerate(order):
                ew = box[k, 2] * NETW / new_w * (1 if relative else w)
                eh = box[k, 3] * NETH / new_h * (1 if relative else h)
                ex = (box[k, 0] - (NETW - new_w) / 2. / NETW) / (new_w / NETW) * (1 if relative else w)
                ey = (box[k, 1] - (NETH - new_h) / 2. / NETH) / (new_h / NETH) * (1 if relative else h)
                for key, e in (("x", ex), ("y", ey), ("w", ew), ("h", eh)):
                    assert abs(got[b][r][key] - e) <= 1e-4 * max(1.0, abs(e)), (b, r, key, got[b][r][key], e, head[k])
                o = got[b][r]["objectness"]   # 0: suppressed; otherwise the candidate's own (fp32 logistic: 2e-6)
                assert o == 0 or abs(o - obj[k]) <= 2e-6, (b, r, o, obj[k])
            assert any(d["objectness"] != 0 for d in got[b])
            ranked = head[order]
            tie = ranked_obj[1:] == ranked_obj[:-1]
            both_at_equal_rank |= bool(np.any(tie & (ranked[:-1] == 0) & (ranked[1:] == 1)))
    assert both_at_equal_rank
    net.close()


def test_capacity_paths_give_the_same_result(single):
    """record capacity 4 (< the candidates of every image): the kernels run a second time with a grown block; NMS
    capacity 4: every image is finished by the host NMS. Both must return what the default capacities return."""
    net = single["net"]
    for relative in (0, 1):
        base, passes = _batch_with_capacities(net, relative, 0, 0)
        assert passes == 1 and all(len(img) > 5 for img in base)
        for b in range(N):
            _assert_same_as_per_image(base[b], single["want"][relative][b])
        grown, passes = _batch_with_capacities(net, relative, 4, 0)
        assert passes == 2
        host_nms, passes = _batch_with_capacities(net, relative, 0, 4)
        assert passes == 1
        both, passes = _batch_with_capacities(net, relative, 4, 4)
        assert passes == 2
        for b in range(N):
            _assert_identical(grown[b], base[b])
            _assert_identical(host_nms[b], base[b])
            _assert_identical(both[b], base[b])


def test_threshold_above_one_and_refusals(single):
    from bcnn_amd import capi
    net = single["net"]
    assert net.get_detections_batch(SIZES, NETW, NETH, 1.5, 1) == [[], [], []]
    ws, hs = (C.c_int * N)(*[s[0] for s in SIZES]), (C.c_int * N)(*[s[1] for s in SIZES])
    dets, counts = (C.POINTER(capi.Detection) * N)(), (C.c_int * N)(-1, -1, -1)
    call = net.L.bcnn_yolo_get_detections_batch
    assert call(net.net, ws, hs, NETW, NETH, 1.5, 1, dets, counts) == 0     # BCNN_SUCCESS, every image empty
    assert list(counts) == [0, 0, 0] and not any(bool(d) for d in dets)

    def untouched_call(handle, w_arg, h_arg, dets_arg, counts_arg):
        marks = (C.c_void_p * N)(0x1234, 0x1234, 0x1234)       # never dereferenced: the call must not write them
        cnt = (C.c_int * N)(-7, -7, -7)
        d = C.cast(marks, C.POINTER(C.POINTER(capi.Detection))) if dets_arg else None
        st = call(handle, w_arg, h_arg, NETW, NETH, I.THRESH, 1, d, cnt if counts_arg else None)
        assert list(marks) == [0x1234] * N and list(cnt) == [-7] * N
        return st

    assert untouched_call(net.net, None, hs, True, True) == INVALID_PARAMETER
    assert untouched_call(net.net, ws, None, True, True) == INVALID_PARAMETER
    assert untouched_call(net.net, ws, hs, False, True) == INVALID_PARAMETER
    assert untouched_call(net.net, ws, hs, True, False) == INVALID_PARAMETER
    assert untouched_call(None, ws, hs, True, True) == INVALID_PARAMETER
    plain = capi.Net(mode=capi.MODE_PREDICT, w=I.W, h=I.H, c=CHANNELS, n=N)   # a net without a head
    plain.upsample(1, "input", "u0")
    plain.compile()
    plain.forward()
    assert untouched_call(plain.net, ws, hs, True, True) == INVALID_PARAMETER
    plain.close()


def test_two_calls_after_one_forward_are_identical(single):
    net = single["net"]
    first = net.get_detections_batch(SIZES, NETW, NETH, I.THRESH, 0)
    second = net.get_detections_batch(SIZES, NETW, NETH, I.THRESH, 0)
    assert sum(len(img) for img in first) > 15
    for b in range(N):
        _assert_identical(second[b], first[b])
