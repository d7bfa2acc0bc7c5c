"""Shared by the detector-training tests: truth lists, head inputs whose predictions overlap chosen truths, and an fp64
NumPy evaluation of what the reference's TRAIN forward of a YOLOv3 head (bcnn_yolo.c:250-415) derives from a head's
activated output: every cell's best IoU, the truth assignment and the statistics."""
import numpy as np

MAX_BOXES = 50
ANCHORS = [1.5, 2.0, 2.5, 1.0, 3.0, 3.5, 4.0, 2.5, 1.2, 1.7]   # total = 5 anchors (w, h), in input pixels


def _sig(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def _overlap(x1, w1, x2, w2):
    return np.minimum(x1 + w1 / 2, x2 + w2 / 2) - np.maximum(x1 - w1 / 2, x2 - w2 / 2)


def iou(a, b):
    """box_iou of (x, y, w, h) arrays that broadcast against each other, in double"""
    w = _overlap(a[..., 0], a[..., 2], b[..., 0], b[..., 2])
    h = _overlap(a[..., 1], a[..., 3], b[..., 1], b[..., 3])
    inter = np.where((w < 0) | (h < 0), 0.0, w * h)
    return inter / (a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter)


class Head:
    """geometry of one head: grid h x w, `mask` into the `anchors` table, input extent in_w x in_h"""

    def __init__(self, h, w, mask, classes, in_w=None, in_h=None, anchors=ANCHORS):
        self.h, self.w, self.mask, self.classes = h, w, list(mask), classes
        self.num = len(self.mask)
        self.anchors = np.asarray(anchors, np.float64).reshape(-1, 2)
        self.in_w, self.in_h = in_w or w, in_h or h
        self.per_box = 5 + classes
        self.channels = self.num * self.per_box

    def view(self, t):
        """[n][num][5 + classes][h][w] view of a head tensor"""
        return np.asarray(t).reshape(-1, self.num, self.per_box, self.h, self.w)

    def boxes(self, dst):
        """get_yolo_box of every prediction from the ACTIVATED output, in double: [n][num][h][w][4]"""
        d = self.view(dst).astype(np.float64)
        col, row = np.arange(self.w)[None, None, None, :], np.arange(self.h)[None, None, :, None]
        a = self.anchors[self.mask]
        return np.stack([(col + d[:, :, 0]) / self.w, (row + d[:, :, 1]) / self.h,
                         np.exp(d[:, :, 2]) * a[None, :, 0, None, None] / self.in_w,
                         np.exp(d[:, :, 3]) * a[None, :, 1, None, None] / self.in_h], axis=-1)


def truths_of(row):
    """the truths of one label row up to the first x == 0 (if (!truth.x) break)"""
    t = np.asarray(row, np.float32).reshape(MAX_BOXES, 5)
    stop = np.flatnonzero(t[:, 0] == 0)
    return t[:stop[0]] if stop.size else t


def best_iou(head, dst, labels):
    """every prediction's largest IoU against the truths of its image (0 without truths): [n][num][h][w]"""
    bx = head.boxes(dst)
    out = np.zeros(bx.shape[:-1])
    for b in range(bx.shape[0]):
        t = truths_of(labels[b]).astype(np.float64)
        if len(t):
            out[b] = iou(bx[b][..., None, :], t[:, :4]).max(axis=-1)
    return out


def assignment(head, dst, labels):
    """the truths the head takes, per image and in order: (b, t, mask_n, j, i, class, iou of the slot's prediction);
    cells and classes outside the head are left out, as the device kernel leaves them out"""
    bx = head.boxes(dst)
    out = []
    for b in range(bx.shape[0]):
        for t, tr in enumerate(truths_of(labels[b])):
            fi, fj = np.float32(tr[0]) * np.float32(head.w), np.float32(tr[1]) * np.float32(head.h)
            if not (-1 < fi < head.w and -1 < fj < head.h and -1 < tr[4] < head.classes):
                continue
            i, j, cls = int(fi), int(fj), int(tr[4])
            anchor = np.concatenate([np.zeros((len(head.anchors), 2)),
                                     head.anchors / [head.in_w, head.in_h]], axis=1)
            shifted = np.array([0.0, 0.0, tr[2], tr[3]], np.float64)
            ious = iou(anchor, shifted)
            best_n = int(np.argmax(ious)) if ious.max() > 0 else 0   # strict >, first wins, from 0
            if best_n not in head.mask:
                continue
            n = head.mask.index(best_n)
            out.append((b, t, n, j, i, cls, float(iou(bx[b, n, j, i], tr[:4].astype(np.float64)))))
    return out


def statistics(head, dst, grad, labels):
    """what bcnn_yolo_get_train_stats reports, from a head's output and gradient, in double. The class average follows
    the order of the truths: it reads the activated class score, which no truth changes."""
    d = head.view(dst).astype(np.float64)
    took = assignment(head, dst, labels)
    cnt = len(took)
    s = dict(count=cnt, cost=float(np.sum(np.asarray(grad, np.float64) ** 2)), avg_anyobj=float(d[:, :, 4].mean()))
    div = float(cnt) if cnt else float("nan")
    s["avg_iou"] = sum(k[6] for k in took) / div
    s["avg_class"] = sum(d[b, n, 5 + c, j, i] for (b, _, n, j, i, c, _) in took) / div
    s["avg_obj"] = sum(d[b, n, 4, j, i] for (b, _, n, j, i, _, _) in took) / div
    s["recall50"] = sum(k[6] > 0.5 for k in took) / div
    s["recall75"] = sum(k[6] > 0.75 for k in took) / div
    return s


def thresholds_clear(head, dst, labels, margin=1e-3):
    """no prediction's best IoU within `margin` of 0.5, no assigned truth's IoU within it of 0.5 or 0.75"""
    if np.any(np.abs(best_iou(head, dst, labels) - 0.5) < margin):
        return False
    for row in labels:   # the choice of the anchor is a comparison too: the two best are apart
        for tr in truths_of(row):
            anchor = np.concatenate([np.zeros((len(head.anchors), 2)), head.anchors / [head.in_w, head.in_h]], axis=1)
            top = np.sort(iou(anchor, np.array([0.0, 0.0, tr[2], tr[3]], np.float64)))
            if len(top) > 1 and top[-1] - top[-2] < margin:
                return False
    return all(abs(k[6] - 0.5) >= margin and abs(k[6] - 0.75) >= margin for k in assignment(head, dst, labels))


# ---- truth lists ------------------------------------------------------------------------------------------------------
def _row(truths):
    row = np.zeros((MAX_BOXES, 5), np.float32)
    t = np.asarray(truths, np.float32).reshape(-1, 5)[:MAX_BOXES]
    row[:len(t)] = t
    return row.reshape(-1)


def random_truth(rs, head, anchor=None, cell=None, cls=None):
    """a truth the size of anchor `anchor` (any of the table by default), centred in `cell` = (j, i) when given"""
    k = rs.randint(len(head.anchors)) if anchor is None else anchor
    w = head.anchors[k, 0] / head.in_w * rs.uniform(0.9, 1.1)
    h = head.anchors[k, 1] / head.in_h * rs.uniform(0.9, 1.1)
    if cell is None:
        x, y = rs.uniform(0.05, 0.95, 2)
    else:
        x, y = (cell[1] + rs.uniform(0.2, 0.8)) / head.w, (cell[0] + rs.uniform(0.2, 0.8)) / head.h
    return [x, y, w, h, rs.randint(head.classes) if cls is None else cls]


def truth_sets(rs, head):
    """name -> label row; `head` gives the grid and the mask the sets are built around"""
    m0, other = head.mask[0], [k for k in range(len(head.anchors)) if k not in head.mask][0]
    c1 = min(1, head.classes - 1)
    sets = {
        "none": [],
        "fifty": [random_truth(rs, head) for _ in range(MAX_BOXES)],
        "zero_in_the_middle": [random_truth(rs, head) for _ in range(3)] + [[0.0, 0.4, 0.2, 0.2, 0]] +
                              [random_truth(rs, head, anchor=m0) for _ in range(3)],
        # two truths in one (cell, anchor) with different classes, then two with the same class
        "same_slot": [random_truth(rs, head, m0, (1, 1), 0), random_truth(rs, head, m0, (1, 1), c1),
                      random_truth(rs, head, m0, (2, 0), c1), random_truth(rs, head, m0, (2, 0), c1)],
        # best anchor outside the mask; last column and last row
        "unmasked_and_corner": [random_truth(rs, head, other), random_truth(rs, head, m0, (head.h - 1, head.w - 1)),
                                random_truth(rs, head, m0), random_truth(rs, head, other)],
    }
    return {k: _row(v) for k, v in sets.items()}


def head_input(rs, head, n, labels, aligned=6):
    """raw head input in [-2, 2]; up to `aligned` predictions per image are set on top of a truth (IoU near 1), in the
    truth's cell and, one each, its two neighbours in the row, so that their objectness gradient is suppressed"""
    x = head.view(rs.uniform(-2, 2, (n, head.channels, head.h, head.w)))
    for b in range(n):
        done = 0
        for tr in truths_of(labels[b]):
            i, j = int(tr[0] * head.w), int(tr[1] * head.h)
            if done >= aligned or not (0 <= i < head.w and 0 <= j < head.h):
                continue
            a = rs.randint(head.num)
            aw, ah = head.anchors[head.mask[a]]
            fx, fy = tr[0] * head.w - i, tr[1] * head.h - j
            if not (0.02 < fx < 0.98 and 0.02 < fy < 0.98):
                continue
            x[b, a, 0, j, i] = np.log(fx / (1 - fx))
            x[b, a, 1, j, i] = np.log(fy / (1 - fy))
            x[b, a, 2, j, i] = np.log(tr[2] * head.in_w / aw)
            x[b, a, 3, j, i] = np.log(tr[3] * head.in_h / ah)
            done += 1
    return x.reshape(n, head.channels, head.h, head.w).astype(np.float32)
