"""An integer numpy restatement of the label warp rule, written from its text and not from
bcnn_amd/host/bip_label_warp.h: the label of output pixel (x, y) of a w x h sample as a pull-back through flip, shift,
scale and rotation. Whole-array gathers, one stage after the other, so that it shares no control flow with the per-pixel
C function it checks."""
import numpy as np

FLIP, SHIFT, SCALE, ROTATE = 1, 2, 4, 8
_M32 = 0xFFFFFFFF


def warp(mask, record=None, taps=None, fill=255):
    """mask: uint8 [h][w] (the cropped mask); record: (flags, x_ul, y_ul, ca, sa, ...) integers or None for the identity;
    taps: (w + h) * 2 int32, (index, frac) pairs of the columns then of the rows, read only with SCALE."""
    mask = np.asarray(mask, dtype=np.uint8)
    h, w = mask.shape
    flags, x_ul, y_ul, ca, sa = (0, 0, 0, 0, 0) if record is None else [int(v) for v in list(record)[:5]]
    F = np.int64(fill)

    # L1: the flipped mask, as a table
    L1 = mask[:, ::-1].astype(np.int64) if flags & FLIP else mask.astype(np.int64)

    # L2 as a table over the sample: the shifted label, F where the source lies outside
    yy, xx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    if flags & SHIFT:
        X, Y = xx + x_ul, yy + y_ul
        inside = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
        L2 = np.where(inside, L1[np.clip(Y, 0, h - 1), np.clip(X, 0, w - 1)], F)
    else:
        L2 = L1

    # L3 as a table: the nearer tap per axis where the resized image covers the pixel, else the shifted label itself
    if flags & SCALE:
        t = np.asarray(taps, dtype=np.int64).reshape(-1, 2)
        ix, fx, iy, fy = t[:w, 0], t[:w, 1], t[w:w + h, 0], t[w:w + h, 1]
        nx = ix + ((fx >= 8) & (w > 1))
        ny = iy + ((fy >= 8) & (h > 1))
        covered = (iy >= 0)[:, None] & (ix >= 0)[None, :]
        picked = L2[np.clip(ny, 0, h - 1)[:, None], np.clip(nx, 0, w - 1)[None, :]]
        L3 = np.where(covered, picked, L2)
    else:
        L3 = L2

    if not flags & ROTATE:
        return L3.astype(np.uint8)

    # L4: 16.16 fixed point with uint32 wrap-around about (w // 2, h // 2)
    cx, cy = w // 2, h // 2
    u, v = (xx - cx) & _M32, (yy - cy) & _M32
    cau, sau = ca & _M32, sa & _M32
    upx = (cau * u - sau * v + ((cx << 16) & _M32)) & _M32     # int64 products wrap modulo 2^64, which 2^32 divides
    upy = (sau * u + cau * v + ((cy << 16) & _M32)) & _M32
    px = np.where(upx >= 1 << 31, upx - (1 << 32), upx)          # as int32
    py = np.where(upy >= 1 << 31, upy - (1 << 32), upy)
    mx, my = px >> 16, py >> 16                                  # arithmetic shift: floor
    covered = (mx >= 0) & (mx < w - 1) & (my >= 0) & (my < h - 1)
    rx = mx + ((px & 0xFFFF) >= 0x8000)
    ry = my + ((py & 0xFFFF) >= 0x8000)
    out = np.where(covered, L3[np.clip(ry, 0, h - 1), np.clip(rx, 0, w - 1)], F)
    return out.astype(np.uint8)
