"""The pool2d cases the CPU extent test and the GPU operator test share: (kind, in_h, in_w, size, stride, pad, ceil,
expected (out_h, out_w) or None). The extent rule of include/bcnn_hip.h was checked against torch on exactly these."""

TABLE = [
    ("max", 7, 9, 3, 1, 1, 0, None),
    ("max", 16, 16, 3, 2, 1, 0, None),
    ("max", 5, 5, 2, 2, 1, 1, (3, 3)),      # the "last window starts outside" clip fires
    ("max", 13, 13, 3, 2, 0, 1, None),
    ("avg", 14, 14, 5, 3, 0, 0, None),
    ("avg", 8, 12, 2, 2, 0, 0, None),
    ("avg", 9, 10, 3, 2, 1, 1, (5, 6)),
    ("avg", 11, 11, 2, 3, 0, 0, None),      # stride > size: uncovered source elements
    ("avg", 7, 7, 7, 1, 3, 0, None),
    ("avg", 7, 7, 7, 1, 0, 0, (1, 1)),
    ("max", 13, 13, 5, 1, 2, 0, None),      # the SPP pools of YOLOv3-SPP / YOLOv4
    ("max", 13, 13, 9, 1, 4, 0, None),
    ("max", 13, 13, 13, 1, 6, 0, None),
    ("max", 36, 40, 3, 2, 1, 0, None),
    ("avg", 33, 37, 3, 2, 1, 1, (17, 19)),
]
