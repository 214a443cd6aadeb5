"""The activity kernel's cases, one table for the CPU proof (tests/test_gate_walk_cpu.py) and the GPU test
(tests/test_gpu_gate_long_rows.py).

    OLD    what the suite ran before: `crop_cases` of every 8-bit format at skews 0 and 1 and the 277-pixel RGB rectangle.  No row of
           them is longer than 64 aligned 16-byte words, one trip of the kernel's loop.
    NEW    rows of 64 words and more.  tests/test_gate_walk_cpu.py asserts what this table has to reach (trips, `e` and the boundary's
           residue at a trip boundary, head parities, a split LOW10 word, every head) and that every seeded defect shows on it.

A case is (name, format word, w, h, rectangle, skew, fill, seed); `frame_of(case)` is the frame as the engine takes it (read-only,
built once), `skew` bytes past a 16-byte boundary; `oracle_view(case)` is (frame, format word) for tests/gate_oracle.py -- the frame
itself, or for the 10-bit formats the 8-bit frame of every sample's top eight bits.
"""
import functools
from collections import namedtuple

import numpy as np

import gate_walk
import pixfmt10_oracle as p10
import tile_oracle as to
from test_gpu_tiled import crop_cases, random_frame
from watsor_amd.runtime import (FMT_BGR24, FMT_GRAY8, FMT_I420, FMT_NV12, FMT_P010, FMT_RGB24, FMT_UYVY422, FMT_YUV420P10, FMT_YUYV422)

Case = namedtuple("Case", "name fmt w h rect skew fill seed")
EIGHT = {FMT_P010: FMT_NV12, FMT_YUV420P10: FMT_I420}
THREE_BYTE = (FMT_RGB24, FMT_BGR24)
TWO_BYTE = (FMT_YUYV422, FMT_UYVY422, FMT_P010, FMT_YUV420P10)
ONE_BYTE = (FMT_GRAY8, FMT_NV12, FMT_I420)
NAMES = {FMT_RGB24: "rgb", FMT_BGR24: "bgr", FMT_GRAY8: "gray", FMT_NV12: "nv12", FMT_I420: "i420", FMT_YUYV422: "yuyv", FMT_UYVY422: "uyvy",
         FMT_P010: "p010", FMT_YUV420P10: "yuv420p10"}


def _shape(w, h, fmt):
    return (h * 3 // 2, 2 * w) if fmt in EIGHT else to.tile_shape(w, h, fmt)


@functools.lru_cache(maxsize=None)
def _frame(fmt, w, h, skew, fill, seed):
    if fill == "old":                                          # the bytes tests/test_gpu_gated.py has always used
        view = random_frame(w, h, fmt, seed, skew)
    else:
        shape = _shape(w, h, fmt)
        n = int(np.prod(shape))
        buf = np.zeros(n + 64, np.uint8)
        start = (-buf.ctypes.data) % 16 + skew
        view = buf[start:start + n].reshape(shape)
        if fill == "random":                                   # (10-bit: random bits where a word carries no sample, too)
            view.reshape(-1)[:] = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
        else:
            view[...] = {"ones": 255, "zeros": 0}[fill]
    assert view.ctypes.data % 16 == skew
    view.setflags(write=False)
    return view


def frame_of(case):
    return _frame(case.fmt, case.w, case.h, case.skew, case.fill, case.seed)


def oracle_view(case):
    frame = frame_of(case)
    if case.fmt in EIGHT:
        return p10.to_8bit(frame, case.w, case.h, case.fmt), EIGHT[case.fmt]
    return frame, case.fmt


def _old():
    out = []
    for fmt in (FMT_RGB24, FMT_BGR24, FMT_GRAY8, FMT_YUYV422, FMT_UYVY422, FMT_NV12, FMT_I420):
        w, h, rects = crop_cases(fmt)
        for skew in (0, 1):
            out += [Case("old-%s-s%d-%d" % (NAMES[fmt], skew, i), fmt, w, h, r, skew, "old", 200 + fmt) for i, r in enumerate(rects)]
    out.append(Case("old-rgb-277", FMT_RGB24, 300, 200, (5, 3, 277, 190), 3, "old", 8))
    return out


def _new():
    out = []

    def add(fmt, w, h, rect, skew, fill="random"):
        name = "%s-%dx%d-%d.%d.%d.%d-s%d%s" % ((NAMES[fmt], w, h) + tuple(rect) + (skew, "" if fill == "random" else "-" + fill))
        out.append(Case(name, fmt, w, h, tuple(rect), skew, fill, 1000 + 16 * len(out) + skew))

    for fmt in THREE_BYTE:
        # 704 x 36: a pitch of 2112 = 132 * 16 bytes, every row of a rectangle has one head.  The full width is 132 words: three trips
        add(fmt, 704, 36, (0, 0, 704, 36), 0)
        add(fmt, 704, 36, (0, 0, 704, 36), 0, "ones")           # every full cell sums to 255 * 256 = 65280
        add(fmt, 704, 36, (0, 0, 704, 36), 1, "zeros")          # no cell is ever added to
        # ragged on all four sides, a last strip of 14 rows; 340 .. 343 pixels bracket the edge between 64 and 65 words
        add(fmt, 704, 36, (11, 3, 340, 30), 2)                  # head 3, 1020 bytes: 64 words, one trip
        add(fmt, 704, 36, (5, 3, 343, 30), 11)                  # head 10, 1029 bytes: 65 words
        add(fmt, 704, 36, (21, 2, 678, 31), 1)                  # head 0, 2034 bytes: 128 words, two full trips
        # 701 x 35: a pitch of 2103 bytes, 7 modulo 16 -- sixteen rows in a row take all sixteen heads
        add(fmt, 701, 35, (5, 3, 341, 30), 1)                   # 64 words under heads 0 and 1, 65 under the others
        add(fmt, 701, 35, (6, 2, 342, 29), 0)
        add(fmt, 701, 35, (3, 1, 343, 31), 11)                  # 65 words, 66 from head 12
        add(fmt, 701, 35, (7, 3, 678, 29), 2)                   # 128 words, 129 under head 15
        add(fmt, 701, 35, (0, 0, 701, 35), 0)                   # 132 or 133 words
    for fmt in TWO_BYTE:
        # 560 x 34: rows of 1120 = 70 * 16 bytes; the head is even at an even address and odd at an odd one
        add(fmt, 560, 34, (0, 0, 560, 34), 0)
        add(fmt, 560, 34, (4, 2, 552, 30), 1)                   # head 9: a two-byte sample lies across the trip boundary
        add(fmt, 560, 34, (6, 4, 520, 28), 2)
        add(fmt, 560, 34, (2, 2, 556, 30), 11)
    add(FMT_UYVY422, 560, 34, (0, 0, 560, 34), 0, "ones")
    add(FMT_YUV420P10, 560, 34, (0, 0, 560, 34), 1, "ones")     # every sample 0xFFFF: (0xFF >> 2) + ((0xFF & 3) << 6) = 255
    for fmt in ONE_BYTE:
        # 1090 x 34: rows of 1090 bytes, 2 modulo 16
        add(fmt, 1090, 34, (0, 0, 1090, 34), 0)
        add(fmt, 1090, 34, (4, 2, 1080, 30), 1)
        add(fmt, 1090, 34, (6, 4, 1078, 28), 11)
    add(FMT_GRAY8, 1090, 34, (3, 1, 1085, 31), 2)               # (GRAY8 alone takes odd rectangles)
    add(FMT_GRAY8, 1090, 34, (0, 0, 1090, 34), 0, "ones")
    return out


OLD = _old()
NEW = _new()


def walk_args(case):
    """what tests/gate_walk.py's `walk` takes for a case: (frame, addr16, offset, pitch, row_bytes, tw, th, mode)"""
    frame = frame_of(case)
    offset, pitch, row_bytes, mode = gate_walk.tile_geometry(case.w, case.fmt, case.rect)
    return frame, frame.ctypes.data % 16, offset, pitch, row_bytes, case.rect[2], case.rect[3], mode
