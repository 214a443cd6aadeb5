"""What the row-staged resize kernel DECIDES for one frame, restated on the CPU  --  TEST INFRASTRUCTURE ONLY.

`wz_k_preprocess_rows` (watsor_amd/csrc/k_preprocess.hip) chooses at run time, from a frame's width, height, format word and address
and from the LDS budget of its launch: how many output rows R a workgroup takes (`need(R)` and the rule
`while (R < WZ_PRE_ROWS_MAX && need(R + 1) <= budget) ++R`, only where scale_y < 2.0f), the span y0 .. y1 of source rows a workgroup
stages (and cy0 .. cy1 of chroma rows), the byte runs' lengths, their residues sh0 / sh1 / sh2 mod 16, the number of 16-byte chunks
and the trips of the `4 * WZ_PRE_ROWS_THREADS` staging loop.  This file restates exactly that in numpy float32 -- one rounding per
operation, as the kernel compiles with fp contraction off -- together with the two host rules `wz_preprocess_rows_lds(max_w)` and
`wz_preprocess_rows_need(w, fmt)` and the 60 KiB switch-off of wz_engine.hip (read_options).

It decides NOTHING about correctness.  The reference for every pixel stays oracle/preprocess.py on the RGB bytes that
tests/pixfmt_oracle.py / tests/pixfmt10_oracle.py work out.  The plan's job is to CHOOSE sizes (tests/resize_cases.py) and to let a
test assert that it ran the class it claims to run (R, tail, trips, residues).  A plan that disagrees with the kernel makes a test
claim the wrong class, never pass a wrong pixel.

It MUST BE RE-READ against the kernel whenever the kernel's `need`, its R rule, its span or its chunk arithmetic changes: nothing on
the GPU reports R, so a stale restatement goes unnoticed until someone compares the two texts.
"""
from collections import namedtuple

import numpy as np

F32 = np.float32

RGB24, NV12, I420, YUYV422, UYVY422, GRAY8, BGR24, P010, YUV420P10 = 0, 1, 2, 3, 4, 5, 6, 0x10, 0x11
BASE_MASK = 0xFF
NAMES = {RGB24: "rgb24", NV12: "nv12", I420: "i420", YUYV422: "yuyv422", UYVY422: "uyvy422", GRAY8: "gray", BGR24: "bgr24", P010: "p010",
         YUV420P10: "yuv420p10"}

SIZE = 300                 # the network's input side (the grid's x dimension: one workgroup per output row)
THREADS = 320              # WZ_PRE_ROWS_THREADS
ROWS_MAX = 8               # WZ_PRE_ROWS_MAX
CHUNKS_PER_TRIP = 4 * THREADS
LDS_FLOOR = 40 * 1024
LDS_LIMIT = 60 * 1024      # wz_engine.hip: above it an engine loses the row-staged kernel

Layout = namedtuple("Layout", "rowb crowb planar two_planes ten luma_bytes")
Workgroup = namedtuple("Workgroup", "oy0 nrows y0 y1 cy0 cy1 nb sh chunks total trips")
Plan = namedtuple("Plan", "R budget layout workgroups")


def layout(w, h, fmt):
    """Bytes of a row of run 0 and of a chroma row, which runs there are, and where the chroma starts."""
    base = fmt & BASE_MASK
    ten = base in (P010, YUV420P10)
    planar = base in (NV12, I420) or ten
    rowb = 3 * w if base in (RGB24, BGR24) else 2 * w if base in (YUYV422, UYVY422) or ten else w
    crowb = 2 * w if base == P010 else w if base in (NV12, YUV420P10) else w >> 1
    return Layout(rowb, crowb, planar, base in (I420, YUV420P10), ten, w * h * (2 if ten else 1))


def frame_bytes(w, h, fmt):
    base = fmt & BASE_MASK
    return w * h * 3 // 2 if base in (NV12, I420) else w * h * 2 if base in (YUYV422, UYVY422) else w * h if base == GRAY8 else w * h * 3


def scale(n_in, size=SIZE):
    return F32(n_in) / F32(size)


def source_coordinate(o, sc, half_pixel):
    """The kernel's in_row / in_x: float32, every operation rounded."""
    o = F32(o)
    return F32(F32(F32(o + F32(0.5)) * sc) - F32(0.5)) if half_pixel else F32(o * sc)


def need(R, w, h, fmt, size=SIZE, short=0):
    """LDS bytes the kernel reserves for R output rows.  `short`: rows left out of the count (the planted fault of the power check)."""
    L = layout(w, h, fmt)
    rows = int(F32(F32(R - 1) * scale(h, size))) + 3 - short
    b = rows * L.rowb + 32
    if L.planar:
        b += (2 if L.two_planes else 1) * (((rows >> 1) + 2) * L.crowb + 32)
    return b


def rows_per_workgroup(w, h, fmt, budget, size=SIZE, short=0):
    R = 1
    if scale(h, size) < F32(2.0):
        while R < ROWS_MAX and need(R + 1, w, h, fmt, size, short) <= budget:
            R += 1
    return R


def plan(w, h, fmt, budget, half_pixel=False, address=0, size=SIZE, faults=frozenset()):
    """The plan of one frame.  `faults` is for the power check of tests/test_resize_cases_cpu.py only: names of planted mistakes
    ("y1_floor", "cy1_short", "need_short", "nrows_unclamped") that a wrong kernel could make; the kernel's plan is faults=()."""
    L = layout(w, h, fmt)
    sy = scale(h, size)
    R = rows_per_workgroup(w, h, fmt, budget, size, short=1 if "need_short" in faults else 0)
    chroma = address + L.luma_bytes
    wgs = []
    for oy0 in range(0, size, R):                                  # (the workgroups behind these leave at `oy0 >= size`)
        nrows = R if "nrows_unclamped" in faults else min(R, size - oy0)
        y0 = max(int(np.floor(source_coordinate(oy0, sy, half_pixel))), 0)
        last = source_coordinate(oy0 + nrows - 1, sy, half_pixel)
        y1 = min(int(np.floor(last) if "y1_floor" in faults else np.ceil(last)), h - 1)
        cy0, cy1 = y0 >> 1, y1 >> 1
        if "cy1_short" in faults:
            cy1 = max(cy1 - 1, cy0)
        nb0 = (y1 - y0 + 1) * L.rowb
        nb1 = (cy1 - cy0 + 1) * L.crowb if L.planar else 0
        nb2 = nb1 if L.two_planes else 0
        src = (address + y0 * L.rowb, chroma + cy0 * L.crowb, chroma + L.crowb * (h >> 1) + cy0 * L.crowb)
        sh = tuple(s & 15 for s in src)
        chunks = tuple((s + nb + 15) >> 4 if nb else 0 for s, nb in zip(sh, (nb0, nb1, nb2)))
        total = sum(chunks)
        wgs.append(Workgroup(oy0, nrows, y0, y1, cy0, cy1, (nb0, nb1, nb2), sh, chunks, total, -(-total // CHUNKS_PER_TRIP)))
    return Plan(R, budget, L, tuple(wgs))


def lds_used(p):
    """The most LDS bytes a workgroup of the plan fills (whole chunks)."""
    return 16 * max(g.total for g in p.workgroups)


def trips(p):
    return max(g.trips for g in p.workgroups)


def residues(p, run):
    """The residues mod 16 of run `run` over the plan's workgroups (an empty set where the format has no such run)."""
    return {g.sh[run] for g in p.workgroups if g.nb[run]}


# ---- the host's rules -------------------------------------------------------------------------------------------------------------
def wz_preprocess_rows_lds(max_w):
    rgb = 3 * max_w * 3 + 32
    yuv = 3 * max_w + 32 + 2 * (3 * max_w + 32)
    return (max(rgb, yuv, LDS_FLOOR) + 255) & ~255


def wz_preprocess_rows_need(w, fmt):
    return 12 * w + 32 * (3 if fmt & BASE_MASK == YUV420P10 else 2)


def engine_keeps_rows_kernel(max_w):
    """wz_engine.hip, read_options: an engine whose launch would need more than 60 KiB runs every batch on the per-pixel kernel."""
    return wz_preprocess_rows_lds(max_w) <= LDS_LIMIT


def rows_fit(w, fmt, budget):
    """wz_engine.hip, rows_fit: a 10-bit frame too wide for the launch's LDS sends its batch to the per-pixel kernel."""
    return fmt & BASE_MASK not in (P010, YUV420P10) or wz_preprocess_rows_need(w, fmt) <= budget


def widest_max_width_with_rows_kernel():
    """(the widest max_width that keeps the row-staged kernel, the next one up, which loses it), from the rule itself"""
    lo, hi = 1, 1 << 20
    assert engine_keeps_rows_kernel(lo) and not engine_keeps_rows_kernel(hi)
    while hi - lo > 1:                                              # (wz_preprocess_rows_lds is monotonic in max_w)
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if engine_keeps_rows_kernel(mid) else (lo, mid)
    return lo, hi
