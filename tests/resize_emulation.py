"""The row-staged resize kernel's DATA PATH in numpy  --  TEST INFRASTRUCTURE ONLY, for the power check of
tests/test_resize_cases_cpu.py.

Workgroup by workgroup, as `wz_k_preprocess_rows` (watsor_amd/csrc/k_preprocess.hip) does it: the byte runs of tests/resize_plan.py
are copied from the frame's bytes, as whole 16-byte chunks from the boundary below each run's first byte, one behind the other into
an LDS image of `budget` bytes (what lies past the budget is lost, and read back as 0, as the hardware answers an LDS read outside
the allocation); every tap is then read from that image at the kernel's own offsets (sh0 / lds1 + sh1 / lds2 + sh2, row - y0,
(row >> 1) - cy0), made RGB by the integer arithmetic of tests/pixfmt_oracle.py / tests/pixfmt10_oracle.py, and interpolated and
normalised with oracle/preprocess.py's weights and operations.

Without a fault it must equal `oracle.preprocess` on the restated RGB frame bit for bit -- which checks the plan's spans against the
oracle's taps.  With one of FAULTS planted it shows what a kernel with that mistake would store, so that a test can prove that the
case list of tests/resize_cases.py tells such a kernel from a right one.  Nothing here is a reference for the GPU.
"""
import numpy as np

import pixfmt10_oracle as p10
import pixfmt_oracle as px
import resize_plan as rp
from oracle import preprocess as pre

FAULTS = ("y1_floor",           # the span's last row from floor instead of ceil
          "cy1_short",          # the chroma span one row short
          "sh1_ignored",        # taps of chroma run 1 read as if it started on a 16-byte boundary
          "need_short",         # need(R) counts one row too few: R grows past the budget, the bytes behind it are lost
          "nrows_unclamped")    # the last workgroup works on R rows whatever is left of the picture
GUARD_ROWS = rp.ROWS_MAX        # rows behind the picture in the output image: where an unclamped last workgroup writes
SENTINEL = np.float32(-77.0)
PAD = 0xEE                      # the bytes around the frame (what an over-read chunk brings along and no tap may use)


def _stage(mem, origin, g, L, h, budget):
    """The LDS image of workgroup g: (bytes, where runs 1 and 2 start)."""
    chroma = origin + L.luma_bytes
    src = (origin + g.y0 * L.rowb, chroma + g.cy0 * L.crowb, chroma + L.crowb * (h >> 1) + g.cy0 * L.crowb)
    lds = np.zeros(max(16 * g.total, budget) + 64, np.uint8)
    at = 0
    for s, sh, n in zip(src, g.sh, g.chunks):
        lds[at:at + 16 * n] = mem[s - sh:s - sh + 16 * n]
        at += 16 * n
    lds[budget:] = 0
    return lds, 16 * g.chunks[0], 16 * (g.chunks[0] + g.chunks[1])


def _word10(lds, at, high):
    wd = lds[at].astype(np.int32) | (lds[at + 1].astype(np.int32) << 8)
    return wd >> 6 if high else wd & 0x3FF


def _taps(lds, lds1, lds2, g, L, fmt, y, x_lo, x_hi, faults):
    """(RGB of the left taps, RGB of the right taps) of source row y: uint8 [n, 3] each."""
    base, flags = fmt & rp.BASE_MASK, fmt & ~rp.BASE_MASK
    row = g.sh[0] + (y - g.y0) * L.rowb
    sh1 = 0 if "sh1_ignored" in faults else g.sh[1]
    crow = ((y >> 1) - g.cy0) * L.crowb
    if base in (rp.RGB24, rp.BGR24):
        off = row + x_lo * 3
        a = lds[off[:, None] + np.arange(3)]
        b = np.where((x_hi != x_lo)[:, None], lds[off[:, None] + 3 + np.arange(3)], a)     # the six bytes of two adjacent pixels
        return (a[:, ::-1], b[:, ::-1]) if base == rp.BGR24 else (a, b)
    out = []
    for x in (x_lo, x_hi):
        if base == rp.GRAY8:
            out.append(np.repeat(lds[row + x][:, None], 3, axis=1))
        elif base in (rp.YUYV422, rp.UYVY422):
            m = lds[(row + (x & ~1) * 2)[:, None] + np.arange(4)].astype(np.int32)
            uyvy = base == rp.UYVY422
            yy = np.where(x & 1, m[:, 3 if uyvy else 2], m[:, 1 if uyvy else 0])
            out.append(px.yuv_to_rgb(yy, m[:, 0 if uyvy else 1], m[:, 2 if uyvy else 3], flags))
        elif L.ten:
            high = base == rp.P010
            up = lds1 + sh1 + crow + (x >> 1) * (4 if high else 2)
            vp = up + 2 if high else lds2 + g.sh[2] + crow + (x >> 1) * 2
            out.append(p10.yuv10_to_rgb(_word10(lds, row + x * 2, high), _word10(lds, up, high), _word10(lds, vp, high), flags))
        elif base == rp.NV12:
            uv = lds1 + sh1 + crow + (x >> 1) * 2
            out.append(px.yuv_to_rgb(lds[row + x], lds[uv], lds[uv + 1], flags))
        else:
            out.append(px.yuv_to_rgb(lds[row + x], lds[lds1 + sh1 + crow + (x >> 1)], lds[lds2 + g.sh[2] + crow + (x >> 1)], flags))
    return out[0], out[1]


def rows_kernel(frame, w, h, fmt, budget, half_pixel=False, address=0, faults=frozenset(), size=rp.SIZE):
    """float32 [size + GUARD_ROWS, size, 3]: what the row-staged kernel computes before its fp16 roundings, SENTINEL where it stores
    nothing (the guard rows, unless a fault writes there)."""
    faults = frozenset(faults)
    assert faults <= set(FAULTS)
    buf = np.ascontiguousarray(frame).reshape(-1).view(np.uint8)
    assert buf.size == rp.frame_bytes(w, h, fmt)
    origin = 16 + (address & 15)
    mem = np.full(origin + buf.size + 16 * (rp.ROWS_MAX + 2), PAD, np.uint8)
    mem[origin:origin + buf.size] = buf
    p = rp.plan(w, h, fmt, budget, half_pixel, address, size, faults=faults - {"sh1_ignored"})
    # the oracle's weights for the picture's rows; the guard rows (reached only with "nrows_unclamped") continue them at the same scale
    src = np.array([rp.source_coordinate(oy, rp.scale(h, size), half_pixel) for oy in range(size + GUARD_ROWS)], np.float32)
    yl, yu = np.maximum(np.floor(src).astype(np.int64), 0), np.minimum(np.ceil(src).astype(np.int64), h - 1)
    yf = (src - np.floor(src)).astype(np.float32)
    assert all((a[:size] == b).all() for a, b in zip((yl, yu, yf), pre.interpolation_weights(size, h, half_pixel)))
    xl, xu, xf = pre.interpolation_weights(size, w, half_pixel)
    out = np.full((size + GUARD_ROWS, size, 3), SENTINEL, np.float32)
    for g in p.workgroups:
        lds, lds1, lds2 = _stage(mem, origin, g, p.layout, h, budget)
        for oy in range(g.oy0, g.oy0 + g.nrows):
            tl, tr = (t.astype(np.float32) for t in _taps(lds, lds1, lds2, g, p.layout, fmt, int(yl[oy]), xl, xu, faults))
            bl, br = (t.astype(np.float32) for t in _taps(lds, lds1, lds2, g, p.layout, fmt, int(yu[oy]), xl, xu, faults))
            top = tl + (tr - tl) * xf[:, None]                                              # (float32 arrays: one rounding per operation,
            bot = bl + (br - bl) * xf[:, None]                                              #  oracle/preprocess.py's order)
            out[oy] = pre.normalise(top + (bot - top) * yf[oy])
    return out


def expected(rgb, half_pixel=False, size=rp.SIZE):
    """The oracle's answer in the same frame: guard rows untouched."""
    out = np.full((size + GUARD_ROWS, size, 3), SENTINEL, np.float32)
    out[:size] = pre.preprocess(rgb, size, half_pixel)
    return out
