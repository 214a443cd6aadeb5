"""The sizes the resize kernels are swept over (tests/test_gpu_resize_sweep.py), chosen with tests/resize_plan.py so that every
decision the row-staged kernel takes at run time, and every tail of the per-pixel kernel, is taken by some case:
tests/test_resize_cases_cpu.py asserts, on the CPU, which cases cover which class, so an edit that loses a class fails there.

A case is (format word, width, height) on one of the ENGINES below; the frames of BATCHES additionally lie at a chosen residue of
the device address mod 16.  A case carries what the plan says about it at its engine's budget -- R, the rows of the last workgroup,
the staging trips (`listed`) -- written out here so that the GPU test can assert, from the plan, that it runs what the list claims.

Frames: a picture with real chroma detail, converted to the case's format, every byte perturbed so that out-of-range levels,
clipping and odd chroma values occur (as `_case` of tests/test_gpu_pixfmt.py and tests/test_gpu_pixfmt10.py make them); random
bytes for the tiny ones.  The expected network input is oracle.preprocess on the RGB bytes the format oracles work out.
"""
import functools
from collections import namedtuple

import numpy as np

import pixfmt10_oracle as p10
import pixfmt_oracle as px
import resize_plan as rp
from oracle import preprocess as pre
from resize_plan import BGR24, GRAY8, I420, NV12, P010, RGB24, UYVY422, YUV420P10, YUYV422

BT709, FULL = px.BT709, px.FULL

# engine class -> (max_width, max_height, max_batch); the row-staged kernel's budget follows from max_width
LIMIT_KEEPS, LIMIT_LOSES = rp.widest_max_width_with_rows_kernel()
ENGINES = {"std": (2560, 1200, 8), "wide": (6000, 600, 1), "limit_keeps": (LIMIT_KEEPS, 8, 1), "limit_loses": (LIMIT_LOSES, 8, 1)}


def budget(engine):
    return rp.wz_preprocess_rows_lds(ENGINES[engine][0])


Case = namedtuple("Case", "fmt w h engine R last trips")


def case_id(c):
    flags = c.fmt & ~rp.BASE_MASK
    return "%s%s-%dx%d-%s" % (rp.NAMES[c.fmt & rp.BASE_MASK], "-%x" % flags if flags else "", c.w, c.h, c.engine)


def _c(fmt, w, h, R, last=None, trips=None, engine="std"):
    return Case(fmt, w, h, engine, R, last, trips)


# ---- rows per workgroup: where the LDS budget ends the R loop (R = 2 .. 7), on cameras' sizes (wide, vertical scale below 2) -------
ROW_COUNTS = [
    _c(RGB24, 2560, 480, 2, 2, 2), _c(RGB24, 1920, 540, 3, 3, 2), _c(RGB24, 1600, 599, 4, 4, 2), _c(RGB24, 1280, 480, 5, 5, 2),
    _c(RGB24, 1200, 520, 6, 6, 2), _c(RGB24, 1000, 500, 7, 6, 2), _c(RGB24, 1919, 301, 5, 5, 2),       # (1919: sh0 takes all 16 residues)
    _c(BGR24, 1280, 480, 5, 5, 2),
    _c(NV12, 2560, 598, 4, 4, 2), _c(NV12 | BT709, 2408, 420, 5, 5, 2), _c(NV12, 2408, 350, 6, 6, 2), _c(NV12, 1920, 540, 7, 6, 2),
    _c(I420, 2560, 360, 6, 6, 2), _c(I420 | FULL, 2406, 300, 7, 6, 2),                                 # (2406 / 2 is odd: sh1, sh2 take all 16)
    _c(YUYV422, 2560, 598, 3, 3, 2), _c(UYVY422, 2560, 376, 4, 4, 2), _c(YUYV422 | BT709, 2560, 300, 5, 5, 2),
    _c(UYVY422, 2560, 250, 6, 6, 2), _c(YUYV422, 2560, 216, 7, 6, 2),
    _c(GRAY8, 2560, 598, 7, 6, 2),
    _c(P010, 1280, 480, 5, 5, 2), _c(YUV420P10, 1600, 400, 4, 4, 2),
    # ... and on up-scales, where a wide, low frame stops the loop the same way: the 10-bit formats' R = 2 .. 7 at a tenth of the bytes
    _c(P010, 2560, 150, 2, 2, (1, 2)), _c(YUV420P10 | BT709, 2560, 100, 3, 3, (1, 2)), _c(P010 | FULL, 2560, 76, 4, 4, 2),
    _c(YUV420P10, 2560, 50, 6, 6, (1, 2)), _c(P010, 2560, 44, 7, 6, 2),
]
# the raised budget (max_width 6000: 54 272 bytes): three trips of the staging loop, and R = 2 / 3 of the 8-bit 4:2:0 and R = 2 of the 4:2:2 formats,
# which no frame 2560 wide reaches under 40 KiB
WIDE = [
    _c(RGB24, 2200, 598, 4, 4, 3, "wide"), _c(RGB24, 1400, 598, 6, 6, 3, "wide"), _c(RGB24, 6000, 4, 8, 4, 3, "wide"),
    _c(NV12, 6000, 302, 3, 3, 3, "wide"), _c(YUYV422, 3000, 598, 4, 4, 3, "wide"),
    _c(NV12, 4936, 450, 2, 2, 2, "wide"), _c(UYVY422, 5432, 300, 2, 2, 2, "wide"), _c(YUV420P10, 3392, 60, 5, 5, 2, "wide"),
]
# ---- the scale-2 switch: 599 stages a span (R > 1), 600 (the scale is exactly 2.0f) and 601 two adjacent rows (R = 1) --------------
SCALE_TWO = [
    _c(RGB24, 16, 599, 8, 4, 1), _c(RGB24, 16, 600, 1, 1, 1), _c(RGB24, 16, 601, 1, 1, 1),
    _c(RGB24, 1600, 600, 1, 1, 1), _c(RGB24, 1600, 601, 1, 1, 1),                                      # (1600 x 599 is above)
    _c(NV12, 16, 598, 8, 4, 1), _c(NV12, 16, 600, 1, 1, 1), _c(YUYV422, 2560, 600, 1, 1, 1), _c(P010, 16, 602, 1, 1, 1),
]
# ---- small and lopsided: up-scales, degenerate sides, extreme aspect; identity; taps on integers ------------------------------------
SMALL = [
    _c(RGB24, 1, 1, 8, 4, 1), _c(RGB24, 2, 3, 8, 4, 1), _c(RGB24, 3, 1, 8, 4, 1), _c(RGB24, 1, 3, 8, 4, 1), _c(RGB24, 299, 299, 8, 4, 1),
    _c(RGB24, 1, 299, 8, 4, 1), _c(RGB24, 299, 2, 8, 4, 1), _c(RGB24, 301, 298, 8, 4, 1), _c(RGB24, 299, 297, 8, 4, 1),
    _c(RGB24, 300, 300, 8, 4, 1), _c(RGB24, 322, 242, 8, 4, 1), _c(RGB24, 2560, 2, 8, 4, 1), _c(RGB24, 2, 1200, 1, 1, 1),
    _c(RGB24, 3, 1200, 1, 1, 1), _c(RGB24, 900, 900, 1, 1, 1), _c(RGB24, 150, 100, 8, 4, 1), _c(RGB24, 100, 100, 8, 4, 1),
    _c(BGR24, 1, 3, 8, 4, 1), _c(BGR24, 3, 1, 8, 4, 1), _c(BGR24, 299, 3, 8, 4, 1), _c(GRAY8, 1, 1, 8, 4, 1), _c(GRAY8, 3, 299, 8, 4, 1),
    _c(GRAY8, 299, 3, 8, 4, 1), _c(GRAY8, 2560, 1, 8, 4, 1),
    _c(NV12, 2, 2, 8, 4, 1), _c(NV12, 2560, 2, 8, 4, 1), _c(NV12, 2, 1200, 1, 1, 1), _c(NV12, 298, 300, 8, 4, 1),
    _c(I420, 2, 2, 8, 4, 1), _c(I420, 2, 1200, 1, 1, 1), _c(I420, 322, 242, 8, 4, 1), _c(I420 | BT709, 900, 600, 1, 1, 1),
    _c(YUYV422, 2, 1, 8, 4, 1), _c(YUYV422, 2, 3, 8, 4, 1), _c(UYVY422, 2, 299, 8, 4, 1), _c(UYVY422, 298, 1, 8, 4, 1),
    _c(YUYV422, 300, 300, 8, 4, 1), _c(UYVY422, 322, 242, 8, 4, 1), _c(YUYV422, 2, 1200, 1, 1, 1),
    _c(P010, 2, 2, 8, 4, 1), _c(P010, 2, 1200, 1, 1, 1), _c(P010, 322, 242, 8, 4, 1), _c(YUV420P10, 2, 2, 8, 4, 1),
    _c(YUV420P10, 298, 2, 8, 4, 1), _c(YUV420P10 | FULL, 322, 242, 8, 4, 1),
]
# ---- the 60 KiB limit: frames as wide as the two engines take -------------------------------------------------------------------------
LIMIT = [
    _c(RGB24, LIMIT_KEEPS, 3, 8, 4, 3, "limit_keeps"), _c(NV12, LIMIT_KEEPS, 4, 8, 4, 2, "limit_keeps"), _c(RGB24, 322, 8, 8, 4, 1, "limit_keeps"),
    _c(RGB24, LIMIT_LOSES, 3, None, None, None, "limit_loses"), _c(NV12, LIMIT_LOSES - 1, 4, None, None, None, "limit_loses"),
    _c(RGB24, 322, 8, None, None, None, "limit_loses"),
]
CASES = ROW_COUNTS + WIDE + SCALE_TWO + SMALL + LIMIT
assert len({case_id(c) for c in CASES}) == len(CASES)

# ---- mixed batches: (case of the list's "std" engine, residue of the frame's device address mod 16); plans that differ inside one launch ------
BatchFrame = namedtuple("BatchFrame", "fmt w h residue R")
BATCHES = [
    [BatchFrame(RGB24, 64, 601, 1, 1), BatchFrame(RGB24, 2560, 480, 2, 2), BatchFrame(RGB24, 1920, 540, 3, 3), BatchFrame(P010, 1280, 480, 5, 5),
     BatchFrame(NV12, 1920, 540, 7, 7), BatchFrame(RGB24, 322, 242, 0, 8), BatchFrame(YUYV422, 2560, 598, 4, 3), BatchFrame(I420, 2560, 360, 6, 6)],
    [BatchFrame(NV12, 16, 600, 9, 1), BatchFrame(P010, 2560, 150, 8, 2), BatchFrame(YUYV422 | FULL, 2560, 598, 10, 3), BatchFrame(RGB24, 1280, 480, 11, 5),
     BatchFrame(GRAY8, 2560, 598, 13, 7), BatchFrame(YUV420P10, 322, 242, 15, 8), BatchFrame(BGR24, 1000, 500, 14, 7),
     BatchFrame(UYVY422, 2560, 376, 12, 4)],
]


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def _picture(w, h, seed):
    """An RGB picture: the synthetic frame (tiled where the case is larger than 640 x 480: the perturbation below makes every byte its
    own), random bytes for the tiny ones."""
    from watsor_amd.synth import synthetic_frame
    if min(w, h) <= 8:
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    tile = synthetic_frame(min(w, 640), min(h, 480), seed)
    return np.tile(tile, (-(-h // tile.shape[0]), -(-w // tile.shape[1]), 1))[:h, :w]


@functools.lru_cache(maxsize=24)
def frame(fmt, w, h):
    """(the frame as the entry points take it, the RGB24 frame the format oracle restates it to); read-only, shared."""
    seed = 31 * w + h + fmt
    rng = np.random.default_rng(seed)
    base, flags = fmt & rp.BASE_MASK, fmt & ~rp.BASE_MASK
    if base in (P010, YUV420P10):
        f8 = px.frame_from_rgb(_picture(w, h, seed), (NV12 if base == P010 else I420) | flags)
        y, u, v = (p.astype(np.int32) for p in p10.unpack(p10.from_8bit(f8, w, h, fmt), w, h, fmt))
        for p in (y, u, v):
            p += rng.integers(-96, 100, p.shape)
            p[::7, ::5] = rng.choice(np.array([0, 1023]), p[::7, ::5].shape)
            np.clip(p, 0, 1023, out=p)
        f = p10.pack(y, u, v, fmt, padding=rng.integers(0, 65536, (h * 3 // 2, w)).astype(np.uint16))
        rgb = p10.rgb_from_frame10(f, w, h, fmt)
    else:
        f = px.frame_from_rgb(_picture(w, h, seed), fmt).astype(np.int16)
        f += rng.integers(-24, 25, f.shape, dtype=np.int16)
        f[::37, ::11] = rng.integers(0, 256, f[::37, ::11].shape)
        f = np.clip(f, 0, 255).astype(np.uint8)
        rgb = px.rgb_from_frame(f, w, h, fmt)
    f.setflags(write=False)
    rgb.setflags(write=False)
    return f, rgb


def random_frame(fmt, w, h):
    """(a frame of random bytes -- every level, every padding bit --, its restated RGB24 frame): what the CPU's emulation is fed, where
    a picture adds nothing and costs time."""
    rng = np.random.default_rng(7 * w + 13 * h + fmt)
    f = rng.integers(0, 256, rp.frame_bytes(w, h, fmt), dtype=np.uint8)
    if fmt & rp.BASE_MASK in (P010, YUV420P10):
        return f, p10.rgb_from_frame10(f.view("<u2"), w, h, fmt)
    return f, px.rgb_from_frame(f, w, h, fmt)


@functools.lru_cache(maxsize=64)
def stored_input(fmt, w, h, half_pixel):
    """(hi, lo): the two float16 [300, 300, 3] planes an engine must store for the case's frame -- oracle.preprocess on the restated
    RGB bytes, rounded to nearest-even fp16, and the fp16 of what that rounding left."""
    ref32 = pre.preprocess(frame(fmt, w, h)[1], half_pixel_centers=half_pixel)
    hi = ref32.astype(np.float16)
    return hi, (ref32 - hi.astype(np.float32)).astype(np.float16)


# ---- what the class asserts look at ---------------------------------------------------------------------------------------------------
def case_plan(c, half_pixel=False, address=0):
    return rp.plan(c.w, c.h, c.fmt, budget(c.engine), half_pixel, address)


def listed(c, half_pixel):
    """(R, rows of the last workgroup, staging trips) the list claims for the case under a coordinate rule; trips written as a pair
    where the two rules' spans differ by a chunk across a trip's end: (legacy, half-pixel)."""
    return c.R, c.last, c.trips[int(half_pixel)] if isinstance(c.trips, tuple) else c.trips


def pixel_kernel_tail_taps(w, h, half_pixel):
    """Output pixels of an RGB24 / BGR24 frame at a 4-byte aligned address whose taps the per-pixel kernel reads byte by byte: the 12
    bytes from the 4-byte boundary below x_lo's pixel would end behind the frame (`base + 12 <= w * h * 3` fails)."""
    yl, yu, _ = pre.interpolation_weights(rp.SIZE, h, half_pixel)
    xl, _, _ = pre.interpolation_weights(rp.SIZE, w, half_pixel)
    n = 0
    for rows in (yl, yu):
        off = (rows[:, None] * w + xl[None, :]) * 3
        n += int((((off & ~3) + 12) > w * h * 3).sum())
    return n


def pixel_kernel_last_macropixel_taps(w, h, half_pixel):
    """... of a 4:2:2 frame: taps whose 8-byte load would end behind the frame, which take the 4-byte load of the last macropixel."""
    yl, yu, _ = pre.interpolation_weights(rp.SIZE, h, half_pixel)
    xl, _, _ = pre.interpolation_weights(rp.SIZE, w, half_pixel)
    n = 0
    for rows in (yl, yu):
        off = (rows[:, None] * w + (xl[None, :] & ~1)) * 2
        n += int(((off + 8) > w * h * 2).sum())
    return n


def first_coordinate(n_in, half_pixel):
    return float(rp.source_coordinate(0, rp.scale(n_in), half_pixel))


def integer_taps(n_in, half_pixel):
    """(output indices whose tap lands exactly on a source sample -- lerp 0 and lower == upper --, those that land between two)"""
    lo, hi, f = pre.interpolation_weights(rp.SIZE, n_in, half_pixel)
    return int(((f == 0) & (lo == hi)).sum()), int(((f != 0) & (lo != hi)).sum())
