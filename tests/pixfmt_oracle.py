"""CPU restatement of the colour conversion the HIP resize kernel applies to a frame of ANY pixel format it takes  --  TEST
INFRASTRUCTURE ONLY, numpy integer arithmetic in the style of oracle/yuv.py (which restates NV12 / I420 at BT.601 limited range and
stays the pin of that case: tests/test_pixfmt_oracle.py holds this file to it byte for byte).

What is restated (`watsor_amd/csrc/k_preprocess.hip`: wz_yuv_coef, wz_yuv_to_rgb, wz_fetch_rgb): a frame's format word is a base
format | colour flags (include/watsor_hip.h).  The four YUV formats -- NV12, I420 (4:2:0: a pixel takes the chroma sample of its
2x2 block), YUYV422, UYVY422 (packed 4:2:2: the chroma sample of its macropixel, x >> 1 on the same row) -- become RGB by the 8.8
fixed-point form, no chroma interpolation:

    C = Y - yoff, D = U - 128, E = V - 128
    R = clip8((cy C + rv E + 128) >> 8),  G = clip8((cy C + gu D + gv E + 128) >> 8),  B = clip8((cy C + bu D + 128) >> 8)

with the coefficients DERIVED here, once, from Kr / Kb (`coefficients`): round(256 x exact), limited range scaled by 255/219 (luma)
and 255/224 (chroma).  GRAY8 is R = G = B = Y unscaled (ffmpeg's `gray` is full range), BGR24 is RGB24 with bytes 0 and 2 swapped.

Pinning status: like the 4:2:0 path, PARITY UNPINNED against ffmpeg's swscale (absent here and on the GPU machine; its C and SIMD
converters differ from each other by one LSB).  The arithmetic is pinned by known answers per (matrix, range): black, white,
clipping, and the round trip of the RGB cube's corners and the 75 % bars through the exact forward matrix.
"""
import numpy as np

RGB24, NV12, I420, YUYV422, UYVY422, GRAY8, BGR24 = range(7)      # base formats (bits 0-7 of the word)
BASE_MASK, BT709, FULL = 0xFF, 0x100, 0x200                       # colour flags
YUV = (NV12, I420, YUYV422, UYVY422)

KR_KB = {0: (0.299, 0.114), BT709: (0.2126, 0.0722)}              # BT.601, BT.709


def coefficients(flags):
    """(yoff, cy, rv, gu, gv, bu) for flags = 0 | BT709 | FULL | BT709 + FULL: round(256 x exact) from Kr / Kb."""
    kr, kb = KR_KB[flags & BT709]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if flags & FULL else (255.0 / 219.0, 255.0 / 224.0)
    q = lambda v: int(np.rint(256.0 * v))
    return (0 if flags & FULL else 16, q(sy), q(2 * (1 - kr) * sc), q(-2 * (1 - kb) * kb / kg * sc), q(-2 * (1 - kr) * kr / kg * sc),
            q(2 * (1 - kb) * sc))


def forward_matrix(flags):
    """The exact float forward transform, for test inputs and the round-trip check: rgb (..., 3) in 0..255 -> (Y, U, V) floats, unrounded."""
    kr, kb = KR_KB[flags & BT709]
    kg = 1.0 - kr - kb
    ys, cs, y0 = (1.0, 1.0, 0.0) if flags & FULL else (219.0 / 255.0, 224.0 / 255.0, 16.0)

    def f(rgb):
        rgb = np.asarray(rgb, np.float64)
        r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
        y = kr * r + kg * g + kb * b
        return y0 + ys * y, 128.0 + cs * (b - y) / (2 * (1 - kb)), 128.0 + cs * (r - y) / (2 * (1 - kr))
    return f


def yuv_to_rgb(y, u, v, flags=0):
    """int arrays Y, U, V of one shape -> (..., 3) uint8."""
    yoff, cy, rv, gu, gv, bu = coefficients(flags)
    c, d, e = np.asarray(y, np.int32) - yoff, np.asarray(u, np.int32) - 128, np.asarray(v, np.int32) - 128
    r = (cy * c + rv * e + 128) >> 8                   # (arithmetic shift on int32: floor, as in the kernel)
    g = (cy * c + gu * d + gv * e + 128) >> 8
    b = (cy * c + bu * d + 128) >> 8
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def frame_bytes(w, h, word):
    """Bytes of a frame, 0 for a word / size that is refused (what wz_frame_bytes says)."""
    base, flags = word & BASE_MASK, word & ~BASE_MASK
    if w < 1 or h < 1 or word < 0 or flags & ~(BT709 | FULL) or base > BGR24 or (flags and base not in YUV):
        return 0
    if base in (NV12, I420):
        return 0 if (w | h) & 1 else w * h * 3 // 2
    if base in (YUYV422, UYVY422):
        return 0 if w & 1 else w * h * 2
    return w * h if base == GRAY8 else w * h * 3


def planes(buf, w, h, word):
    """(Y, U, V) int32 [h, w] of a YUV frame, the chroma already spread to every pixel (nearest)."""
    base = word & BASE_MASK
    buf = np.asarray(buf, np.uint8).reshape(-1)
    if buf.size != frame_bytes(w, h, word) or base not in YUV:
        raise ValueError("not a %dx%d frame of format word 0x%x" % (w, h, word))
    if base in (YUYV422, UYVY422):
        m = buf.reshape(h, w // 2, 4).astype(np.int32)                  # one macropixel: Y0 U Y1 V | U Y0 V Y1
        yi, ui, vi = ((0, 2), 1, 3) if base == YUYV422 else ((1, 3), 0, 2)
        y = m[..., list(yi)].reshape(h, w)
        return y, np.repeat(m[..., ui], 2, axis=1), np.repeat(m[..., vi], 2, axis=1)
    y = buf[:w * h].reshape(h, w).astype(np.int32)
    c = buf[w * h:]
    if base == NV12:
        uv = c.reshape(h // 2, w // 2, 2).astype(np.int32)
        u, v = uv[..., 0], uv[..., 1]
    else:
        q = (w // 2) * (h // 2)
        u, v = c[:q].reshape(h // 2, w // 2).astype(np.int32), c[q:].reshape(h // 2, w // 2).astype(np.int32)
    spread = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    return y, spread(u), spread(v)


def rgb_from_frame(buf, w, h, word):
    """The (h, w, 3) uint8 RGB24 frame the detector sees for a frame of format word `word`."""
    base = word & BASE_MASK
    buf = np.asarray(buf, np.uint8)
    if not frame_bytes(w, h, word) or buf.size != frame_bytes(w, h, word):
        raise ValueError("not a %dx%d frame of format word 0x%x" % (w, h, word))
    if base == RGB24:
        return buf.reshape(h, w, 3).copy()
    if base == BGR24:
        return buf.reshape(h, w, 3)[..., ::-1].copy()
    if base == GRAY8:
        return np.repeat(buf.reshape(h, w, 1), 3, axis=2)
    y, u, v = planes(buf, w, h, word)
    return yuv_to_rgb(y, u, v, word & ~BASE_MASK)


def frame_from_rgb(rgb, word):
    """A test-input generator, NOT part of the restated path: the frame of format word `word` made from an RGB24 picture by the exact
    forward matrix (rounded), chroma averaged over each 2x2 block (4:2:0) or macropixel (4:2:2); gray is the BT.601 luma at full range.
    Shapes: (H*3/2, W) planar, (H, W, 2) packed 4:2:2, (H, W) gray, (H, W, 3) BGR24 / RGB24."""
    rgb = np.asarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    base, flags = word & BASE_MASK, word & ~BASE_MASK
    if not frame_bytes(w, h, word):
        raise ValueError("no %dx%d frame of format word 0x%x" % (w, h, word))
    if base == RGB24:
        return rgb.copy()
    if base == BGR24:
        return rgb[..., ::-1].copy()
    y, u, v = forward_matrix(FULL if base == GRAY8 else flags)(rgb)
    r8 = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    if base == GRAY8:
        return r8(y)
    if base in (YUYV422, UYVY422):
        u8, v8 = r8(u.reshape(h, w // 2, 2).mean(axis=2)), r8(v.reshape(h, w // 2, 2).mean(axis=2))
        y8 = r8(y).reshape(h, w // 2, 2)
        order = [y8[..., 0], u8, y8[..., 1], v8] if base == YUYV422 else [u8, y8[..., 0], v8, y8[..., 1]]
        return np.stack(order, axis=-1).reshape(h, w, 2)
    sub = lambda p: r8(p.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3)))
    u8, v8 = sub(u), sub(v)
    if base == NV12:
        chroma = np.stack([u8, v8], axis=-1).reshape(h // 2, w)
    else:
        chroma = np.concatenate([u8.reshape(-1), v8.reshape(-1)]).reshape(h // 2, w)
    return np.concatenate([r8(y), chroma], axis=0)
