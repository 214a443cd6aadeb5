"""CPU restatement of the colour conversion the HIP resize kernels apply to a 10-bit 4:2:0 frame (P010, YUV420P10)  --  TEST
INFRASTRUCTURE ONLY, numpy integer arithmetic beside tests/pixfmt_oracle.py, whose derived coefficient table it takes.

What is restated (`watsor_amd/csrc/k_preprocess.hip`: wz_sample10, wz_yuv10_to_rgb, the 10-bit arm of wz_fetch_rgb).  A frame is
3*w*h bytes -- little-endian 16-bit words, even w and h:
    P010       (0x10, ffmpeg's p010le):       h x w luma words, then h/2 x w/2 interleaved (U, V) word pairs; the sample is the word's
                                              HIGH ten bits (word >> 6), the low six are ignored
    YUV420P10  (0x11, ffmpeg's yuv420p10le):  h x w luma words, then the h/2 x w/2 U plane, then the V plane; the sample is the word's
                                              LOW ten bits (word & 0x3ff), the high six are ignored
A pixel takes the chroma sample of its 2x2 block (no interpolation) and the full ten bits go into the matrix:

    C = Y10 - 4 yoff, D = U10 - 512, E = V10 - 512
    R = clip8((cy C + rv E + 512) >> 10),  G = clip8((cy C + gu D + gv E + 512) >> 10),  B = clip8((cy C + bu D + 512) >> 10)

For samples whose two low bits are zero this is the 8-bit formula on sample >> 2 exactly: (4x + 512) >> 10 == (x + 128) >> 8.
"""
import numpy as np

import pixfmt_oracle as px

P010, YUV420P10 = 0x10, 0x11
BASE_MASK, BT709, FULL = px.BASE_MASK, px.BT709, px.FULL
TEN = (P010, YUV420P10)


def frame_bytes(w, h, word):
    """Bytes of a 10-bit frame, 0 for a word / size that is refused (what wz_frame_bytes says for bases 0x10 and 0x11)."""
    base, flags = word & BASE_MASK, word & ~BASE_MASK
    if w < 1 or h < 1 or word < 0 or flags & ~(BT709 | FULL) or base not in TEN or (w | h) & 1:
        return 0
    return 3 * w * h


def yuv10_to_rgb(y, u, v, flags=0):
    """int arrays of 10-bit Y, U, V of one shape -> (..., 3) uint8."""
    yoff, cy, rv, gu, gv, bu = px.coefficients(flags)
    c, d, e = np.asarray(y, np.int32) - 4 * yoff, np.asarray(u, np.int32) - 512, np.asarray(v, np.int32) - 512
    r = (cy * c + rv * e + 512) >> 10                  # (arithmetic shift on int32: floor, as in the kernel)
    g = (cy * c + gu * d + gv * e + 512) >> 10
    b = (cy * c + bu * d + 512) >> 10
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def _words(frame, w, h, word):
    """The frame's 3*w*h/2 words as a flat uint16 array, whatever view of its bytes was handed over."""
    f = np.ascontiguousarray(frame)
    if f.dtype == np.uint8:
        f = f.reshape(-1).view("<u2")
    if f.dtype != np.uint16 or not frame_bytes(w, h, word) or f.size * 2 != frame_bytes(w, h, word):
        raise ValueError("not a %dx%d frame of format word 0x%x" % (w, h, word))
    return f.reshape(-1)


def unpack(frame, w, h, word):
    """(Y [h, w], U [h/2, w/2], V [h/2, w/2]) int32 10-bit samples of a frame; the padding bits are dropped."""
    base = word & BASE_MASK
    wd = _words(frame, w, h, word).astype(np.int32)
    s = wd >> 6 if base == P010 else wd & 0x3FF
    y, c = s[:w * h].reshape(h, w), s[w * h:]
    if base == P010:
        uv = c.reshape(h // 2, w // 2, 2)
        return y, uv[..., 0], uv[..., 1]
    q = (w // 2) * (h // 2)
    return y, c[:q].reshape(h // 2, w // 2), c[q:].reshape(h // 2, w // 2)


def pack(y, u, v, word, padding=None):
    """The (h*3/2, w) uint16 frame of format word `word` from 10-bit samples Y [h, w], U, V [h/2, w/2].  padding: a uint16 array of
    the frame's shape whose bits fill the six bits of every word that carry no sample (None: zeros, as a decoder writes them)."""
    base = word & BASE_MASK
    y, u, v = (np.asarray(p).astype(np.uint16) for p in (y, u, v))
    h, w = y.shape
    if not frame_bytes(w, h, word) or u.shape != (h // 2, w // 2) or v.shape != u.shape or max(y.max(), u.max(), v.max()) > 1023:
        raise ValueError("no %dx%d frame of format word 0x%x from these planes" % (w, h, word))
    if base == P010:
        chroma = np.stack([u, v], axis=-1).reshape(h // 2, w)
    else:
        chroma = np.concatenate([u.reshape(-1), v.reshape(-1)]).reshape(h // 2, w)
    s = np.concatenate([y, chroma], axis=0)
    pad = np.zeros_like(s) if padding is None else np.asarray(padding, np.uint16).reshape(s.shape)
    if base == P010:
        return ((s << 6) | (pad & 0x3F)).astype(np.uint16)
    return (s | (pad & 0xFC00)).astype(np.uint16)


def rgb_from_frame10(frame, w, h, word):
    """The (h, w, 3) uint8 RGB24 frame the detector sees for a 10-bit frame of format word `word`."""
    y, u, v = unpack(frame, w, h, word)
    spread = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    return yuv10_to_rgb(y, spread(u), spread(v), word & ~BASE_MASK)


def from_8bit(frame8, w, h, word):
    """A test-input generator: the 10-bit frame of format word `word` (P010 from an NV12, YUV420P10 from an I420 frame of the same
    flags) whose samples are the 8-bit frame's << 2."""
    base = word & BASE_MASK
    y, u, v = (p.astype(np.int32) for p in _planes8(frame8, w, h, px.NV12 if base == P010 else px.I420))
    return pack(y << 2, u << 2, v << 2, word)


def to_8bit(frame, w, h, word):
    """The 8-bit frame (NV12 for P010, I420 for YUV420P10; (h*3/2, w) uint8) of every sample's top eight bits."""
    base = word & BASE_MASK
    y, u, v = (p >> 2 for p in unpack(frame, w, h, word))
    if base == P010:
        chroma = np.stack([u, v], axis=-1).reshape(h // 2, w)
    else:
        chroma = np.concatenate([u.reshape(-1), v.reshape(-1)]).reshape(h // 2, w)
    return np.concatenate([y, chroma], axis=0).astype(np.uint8)


def _planes8(frame8, w, h, base8):
    buf = np.asarray(frame8, np.uint8).reshape(-1)
    y, c = buf[:w * h].reshape(h, w), buf[w * h:]
    if base8 == px.NV12:
        uv = c.reshape(h // 2, w // 2, 2)
        return y, uv[..., 0], uv[..., 1]
    q = (w // 2) * (h // 2)
    return y, c[:q].reshape(h // 2, w // 2), c[q:].reshape(h // 2, w // 2)
