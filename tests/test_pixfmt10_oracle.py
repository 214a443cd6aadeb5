"""tests/pixfmt10_oracle.py (the CPU restatement of the 10-bit colour conversion) held to known answers and to the 8-bit
restatement, the library's sizing of the two 10-bit format words, and the Python layers that name and shape them.  No GPU."""
import numpy as np
import pytest

import pixfmt10_oracle as p10
import pixfmt_oracle as px
from watsor_amd import _lib
from watsor_amd.runtime import (CSP_BT709, FMT_I420, FMT_NV12, FMT_P010, FMT_RGB24, FMT_YUV420P10, FMT_YUYV422, RANGE_FULL, TEN_BIT_FORMATS,
                                YUV_FORMATS, HipEngine)

ALL_FLAGS = [0, px.FULL, px.BT709, px.BT709 | px.FULL]
TEN = [p10.P010, p10.YUV420P10]


def test_the_oracle_the_library_and_the_header_name_the_same_words():
    assert (FMT_P010, FMT_YUV420P10) == (p10.P010, p10.YUV420P10) == (0x10, 0x11) == (_lib.WZ_FMT_P010, _lib.WZ_FMT_YUV420P10)
    assert TEN_BIT_FORMATS == (FMT_P010, FMT_YUV420P10) and set(TEN_BIT_FORMATS) <= set(YUV_FORMATS)
    assert (CSP_BT709, RANGE_FULL) == (p10.BT709, p10.FULL)


# ---- known answers per (matrix, range) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_black_white_and_clipping(flags):
    full = bool(flags & px.FULL)
    one = lambda y, u=512, v=512: p10.yuv10_to_rgb(np.array([y]), np.array([u]), np.array([v]), flags)[0].tolist()
    black, white = (0, 1020) if full else (64, 940)
    assert one(black) == [0, 0, 0]
    assert one(white) == [255, 255, 255]
    if full:
        # (256 * 1023 + 512) >> 10 = 256: the top code is clipped, not wrapped
        yoff, cy = px.coefficients(flags)[:2]
        assert (cy * (1023 - 4 * yoff) + 512) >> 10 == 256
    assert one(1023) == [255, 255, 255]                      # full range 1023 / limited-range super-white
    assert one(0) == [0, 0, 0]                               # sub-black (limited) / black (full)
    if not full:
        assert one(1019) == [255, 255, 255] and one(4) == [0, 0, 0] and one(63) == [0, 0, 0]
    # a chroma excursion that leaves the cube clips channel by channel
    hot = one(white, 512, 1023)
    assert hot[0] == 255 and hot[1] < 255 and hot[2] == 255
    cold = one(black, 0, 512)
    assert cold[2] == 0 and cold[0] == 0 and cold[1] > 0


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_every_code_with_zero_low_bits_is_the_8_bit_formula(flags):
    """(4x + 512) >> 10 == (x + 128) >> 8: on samples << 2 the 10-bit arithmetic IS the 8-bit one, for every (Y, U, V) on a grid
    that holds the extremes, and for 200 000 random triples."""
    rng = np.random.default_rng(10 + flags)
    grid = np.array([0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 240, 254, 255])
    y, u, v = (a.reshape(-1) for a in np.meshgrid(grid, grid, grid, indexing="ij"))
    y, u, v = (np.concatenate([a, rng.integers(0, 256, 200000)]) for a in (y, u, v))
    np.testing.assert_array_equal(p10.yuv10_to_rgb(y << 2, u << 2, v << 2, flags), px.yuv_to_rgb(y, u, v, flags))


def test_the_low_bits_are_not_ignored():
    """... and the other three quarters of the codes are not rounded to those: the two extra bits reach the matrix."""
    y = np.arange(64, 941)
    mid = np.full_like(y, 512)
    ten = p10.yuv10_to_rgb(y, mid, mid)[:, 0].astype(int)
    eight = px.yuv_to_rgb(y >> 2, mid >> 2, mid >> 2)[:, 0].astype(int)
    assert (ten != eight).any() and np.abs(ten - eight).max() == 1
    assert (np.diff(ten) >= 0).all() and len(np.unique(ten)) == 256


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("word,word8", [(p10.P010, px.NV12), (p10.YUV420P10, px.I420)], ids=["p010-nv12", "yuv420p10-i420"])
@pytest.mark.parametrize("size", [(2, 2), (4, 2), (34, 18)], ids=lambda s: "%dx%d" % s)
def test_a_frame_of_shifted_samples_is_the_8_bit_frame(word, word8, flags, size):
    w, h = size
    rng = np.random.default_rng(w * 100 + h + flags + word)
    f8 = rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)
    f10 = p10.from_8bit(f8, w, h, word | flags)
    assert f10.dtype == np.uint16 and f10.shape == (h * 3 // 2, w) and f10.nbytes == p10.frame_bytes(w, h, word | flags) == 3 * w * h
    np.testing.assert_array_equal(p10.rgb_from_frame10(f10, w, h, word | flags), px.rgb_from_frame(f8, w, h, word8 | flags))
    np.testing.assert_array_equal(p10.to_8bit(f10, w, h, word), f8)


# ---- layouts -----------------------------------------------------------------------------------------------------------------
def test_layouts_byte_for_byte():
    """A 4x2 frame written out by hand: where every sample's two bytes lie in each layout."""
    y = np.array([[0x001, 0x102, 0x203, 0x3FF], [0x010, 0x020, 0x030, 0x040]])
    u, v = np.array([[0x155, 0x2AA]]), np.array([[0x0F0, 0x30F]])
    p = p10.pack(y, u, v, p10.P010).view(np.uint8).reshape(-1)
    w16 = lambda s: [(s << 6) & 0xFF, (s << 6) >> 8]
    assert p.tolist() == sum([w16(s) for s in y.reshape(-1).tolist() + [0x155, 0x0F0, 0x2AA, 0x30F]], [])
    q = p10.pack(y, u, v, p10.YUV420P10).view(np.uint8).reshape(-1)
    l16 = lambda s: [s & 0xFF, s >> 8]
    assert q.tolist() == sum([l16(s) for s in y.reshape(-1).tolist() + [0x155, 0x2AA, 0x0F0, 0x30F]], [])
    for word, f in ((p10.P010, p), (p10.YUV420P10, q)):
        for view in (f, f.reshape(3, 8), f.reshape(3, 4, 2), f.view(np.uint16).reshape(3, 4)):
            yy, uu, vv = p10.unpack(view, 4, 2, word)
            assert (yy == y).all() and (uu == u).all() and (vv == v).all()
    with pytest.raises(ValueError):
        p10.unpack(p[:-2], 4, 2, p10.P010)
    with pytest.raises(ValueError):
        p10.pack(y + 1, u, v, p10.P010)                       # 0x400: no 10-bit sample


@pytest.mark.parametrize("word", TEN, ids=["p010", "yuv420p10"])
def test_padding_bits_are_ignored(word):
    rng = np.random.default_rng(word)
    w, h = 6, 4
    y, u, v = rng.integers(0, 1024, (h, w)), rng.integers(0, 1024, (h // 2, w // 2)), rng.integers(0, 1024, (h // 2, w // 2))
    clean = p10.pack(y, u, v, word)
    dirty = p10.pack(y, u, v, word, padding=rng.integers(0, 65536, (h * 3 // 2, w)).astype(np.uint16))
    mask = 0x3F if word == p10.P010 else 0xFC00
    assert (clean & mask == 0).all() and (dirty & mask != 0).any() and ((clean ^ dirty) & ~np.uint16(mask) == 0).all()
    np.testing.assert_array_equal(p10.rgb_from_frame10(dirty, w, h, word | px.BT709), p10.rgb_from_frame10(clean, w, h, word | px.BT709))
    # the same words read as the other layout are another picture: the two are not interchangeable
    assert (p10.rgb_from_frame10(clean, w, h, word) != p10.rgb_from_frame10(clean, w, h, TEN[1 - TEN.index(word)])).any()


# ---- the library's sizing and validation -----------------------------------------------------------------------------------
def test_the_library_sizes_and_validates_the_10_bit_words():
    fb = _lib.load().wz_frame_bytes
    for base in TEN:
        for flags in (0, CSP_BT709, RANGE_FULL, CSP_BT709 | RANGE_FULL):
            assert fb(640, 480, base | flags) == 3 * 640 * 480 == fb(640, 480, FMT_RGB24)
            assert fb(2, 2, base | flags) == 12
            for w, h in ((641, 480), (640, 481), (641, 481), (1, 2), (2, 1), (0, 2), (-2, 2)):
                assert fb(w, h, base | flags) == 0, (w, h, hex(base | flags))
        for bad in (0x400, 0x800, 0x1000, 0x10000):
            assert fb(640, 480, base | bad) == 0
    for base in list(range(7, 16)) + [0x12, 0x13, 0x20, 0x91, 0xFF]:
        for flags in (0, CSP_BT709, RANGE_FULL):
            assert fb(640, 480, base | flags) == 0, hex(base | flags)
    # the restatement sizes and refuses alike
    for w, h in ((640, 480), (641, 480), (640, 481), (2, 2), (1, 1)):
        for word in [b | f for b in (0x10, 0x11) for f in (0, 0x100, 0x200, 0x300, 0x400)]:
            assert fb(w, h, word) == p10.frame_bytes(w, h, word), (w, h, hex(word))
    # and the words that were there before mean what they meant
    assert (fb(640, 480, 0), fb(640, 480, 1), fb(640, 480, 2), fb(640, 480, 3), fb(640, 480, 5)) == (921600, 460800, 460800, 614400, 307200)


# ---- the Python layers ---------------------------------------------------------------------------------------------------------
def test_plugin_names_and_format_words():
    from watsor_amd.detection.hip_gpu import PIXEL_FORMATS, _planar_format, format_words, frame_formats, pixel_format_code
    assert pixel_format_code("p010le") == FMT_P010 and pixel_format_code("YUV420P10LE") == FMT_YUV420P10
    assert PIXEL_FORMATS["p010le"] == 0x10 and PIXEL_FORMATS["yuv420p10le"] == 0x11
    assert format_words({"pixel_format": "p010le"}) == (FMT_P010, {})
    assert format_words({"pixel_format": "p010le", "color_matrix": "bt709"}) == (FMT_P010 | CSP_BT709, {})
    assert format_words({"pixel_format": "yuv420p10le", "color_matrix": "bt709", "color_range": "full"}) == (FMT_YUV420P10 | CSP_BT709 | RANGE_FULL, {})
    dflt, cams = format_words({"pixel_format": {"uhd": "p010le", "sw": "yuv420p10le", "old": "nv12"}, "color_matrix": {"uhd": "bt709"},
                               "color_range": {"sw": "full"}})
    assert dflt == FMT_RGB24 and cams == {"uhd": FMT_P010 | CSP_BT709, "sw": FMT_YUV420P10 | RANGE_FULL, "old": FMT_NV12}
    for bad in ("p010", "p010be", "yuv420p10", "yuv420p10be", "yuv422p10le", "p016le"):
        with pytest.raises(ValueError):
            format_words({"pixel_format": bad})
    # 10-bit is by configuration only: a planar buffer under an RGB24 camera is never taken for it
    assert _planar_format(FMT_P010, {0: FMT_YUV420P10 | CSP_BT709}) == FMT_NV12
    assert _planar_format(FMT_P010, {0: FMT_I420}) == FMT_I420
    words16, bytes8, rgb = np.zeros((6, 4), np.uint16), np.zeros((6, 8), np.uint8), np.zeros((4, 4, 3), np.uint8)
    by_cam = {0: FMT_P010 | CSP_BT709, 1: FMT_YUV420P10, 2: FMT_RGB24}
    assert frame_formats([words16, bytes8, rgb], [0, 1, 2], FMT_RGB24, by_cam) == [FMT_P010 | CSP_BT709, FMT_YUV420P10, FMT_RGB24]
    assert frame_formats([bytes8], [2], FMT_RGB24, by_cam) == [FMT_NV12]


def test_frame_geometry_of_10_bit_frames():
    g = HipEngine.frame_geometry
    z8, z16 = (lambda *s: np.zeros(s, np.uint8)), (lambda *s: np.zeros(s, np.uint16))
    for word in (FMT_P010, FMT_YUV420P10, FMT_P010 | CSP_BT709, FMT_YUV420P10 | RANGE_FULL | CSP_BT709):
        for ok in (z16(720, 640), z16(720, 640, 1), z8(720, 640, 2), z8(720, 1280), z8(720, 1280, 1)):
            assert g(ok, word) == (640, 480), (ok.shape, ok.dtype)
        assert g(z16(3, 2), word) == (2, 2) and g(z8(3, 4), word) == (2, 2)
        for bad in (z16(720, 641), z16(721, 640), z16(722, 640), z16(720, 640, 2), z16(720, 640, 3), z8(720, 640, 3), z8(720, 1282), z8(720, 1281),
                    z8(720, 641, 2), z8(722, 1280), z16(720), z8(720, 640, 2, 1), z16(720, 640).astype(np.int16), z16(720, 640).astype(np.float32)):
            with pytest.raises(ValueError):
                g(bad, word)
        for bad in (z8(6, 4, 0), z16(6, 4, 0), z8(720, 1280, 0), z16(0, 0), z8(0, 0), z8(0, 4, 2), z16(3, 0), z8(3, 0, 2)):   # empty arrays hold no frame
            with pytest.raises(ValueError):
                g(bad, word)
    # uint16 is these two formats' only; unknown bases and bits stay refused
    for word in (FMT_RGB24, FMT_NV12, FMT_I420, FMT_YUYV422, 5, 6):
        with pytest.raises(ValueError):
            g(z16(720, 640), word)
    for word in (0x12, 0x0F, 7, FMT_P010 | 0x400, FMT_YUV420P10 | 0x1000):
        for f in (z16(720, 640), z8(720, 1280)):
            with pytest.raises(ValueError):
                g(f, word)


def test_the_one_shape_rule_behind_arrays_and_frame_buffers():
    """`runtime.frame_shape`: what `frame_geometry` asks with an array's shape (channels None: no channel axis) and the frame table with a
    frame buffer's header (its one-channel image counts as 2-D).  Known answers per format, the shapes only one of the two takes, and
    a channel axis of length 0 -- an empty array, never "no channel axis"."""
    from watsor_amd.runtime import FMT_BGR24, FMT_GRAY8, FMT_UYVY422, FMT_YUYV422, frame_shape as fs
    assert fs(FMT_RGB24, 480, 640, 3, 1) == fs(FMT_BGR24, 480, 640, 3, 1) == (640, 480)
    assert fs(FMT_RGB24, 480, 640, None, 1) is None and fs(FMT_RGB24, 480, 640, 1, 1) is None and fs(FMT_RGB24, 480, 640, 3, 2) is None
    assert fs(FMT_GRAY8, 481, 643, None, 1) == fs(FMT_GRAY8, 481, 643, 1, 1) == (643, 481) and fs(FMT_GRAY8, 481, 643, 3, 1) is None
    for f in (FMT_YUYV422, FMT_UYVY422):
        assert fs(f, 481, 640, 2, 1) == (640, 481) and fs(f, 481, 1280, None, 1) == (640, 481)
        assert fs(f, 481, 641, 2, 1) is None and fs(f, 481, 1282, None, 1) is None
        assert fs(f, 481, 1280, 1, 1) is None                  # (H, 2W, 1) is no ARRAY of 4:2:2; the frame table passes None for its one channel
    for f in (FMT_NV12, FMT_I420):
        assert fs(f, 720, 640, None, 1) == fs(f, 720, 640, 1, 1) == (640, 480)
        assert all(fs(f, r, c, ch, 1) is None for r, c, ch in ((721, 640, None), (722, 640, None), (720, 641, None), (720, 640, 2), (720, 640, 3)))
        assert fs(f, 720, 640, None, 2) is None                # 16-bit items are the 10-bit formats' only
    for f in (FMT_P010, FMT_YUV420P10):
        assert fs(f, 720, 640, None, 2) == fs(f, 720, 640, 1, 2) == fs(f, 720, 640, 2, 1) == fs(f, 720, 1280, None, 1) == fs(f, 720, 1280, 1, 1) == (640, 480)
        assert all(fs(f, r, c, ch, i) is None for r, c, ch, i in ((720, 640, 2, 2), (720, 1282, None, 1), (720, 1281, 1, 1), (720, 641, 2, 1),
                                                                 (722, 1280, None, 1), (720, 640, 3, 1), (720, 640, None, 4)))
    assert fs(7, 480, 640, 3, 1) is None and fs(0x12, 720, 640, None, 2) is None
    for f in (FMT_RGB24, FMT_BGR24, FMT_GRAY8, FMT_YUYV422, FMT_UYVY422, FMT_NV12, FMT_I420, FMT_P010, FMT_YUV420P10):
        assert fs(f, 6, 4, 0, 1) is None and fs(f, 6, 4, 0, 2) is None and fs(f, 720, 1280, 0, 1) is None, f


class _Frame:
    """What `bind_frame_table` reads of a reference Frame: header, image, latch (as in tests/test_pixfmt_oracle.py)."""
    def __init__(self, w, h, channels, nbytes):
        import ctypes
        from watsor_amd.share import DetectionArray

        class Header(ctypes.Structure):
            _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("channels", ctypes.c_int), ("detections", DetectionArray)]
        self.header = Header(w, h, channels)
        self.image = (ctypes.c_uint8 * nbytes)()
        self.latch = type("Latch", (), {"next": staticmethod(lambda: None)})()


def test_frame_table_of_10_bit_cameras(tmp_path, monkeypatch):
    """A 10-bit camera's uint8 FrameBuffer, (H*3/2, 2W, 1) or (H*3/2, W, 2), is bound as the W x H frame it holds, sized by wz_frame_bytes."""
    from watsor_amd.detection import hip_gpu

    class Engine:
        def __init__(self, *a, **k):
            self.table = None

        def bind_frames(self, pix, ws, hs, fmts, cams, rows):
            self.table = list(zip(ws, hs, fmts, cams))
        submit_bound = collect_bound = None

    monkeypatch.setattr(hip_gpu, "HipEngine", Engine)
    (tmp_path / hip_gpu.ENGINE_FILE).write_bytes(b"stub")
    opts = {"pixel_format": {"hw": "p010le", "sw": "yuv420p10le"}, "color_matrix": {"hw": "bt709"}, "numa": False}
    det = hip_gpu.HipObjectDetector(str(tmp_path), 0, opts)
    fb = lambda *frames: type("FrameBuffer", (), {"frames": list(frames)})()
    nb = 3 * 64 * 48
    buffers = {"hw": fb(_Frame(128, 72, 1, nb)), "sw": fb(_Frame(64, 72, 2, nb)), "door": fb(_Frame(64, 48, 3, nb))}
    ids = {"hw": 0, "sw": 1, "door": -1}
    det._adopt_ids(ids)
    det.bind_frame_table(buffers, ids)
    assert det.engine.table == [(64, 48, FMT_RGB24, -1), (64, 48, FMT_P010 | CSP_BT709, 0), (64, 48, FMT_YUV420P10, 1)]
    for name, frame in (("hw", _Frame(128, 72, 1, nb - 1)), ("hw", _Frame(64, 72, 3, nb)), ("sw", _Frame(63, 72, 2, nb)), ("sw", _Frame(64, 73, 2, nb)),
                        ("hw", _Frame(130, 72, 1, nb + 999))):
        with pytest.raises(ValueError):
            det.bind_frame_table(dict(buffers, **{name: fb(frame)}), ids)
    # a header with 0 channels is no one-channel image: each family's own refusal, as before the shape rule was shared
    for name, frame, text in (("hw", _Frame(128, 72, 0, nb), "P010 / YUV420P10 frame buffer must be"), ("door", _Frame(64, 48, 0, nb), "must have 3 channels")):
        with pytest.raises(ValueError, match=text):
            det.bind_frame_table(dict(buffers, **{name: fb(frame)}), ids)
    # a base format the library does not know: held to three channels, then the library's sizing refuses it in its own words
    det._cams[0] = det._cams[0]._replace(fmt=9)
    for channels, text in ((3, "pixel format word 0x9 is not taken at 64x48"), (1, "must have 3 channels")):
        with pytest.raises(ValueError, match=text):
            det.bind_frame_table(dict(buffers, hw=fb(_Frame(64, 48, channels, nb))), ids)
