"""tests/pixfmt_oracle.py -- the CPU restatement of the colour conversion for every pixel format and colour description the resize
kernel takes -- pinned by known answers (there is no ffmpeg here to pin it against), the geometry of the new frame shapes, the plugin
options, and the library's own sizing / validation of format words (the library loads without a GPU, as in tests/test_abi.py)."""
import numpy as np
import pytest

import pixfmt_oracle as px
from oracle import yuv
from watsor_amd import _lib
from watsor_amd.runtime import (CSP_BT709, FMT_BGR24, FMT_GRAY8, FMT_I420, FMT_NV12, FMT_RGB24, FMT_UYVY422, FMT_YUYV422, RANGE_FULL,
                                HipEngine)

COLOURS = [0, px.FULL, px.BT709, px.BT709 | px.FULL]
CORNERS = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
BARS_75 = np.array([[191, 191, 191], [191, 191, 0], [0, 191, 191], [0, 191, 0], [191, 0, 191], [191, 0, 0], [0, 0, 191], [0, 0, 0]], np.uint8)


def test_the_oracle_and_the_library_name_the_same_words():
    assert (px.RGB24, px.NV12, px.I420, px.YUYV422, px.UYVY422, px.GRAY8, px.BGR24) == \
           (FMT_RGB24, FMT_NV12, FMT_I420, FMT_YUYV422, FMT_UYVY422, FMT_GRAY8, FMT_BGR24) == (0, 1, 2, 3, 4, 5, 6)
    assert (px.BT709, px.FULL, px.BASE_MASK) == (CSP_BT709, RANGE_FULL, _lib.WZ_FMT_BASE_MASK) == (0x100, 0x200, 0xFF)


def test_derived_coefficients_are_the_published_table():
    """round(256 x exact) from Kr / Kb, against the table of the kernel's header comment: no rounding disagrees."""
    assert px.coefficients(0) == (16, 298, 409, -100, -208, 516)
    assert px.coefficients(px.FULL) == (0, 256, 359, -88, -183, 454)
    assert px.coefficients(px.BT709) == (16, 298, 459, -55, -136, 541)
    assert px.coefficients(px.BT709 | px.FULL) == (0, 256, 403, -48, -120, 475)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_no_flags_on_420_is_oracle_yuv_byte_for_byte(fmt):
    rng = np.random.default_rng(5)
    word = {"nv12": px.NV12, "i420": px.I420}[fmt]
    for w, h in ((2, 2), (6, 4), (34, 18), (64, 48)):
        frame = rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)
        np.testing.assert_array_equal(px.rgb_from_frame(frame, w, h, word), yuv.rgb_from_yuv420(frame, w, h, fmt))


@pytest.mark.parametrize("flags", COLOURS)
def test_black_white_and_clipping(flags):
    lo, hi = (0, 255) if flags & px.FULL else (16, 235)
    assert px.yuv_to_rgb(lo, 128, 128, flags).tolist() == [0, 0, 0]
    assert px.yuv_to_rgb(hi, 128, 128, flags).tolist() == [255, 255, 255]
    # out-of-range inputs clip: below black / above white (limited range), and chroma that drives a channel past either end
    assert px.yuv_to_rgb(0, 128, 128, flags).tolist() == [0, 0, 0]
    assert px.yuv_to_rgb(255, 128, 128, flags).tolist() == [255, 255, 255]
    assert px.yuv_to_rgb(hi, 255, 255, flags).tolist()[0::2] == [255, 255]
    assert px.yuv_to_rgb(lo, 0, 0, flags).tolist()[0::2] == [0, 0]
    assert px.yuv_to_rgb(lo, 255, 255, flags).tolist()[1] == 0 and px.yuv_to_rgb(hi, 0, 0, flags).tolist()[1] == 255


@pytest.mark.parametrize("flags", COLOURS)
def test_round_trip_of_the_cube_corners_and_the_75_percent_bars(flags):
    """exact forward matrix -> 8 bits -> fixed-point inverse: within 3 levels.  (+-1/2 LSB of rounding in each of Y, U, V times the
    largest row of coefficient magnitudes -- 709 limited, B: 1.164 + 2.112 -- plus the 8.8 truncation stays below 2.3.)"""
    for colours in (CORNERS, BARS_75):
        y, u, v = px.forward_matrix(flags)(colours)
        back = px.yuv_to_rgb(np.rint(y).astype(int), np.rint(u).astype(int), np.rint(v).astype(int), flags)
        assert np.abs(back.astype(int) - colours.astype(int)).max() <= 3


def _chroma_rich(w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_the_flags_are_not_ignored():
    rgb = _chroma_rich(16, 8, 1)
    for base in px.YUV:
        frame = px.frame_from_rgb(rgb, base)
        out = {f: px.rgb_from_frame(frame, 16, 8, base | f) for f in COLOURS}
        assert (out[0] != out[px.BT709]).any() and (out[0] != out[px.FULL]).any() and (out[px.BT709] != out[px.BT709 | px.FULL]).any()
        assert (out[px.FULL] != out[px.BT709 | px.FULL]).any()


@pytest.mark.parametrize("flags", COLOURS)
def test_yuyv_and_uyvy_of_one_picture_give_the_same_rgb(flags):
    rng = np.random.default_rng(2)
    yuyv = rng.integers(0, 256, (5, 6, 2), dtype=np.uint8)                       # odd height, three macropixels per row
    uyvy = yuyv.reshape(5, 3, 4)[..., [1, 0, 3, 2]].reshape(5, 6, 2)
    a = px.rgb_from_frame(yuyv, 6, 5, px.YUYV422 | flags)
    np.testing.assert_array_equal(a, px.rgb_from_frame(uyvy, 6, 5, px.UYVY422 | flags))
    # ... and it is the macropixel's chroma with each pixel's own luma
    m = yuyv.reshape(5, 3, 4).astype(int)
    np.testing.assert_array_equal(a[:, 0::2], px.yuv_to_rgb(m[..., 0], m[..., 1], m[..., 3], flags))
    np.testing.assert_array_equal(a[:, 1::2], px.yuv_to_rgb(m[..., 2], m[..., 1], m[..., 3], flags))


def test_gray_and_bgr():
    rng = np.random.default_rng(3)
    g = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    out = px.rgb_from_frame(g, 7, 5, px.GRAY8)
    assert out.shape == (5, 7, 3) and all((out[..., c] == g).all() for c in range(3))
    bgr = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    np.testing.assert_array_equal(px.rgb_from_frame(bgr, 7, 5, px.BGR24), bgr[..., ::-1])
    np.testing.assert_array_equal(px.rgb_from_frame(bgr, 7, 5, px.RGB24), bgr)


def test_generated_frames_round_trip_close_to_the_picture():
    """The input generator and the restated path are each other's inverse up to subsampling and rounding, on a smooth picture."""
    yy, xx = np.mgrid[0:16, 0:20]
    smooth = np.stack([40 + 8 * xx, 200 - 6 * yy, 60 + 4 * xx + 3 * yy], axis=-1).astype(np.uint8)
    for base in px.YUV:
        for flags in COLOURS:
            back = px.rgb_from_frame(px.frame_from_rgb(smooth, base | flags), 20, 16, base | flags)
            assert np.abs(back.astype(int) - smooth.astype(int)).max() <= 12       # (chroma is averaged over a block of a gradient)
    np.testing.assert_array_equal(px.rgb_from_frame(px.frame_from_rgb(smooth, px.BGR24), 20, 16, px.BGR24), smooth)


# ---- geometry, the library's sizing and validation, option parsing ---------------------------------------------------------
def test_frame_geometry_of_the_new_shapes():
    g = HipEngine.frame_geometry
    z = lambda *s: np.zeros(s, np.uint8)
    for word in (FMT_YUYV422, FMT_UYVY422, FMT_YUYV422 | CSP_BT709, FMT_UYVY422 | RANGE_FULL | CSP_BT709):
        assert g(z(480, 640, 2), word) == (640, 480)
        assert g(z(481, 1280), word) == (640, 481)                               # (H, 2W), odd height
        for bad in (z(480, 641, 2), z(480, 1282), z(480, 640, 3), z(480, 640, 1), z(6, 4, 0), z(480, 1280, 0)):
            with pytest.raises(ValueError):
                g(bad, word)
    assert g(z(481, 643), FMT_GRAY8) == (643, 481) and g(z(481, 643, 1), FMT_GRAY8) == (643, 481)
    assert g(z(481, 643, 3), FMT_BGR24) == (643, 481)
    assert g(z(720, 640), FMT_NV12 | CSP_BT709) == (640, 480) and g(z(720, 640), FMT_I420 | RANGE_FULL) == (640, 480)
    for bad, word in ((z(6, 4, 0), FMT_GRAY8), (z(6, 4, 0), FMT_NV12), (z(6, 4, 0), FMT_I420), (z(6, 4, 0), FMT_RGB24), (z(6, 4, 0), FMT_BGR24),
                      (z(480, 640, 3), FMT_GRAY8), (z(480, 640), FMT_BGR24), (z(480, 640, 3), FMT_RGB24 | CSP_BT709),
                      (z(480, 640), FMT_GRAY8 | RANGE_FULL), (z(480, 640, 3), FMT_BGR24 | CSP_BT709), (z(720, 640), FMT_NV12 | 0x400),
                      (z(480, 640, 3), 9), (z(480, 640, 3), 7), (z(480, 640, 2).astype(np.float32), FMT_YUYV422)):
        with pytest.raises(ValueError):
            g(bad, word)


def test_the_library_sizes_and_validates_format_words():
    lib = _lib.load()
    fb = lib.wz_frame_bytes
    assert fb(640, 480, FMT_YUYV422) == fb(640, 480, FMT_UYVY422) == 2 * 640 * 480
    assert fb(640, 481, FMT_YUYV422) == 2 * 640 * 481 and fb(641, 480, FMT_YUYV422) == 0 and fb(641, 480, FMT_UYVY422) == 0
    assert fb(643, 481, FMT_GRAY8) == 643 * 481 and fb(643, 481, FMT_BGR24) == 3 * 643 * 481
    for base in (FMT_NV12, FMT_I420, FMT_YUYV422, FMT_UYVY422):
        for flags in (CSP_BT709, RANGE_FULL, CSP_BT709 | RANGE_FULL):
            assert fb(640, 480, base | flags) == fb(640, 480, base) > 0
    for base in (FMT_RGB24, FMT_GRAY8, FMT_BGR24):
        for flags in (CSP_BT709, RANGE_FULL, CSP_BT709 | RANGE_FULL):
            assert fb(640, 480, base | flags) == 0
    for word in (7, 9, 0xFF, 0x400 | FMT_NV12, 0x1000, 0x10000 | FMT_RGB24, -1, 1 << 30):
        assert fb(640, 480, word) == 0
    # the words that were there before mean what they meant
    assert (fb(640, 480, 0), fb(640, 480, 1), fb(640, 480, 2), fb(641, 480, 1)) == (640 * 480 * 3, 640 * 480 * 3 // 2, 640 * 480 * 3 // 2, 0)
    # and the restatement sizes and refuses alike
    for w, h in ((640, 480), (641, 480), (640, 481), (643, 481), (2, 2), (1, 1)):
        for word in list(range(10)) + [b | f for b in range(8) for f in (0x100, 0x200, 0x300, 0x400)]:
            assert fb(w, h, word) == px.frame_bytes(w, h, word), (w, h, hex(word))


def test_plugin_names_and_colour_options():
    from watsor_amd.detection.hip_gpu import COLOR_MATRICES, COLOR_RANGES, PIXEL_FORMATS, format_words, frame_formats, pixel_format_code
    assert pixel_format_code("yuyv422") == FMT_YUYV422 and pixel_format_code("UYVY422") == FMT_UYVY422
    assert pixel_format_code("gray") == FMT_GRAY8 and pixel_format_code("yuvj420p") == FMT_I420 | RANGE_FULL
    assert {"yuyv422", "uyvy422", "gray", "yuvj420p", "rgb24", "nv12", "yuv420p"} <= set(PIXEL_FORMATS)
    assert COLOR_MATRICES == {"bt601": 0, "bt709": CSP_BT709} and COLOR_RANGES == {"limited": 0, "full": RANGE_FULL}
    assert format_words({}) == (FMT_RGB24, {})
    assert format_words({"pixel_format": "nv12", "color_matrix": "bt709"}) == (FMT_NV12 | CSP_BT709, {})
    assert format_words({"pixel_format": "yuyv422", "color_range": "full", "color_matrix": "BT709"}) == (FMT_YUYV422 | CSP_BT709 | RANGE_FULL, {})
    assert format_words({"pixel_format": "yuvj420p", "color_matrix": "bt601", "color_range": "limited"}) == (FMT_I420 | RANGE_FULL, {})
    # a matrix / range does not touch a format that has no YUV in it
    assert format_words({"pixel_format": "gray", "color_matrix": "bt709", "color_range": "full"}) == (FMT_GRAY8, {})
    assert format_words({"color_matrix": "bt709"}) == (FMT_RGB24, {})
    # per camera, each option on its own
    dflt, cams = format_words({"pixel_format": {"usb": "yuyv422", "ir": "gray", "hd": "nv12"}, "color_matrix": {"hd": "bt709"},
                               "color_range": {"usb": "full", "door": "full"}})
    assert dflt == FMT_RGB24
    assert cams == {"usb": FMT_YUYV422 | RANGE_FULL, "ir": FMT_GRAY8, "hd": FMT_NV12 | CSP_BT709, "door": FMT_RGB24}
    dflt, cams = format_words({"pixel_format": "nv12", "color_matrix": "bt709", "color_range": {"mjpeg": "full"}})
    assert dflt == FMT_NV12 | CSP_BT709 and cams == {"mjpeg": FMT_NV12 | CSP_BT709 | RANGE_FULL}
    for bad in ({"pixel_format": "p010"}, {"pixel_format": {"a": "yuv422p"}}, {"color_matrix": "bt2020"}, {"color_matrix": {"a": "smpte240m"}},
                {"color_range": "tv"}, {"color_range": {"a": "pc"}}):
        with pytest.raises(ValueError):
            format_words(bad)
    # what a one-channel array holds: a configured gray / 4:2:2 camera keeps its format, and is never what an (H*3/2, W) buffer
    # under an RGB24 camera is taken for
    gray, packed, planar, rgb = np.zeros((4, 4), np.uint8), np.zeros((4, 8), np.uint8), np.zeros((6, 4), np.uint8), np.zeros((4, 4, 3), np.uint8)
    by_cam = {0: FMT_GRAY8, 1: FMT_YUYV422 | RANGE_FULL, 2: FMT_RGB24}
    assert frame_formats([gray, packed, rgb], [0, 1, 2], FMT_RGB24, by_cam) == [FMT_GRAY8, FMT_YUYV422 | RANGE_FULL, FMT_RGB24]
    assert frame_formats([gray[:, :, None]], [0], FMT_RGB24, by_cam) == [FMT_GRAY8]
    assert frame_formats([planar], [2], FMT_RGB24, by_cam) == [FMT_NV12]
    assert frame_formats([planar], [2], FMT_RGB24, {**by_cam, 3: FMT_I420 | CSP_BT709}) ==[FMT_I420 | CSP_BT709]
    assert frame_formats([gray], None, FMT_GRAY8, {}) == [FMT_GRAY8]


def test_frame_table_of_gray_and_packed_cameras(tmp_path, monkeypatch):
    """A configured gray camera's one-channel FrameBuffer is bound as GRAY8 (not as the planar buffer of an NV12 camera), a 4:2:2
    camera's as (H, W, 2) or (H, 2W, 1), and the size check is the library's wz_frame_bytes."""
    from detector_calls import _Frame, fb
    from watsor_amd.detection import hip_gpu

    class Engine:
        def __init__(self, *a, **k):
            self.table = None

        def bind_frames(self, pix, ws, hs, fmts, cams, rows):
            self.table = list(zip(ws, hs, fmts, cams))
        submit_bound = collect_bound = None

    monkeypatch.setattr(hip_gpu, "HipEngine", Engine)
    (tmp_path / hip_gpu.ENGINE_FILE).write_bytes(b"stub")
    opts = {"pixel_format": {"ir": "gray", "usb": "yuyv422", "usb2": "uyvy422", "hd": "nv12"}, "color_matrix": {"hd": "bt709"}, "numa": False}
    det = hip_gpu.HipObjectDetector(str(tmp_path), 0, opts)
    buffers = {"ir": fb(_Frame(64, 48, 1, 64 * 48)), "usb": fb(_Frame(64, 48, 2, 64 * 48 * 2)), "usb2": fb(_Frame(128, 48, 1, 64 * 48 * 2)),
               "hd": fb(_Frame(64, 72, 1, 64 * 48 * 3 // 2)), "door": fb(_Frame(64, 48, 3, 64 * 48 * 3))}
    ids = {"ir": 0, "usb": 1, "usb2": 2, "hd": 3, "door": -1}
    det._adopt_ids(ids)
    det.bind_frame_table(buffers, ids)
    assert det.engine.table == [(64, 48, FMT_RGB24, -1), (64, 48, FMT_NV12 | CSP_BT709, 3), (64, 48, FMT_GRAY8, 0), (64, 48, FMT_YUYV422, 1),
                                (64, 48, FMT_UYVY422, 2)]
    for name, frame in (("ir", _Frame(64, 48, 3, 64 * 48 * 3)), ("usb", _Frame(63, 48, 2, 63 * 48 * 2)), ("usb", _Frame(64, 48, 2, 64 * 48 * 2 - 1)),
                        ("ir", _Frame(64, 48, 1, 64 * 48 - 1))):
        with pytest.raises(ValueError):
            det.bind_frame_table(dict(buffers, **{name: fb(frame)}), ids)
