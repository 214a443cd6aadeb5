"""10-bit 4:2:0 frames (P010, YUV420P10: what an HEVC Main10 stream decodes to) through the HIP path, at every frame entry point.
The colour conversion is integer arithmetic and only decides which bytes a tap is made of: the resize kernels must see exactly
the RGB bytes tests/pixfmt10_oracle.py works out, so everything downstream -- network input, rows -- is bit-identical to the RGB24
path on those bytes; and a frame whose samples are an 8-bit frame's << 2 must give that 8-bit frame's rows.  Both kernels: the
per-pixel form and the row-staged form (WZ_PRE_ROWS=1, and frames read in place from page-locked host memory), and the rule that
keeps a 10-bit frame too wide for the row-staged kernel's LDS away from it."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import conftest
import pixfmt10_oracle as p10
import pixfmt_oracle as px
from watsor_amd.runtime import (CSP_BT709, FMT_I420, FMT_NV12, FMT_P010, FMT_RGB24, FMT_YUV420P10, RANGE_FULL, ROW_DTYPE, tile_grid)
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

FMT = {"p010": FMT_P010, "yuv420p10": FMT_YUV420P10}
EIGHT = {FMT_P010: FMT_NV12, FMT_YUV420P10: FMT_I420}            # the 8-bit format of the same layout
COLOURS = {"601-limited": 0, "601-full": RANGE_FULL, "709-limited": CSP_BT709, "709-full": CSP_BT709 | RANGE_FULL}
IOS = 0.6


def engine_with(model_dir, env, **kw):
    saved = {k: os.environ.get(k) for k in ("WZ_PRE_ROWS", "WZ_HOST_READ")}
    for k in saved:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return conftest.make_engine(model_dir, dev=True, **kw)         # (the knobs are read when the engine is created)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines(model_dir):
    """The per-pixel kernel and the row-staged kernel, one engine each."""
    e = {"pixel": engine_with(model_dir, {"WZ_PRE_ROWS": "0"}), "rows": engine_with(model_dir, {"WZ_PRE_ROWS": "1"})}
    yield e
    for x in e.values():
        x.close()


def _picture(w, h, seed):
    rng = np.random.default_rng(seed)
    return synthetic_frame(w, h, seed) if w > 8 and h > 8 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _case(w, h, word):
    """(frame (H*3/2, W) uint16, the RGB24 frame the restatement converts it to), built once and shared (read-only).  A picture with
    real chroma detail: the synthetic RGB frame converted to the 8-bit format of the same layout, its samples << 2 with random low
    bits, every sample perturbed (so that out-of-range levels, clipping and odd chroma values occur), sprinkled with 0 and 1023,
    and with random bits where a word carries no sample."""
    seed = 31 * w + h + word
    rng = np.random.default_rng(seed)
    base, flags = word & 0xFF, word & ~0xFF
    f8 = px.frame_from_rgb(_picture(w, h, seed), EIGHT[base] | flags)
    y, u, v = (p.astype(np.int32) for p in p10.unpack(p10.from_8bit(f8, w, h, word), w, h, word))
    for p in (y, u, v):
        p += rng.integers(-96, 100, p.shape)
        p[::7, ::5] = rng.choice(np.array([0, 1023]), p[::7, ::5].shape)
        np.clip(p, 0, 1023, out=p)
    f = p10.pack(y, u, v, word, padding=rng.integers(0, 65536, (h * 3 // 2, w)).astype(np.uint16))
    want = p10.rgb_from_frame10(f, w, h, word)
    f.setflags(write=False)
    want.setflags(write=False)
    return f, want


@functools.lru_cache(maxsize=None)
def _shifted(w, h, word, seed):
    """(10-bit frame whose samples are an 8-bit frame's << 2, that 8-bit frame, its format word)"""
    word8 = EIGHT[word & 0xFF] | (word & ~0xFF)
    f8 = px.frame_from_rgb(synthetic_frame(w, h, seed), word8)
    f10 = p10.from_8bit(f8, w, h, word)
    f8.setflags(write=False)
    f10.setflags(write=False)
    return f10, f8, word8


def _same_network_input(eng, w, h, word):
    frame, rgb = _case(w, h, word)
    got = eng.stage_preprocess(frame, word)
    want = eng.stage_preprocess(rgb)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint16), want.view(np.uint16))


def _rows(n):
    return [np.zeros(100, ROW_DTYPE) for _ in range(n)]


# ---- 1. network input ----------------------------------------------------------------------------------------------------------
# one / two chroma samples; identity; a scale just above 1 (several output rows per workgroup of the row-staged kernel); 646x482;
# 1080p (the resize skips rows)
SIZES = [(2, 2), (4, 2), (300, 300), (322, 242), (646, 482), (1920, 1080)]


@pytest.mark.parametrize("kernel", ["pixel", "rows"])
@pytest.mark.parametrize("fmt", list(FMT))
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_resize_kernels_see_the_restated_rgb(engines, kernel, fmt, size):
    _same_network_input(engines[kernel], size[0], size[1], FMT[fmt])


@pytest.mark.parametrize("kernel", ["pixel", "rows"])
@pytest.mark.parametrize("colour", list(COLOURS))
@pytest.mark.parametrize("fmt", list(FMT))
@pytest.mark.parametrize("size", [(4, 2), (322, 242)], ids=["4x2", "322x242"])
def test_every_matrix_and_range_on_both_formats(engines, kernel, colour, fmt, size):
    _same_network_input(engines[kernel], size[0], size[1], FMT[fmt] | COLOURS[colour])


def test_the_flags_change_the_network_input(engines):
    """... so the cases above are not four spellings of one conversion."""
    frame, _ = _case(322, 242, FMT_P010)
    outs = [engines["pixel"].stage_preprocess(frame, FMT_P010 | c).view(np.uint16) for c in COLOURS.values()]
    for i in range(4):
        for j in range(i):
            assert (outs[i] != outs[j]).any()


def test_every_view_of_a_frames_bytes_is_the_same_frame(engines):
    """uint16 (H*3/2, W) and (H*3/2, W, 1), uint8 (H*3/2, W, 2), (H*3/2, 2W) and (H*3/2, 2W, 1): one network input"""
    eng, (w, h) = engines["rows"], (34, 18)
    frame, _ = _case(w, h, FMT_YUV420P10)
    b = frame.view(np.uint8)
    want = eng.stage_preprocess(frame, FMT_YUV420P10).view(np.uint16)
    for view in (frame[:, :, None], b.reshape(h * 3 // 2, w, 2), b.reshape(h * 3 // 2, 2 * w), b.reshape(h * 3 // 2, 2 * w, 1)):
        np.testing.assert_array_equal(eng.stage_preprocess(view, FMT_YUV420P10).view(np.uint16), want)


# ---- 2. rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["pixel", "rows"])
@pytest.mark.parametrize("fmt", list(FMT))
def test_rows_of_a_shifted_8_bit_frame_are_that_frames_rows(engines, kernel, fmt):
    """samples = an NV12 / I420 frame's << 2: the 8-bit frame's rows byte for byte, synchronously and through the asynchronous host path"""
    eng, word = engines[kernel], FMT[fmt] | CSP_BT709
    f10, f8, word8 = _shifted(640, 480, word, 77)
    want, got, again = _rows(1), _rows(1), _rows(1)
    eng.detect_batch([f8], want, formats=[word8])
    eng.detect_batch([f10], got, formats=[word])
    assert got[0].tobytes() == want[0].tobytes() and (want[0]["confidence"] > 0.3).any()
    eng.submit_host(0, [f10], formats=[word])
    eng.collect(0, again)
    assert again[0].tobytes() == want[0].tobytes()


MIXED = [(FMT_RGB24, 640, 480), (FMT_NV12, 1280, 720), (FMT_P010 | CSP_BT709, 646, 482), (FMT_YUV420P10 | RANGE_FULL, 322, 242)]


@pytest.mark.parametrize("kernel", ["pixel", "rows"])
def test_rows_of_a_mixed_batch(engines, kernel):
    """RGB24, NV12, P010 | 709 and YUV420P10 | full frames of different sizes in ONE batch give the rows of the RGB24 frames the
    restatement converts them to, and each of them run alone gives the rows of its RGB24 frame run alone.  (Rows are compared at one batch
    size: a batch size picks the network's summation order -- tests/test_gpu_bound_frames.py, tests/test_gpu_worker.py -- so a frame's rows
    in a batch of four and alone differ in the last bits of a confidence, whatever its format; measured here on RGB24 frames.)"""
    import test_gpu_pixfmt as eight
    eng = engines[kernel]
    frames, as_rgb = zip(*[_case(w, h, word) if (word & 0xFF) in EIGHT else eight._case(w, h, word) for word, w, h in MIXED])
    formats = [word for word, _, _ in MIXED]
    for frame, rgb, word in zip(frames, as_rgb, formats):
        alone, alone_rgb = _rows(1), _rows(1)
        eng.detect_batch([frame], alone, formats=[word])
        eng.detect_batch([rgb], alone_rgb)
        assert alone[0].tobytes() == alone_rgb[0].tobytes(), hex(word)
    ref = _rows(len(frames))
    eng.detect_batch(list(as_rgb), ref)
    got = _rows(len(frames))
    eng.detect_batch(list(frames), got, formats=formats)
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()
    assert any((r["confidence"] > 0.3).any() for r in got)
    eng.submit_host(0, list(frames), formats=formats)
    again = _rows(len(frames))
    eng.collect(0, again)
    for a, b in zip(again, ref):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kernel", ["pixel", "rows"])
def test_frames_at_odd_device_addresses(engines, kernel):
    """A frame one byte off alignment on the device: no 16-bit word of it lies at an even address; same rows."""
    eng = engines[kernel]
    specs = [(FMT_P010, 322, 242), (FMT_YUV420P10 | CSP_BT709, 322, 242)]
    frames, as_rgb = zip(*[_case(w, h, word) for word, w, h in specs])
    ref = _rows(len(frames))
    eng.detect_batch(list(as_rgb), ref)
    ptrs = [eng.upload(np.concatenate([np.zeros(1 + 2 * i, np.uint8), f.view(np.uint8).reshape(-1)])) for i, f in enumerate(frames)]
    try:
        eng.submit_device(0, [p + 1 + 2 * i for i, p in enumerate(ptrs)], [s[1] for s in specs], [s[2] for s in specs],
                          formats=[s[0] for s in specs])
        got = _rows(len(frames))
        eng.collect(0, got)
    finally:
        eng.sync()
        for p in ptrs:
            eng.free(p)
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()
    assert any((r["confidence"] > 0).any() for r in got)


# ---- 3. frames read in place -------------------------------------------------------------------------------------------------------
def _arena(frames, lead=5):
    """the frames' bytes at odd offsets of one array; (arena, uint8 views (H*3/2, 2W) of the frames in it)"""
    arena = np.zeros(sum(f.nbytes for f in frames) + 64 * len(frames) + 16, np.uint8)
    views, off = [], lead
    for i, f in enumerate(frames):
        b = f.view(np.uint8)
        view = arena[off:off + b.size].reshape(b.shape)
        view[...] = b
        assert view.ctypes.data % 2 == 1
        views.append(view)
        off += b.size + 14 + 2 * i
    return arena, views


def _bound_source(e, slot, n):
    out = (C.c_int32 * n)()
    e._ck(e._lib.wz_debug_bound_source(e._h, slot, C.byref(out)))
    return list(out)


def test_frames_read_in_place_give_the_same_rows_as_staged_frames(model_dir):
    """1920x1080 P010 and YUV420P10 frames at odd offsets of one page-locked arena, read in place over PCIe by the row-staged kernel
    (WZ_HOST_READ=1): rows == a staged engine's rows for the restated RGB24 frames, bit for bit -- handed over as host pointers and
    through the frame table, where wz_debug_bound_source tells that they were read in place."""
    specs = [(FMT_P010, 1920, 1080), (FMT_YUV420P10 | CSP_BT709, 1920, 1080)]
    cases = [_case(w, h, word) for word, w, h in specs]
    fmts = [s[0] for s in specs]
    staged = engine_with(model_dir, {"WZ_PRE_ROWS": "0", "WZ_HOST_READ": "0"}, max_batch=4)
    try:
        want = _rows(len(cases))
        staged.detect_batch([rgb for _, rgb in cases], want)
    finally:
        staged.close()
    arena, frames = _arena([f for f, _ in cases])
    direct = engine_with(model_dir, {"WZ_HOST_READ": "1"}, max_batch=4)
    try:
        direct.host_register(arena)
        try:
            direct.submit_host(1, frames, formats=fmts)
            direct.wait(1)
            got = direct.slot_rows(1, len(frames)).copy()
            bound = np.zeros((len(frames), 100), ROW_DTYPE)
            direct.bind_frames([v.ctypes.data for v in frames], [1920] * 2, [1080] * 2, fmts, [-1, -1], [bound[i].ctypes.data for i in range(2)])
            direct.submit_bound(2, [0, 1])
            direct.collect_bound(2)
            assert _bound_source(direct, 2, 2) == [1, 1]
        finally:
            direct.sync()
            direct.bind_frames([], [], [], [], [], [])
            direct.host_unregister(arena)
    finally:
        direct.close()
    for i in range(len(frames)):
        assert got[i].tobytes() == want[i].tobytes(), i
        assert bound[i].tobytes() == want[i].tobytes(), i
        assert got[i]["confidence"][0] > 0


def test_a_frame_too_wide_for_the_row_kernels_lds_takes_the_per_pixel_kernel(model_dir):
    """The LDS rule.  An engine created for frames up to 4096 wide launches the row-staged kernel with 40 KiB of LDS; one output row of a
    P010 frame needs 12 w + 64 bytes.  3842 wide (46 168 bytes) does not fit: the frame gives the network input of its RGB24 restatement
    all the same -- it went to the per-pixel kernel --, and a batch that holds it is staged whole.  3400 wide (40 864 bytes) fits and is
    still read in place."""
    eng = engine_with(model_dir, {"WZ_PRE_ROWS": "1", "WZ_HOST_READ": "1"}, max_batch=2, max_width=4096, max_height=32)
    try:
        wide, wide_rgb = _case(3842, 16, FMT_P010)
        fits, fits_rgb = _case(3400, 16, FMT_P010)
        for frame, rgb in ((wide, wide_rgb), (fits, fits_rgb)):
            np.testing.assert_array_equal(eng.stage_preprocess(frame, FMT_P010).view(np.uint16), eng.stage_preprocess(rgb).view(np.uint16))
        rgb_of = [wide_rgb, fits_rgb]
        arena, views = _arena([wide, fits])
        eng.host_register(arena)
        try:
            bound = np.zeros((2, 100), ROW_DTYPE)
            eng.bind_frames([v.ctypes.data for v in views], [3842, 3400], [16, 16], [FMT_P010] * 2, [-1, -1], [bound[i].ctypes.data for i in range(2)])
            for entries, source in (([1], [1]), ([0], [0]), ([0, 1], [0, 0])):
                bound.view(np.uint8)[...] = 0xA5
                eng.submit_bound(1, entries)
                eng.collect_bound(1)
                assert _bound_source(eng, 1, len(entries)) == source, entries
                want = _rows(len(entries))                               # (at the same batch size: it picks the network's summation order)
                eng.detect_batch([rgb_of[i] for i in entries], want)
                for k, i in enumerate(entries):
                    assert bound[i].tobytes() == want[k].tobytes(), (entries, i)
        finally:
            eng.sync()
            eng.bind_frames([], [], [], [], [], [])
            eng.host_unregister(arena)
    finally:
        eng.close()


# ---- 4. tiled and gated ------------------------------------------------------------------------------------------------------------
SMALL = dict(max_batch=8, max_width=96, max_height=64)


@pytest.fixture(scope="module")
def small(model_dir):
    e = engine_with(model_dir, {}, **SMALL)
    yield e
    e.close()


@pytest.mark.parametrize("fmt", list(FMT))
def test_tiled_detection_equals_the_restated_rgb_frames(small, fmt):
    """64x48, a 2 x 2 grid plus the whole frame: the crop kernel cuts a 2-byte luma plane and one (P010) or two (YUV420P10) chroma planes"""
    word = FMT[fmt] | CSP_BT709
    frame, rgb = _case(64, 48, word)
    rects = tile_grid(64, 48, 2, 2, 0.25, even=True)
    assert len(rects) == 5 and (0, 0, 64, 48) in [tuple(r) for r in rects]
    want, got = _rows(1), _rows(1)
    small.detect_tiled([rgb], [rects], want, ios=IOS)
    small.detect_tiled([frame], [rects], got, formats=[word], ios=IOS)
    assert got[0].tobytes() == want[0].tobytes()
    for rect in rects:                                                   # ... and every crop is the bytes of the frame the oracle cuts
        x0, y0, w, h = rect
        crop = small.stage_crop_tile(frame, rect, word)
        assert crop.size == 3 * w * h
        np.testing.assert_array_equal(p10.rgb_from_frame10(crop, w, h, word), rgb[y0:y0 + h, x0:x0 + w])
    for bad in ((1, 0, 32, 24), (0, 1, 32, 24), (0, 0, 31, 24), (0, 0, 32, 23)):
        with pytest.raises(ValueError, match="P010 / YUV420P10"):
            small.detect_tiled([frame], [[bad]], got, formats=[word], ios=IOS)


def _gated(eng, frame, cam, fmt):
    rows = np.zeros(100, ROW_DTYPE)
    eng.detect_gated([frame], [cam], [rows], formats=[fmt], ios=IOS)
    ran, act = eng.gate_stats(0)
    return rows, ran[0], act[0].tolist()


@pytest.mark.parametrize("fmt", list(FMT))
def test_a_gated_camera_decides_and_answers_as_on_the_8_bit_frame(small, fmt):
    """The gate sums the top 8 bits of the 10-bit lumas (P010: the odd bytes; YUV420P10: bits 2 .. 9 of a word), so sums and threshold
    keep their 8-bit meaning: over still, one cell changed by more than the threshold, still, a camera of 10-bit frames runs the tiles
    its `>> 2` NV12 / I420 twin runs, with the same activity, and returns the same rows.  The padding bits differ from frame to frame
    and decide nothing."""
    word = FMT[fmt]
    word8 = EIGHT[word]
    rects = tile_grid(64, 48, 2, 2, 0.25, even=True)
    a8 = px.frame_from_rgb(synthetic_frame(64, 48, 91), word8)
    b8 = a8.copy()
    b8[16:32, 32:48] = np.clip(b8[16:32, 32:48].astype(np.int32) + 40, 0, 255).astype(np.uint8)   # one cell of luma, 40 levels brighter
    rng = np.random.default_rng(92)

    def ten(f8):
        y, u, v = p10.unpack(p10.from_8bit(f8, 64, 48, word), 64, 48, word)
        return p10.pack(y, u, v, word, padding=rng.integers(0, 65536, (72, 64)).astype(np.uint16))

    cams = (31, 32)
    small.set_camera_tiles(cams[0], 64, 48, rects, 8, 1, 0, fmt=word8)
    small.set_camera_tiles(cams[1], 64, 48, rects, 8, 1, 0, fmt=word)
    try:
        ran = []
        for step, f8 in enumerate((a8, a8, b8, b8)):
            rows8, ran8, act8 = _gated(small, f8, cams[0], word8)
            rows10, ran10, act10 = _gated(small, ten(f8), cams[1], word)
            assert (ran10, act10) == (ran8, act8), step
            assert rows10.tobytes() == rows8.tobytes(), step
            ran.append(ran8)
        assert ran[0] == (1 << len(rects)) - 1 and ran[1] == 0 and ran[2] != 0 and ran[3] == 0
        assert (rows8["confidence"] > 0).any()
    finally:
        small.clear_camera_tiles(cams[0])
        small.clear_camera_tiles(cams[1])


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("fmt", list(FMT))
def test_activity_kernel_sums_the_top_eight_bits(small, fmt, skew):
    """the activity kernel's cell sums of a 10-bit frame, at an even and an odd address, == those of its `>> 2` 8-bit frame"""
    word = FMT[fmt]
    frame, _ = _case(64, 48, word | CSP_BT709)
    f8 = p10.to_8bit(frame, 64, 48, word)
    holder = np.zeros(frame.nbytes + 16, np.uint8)
    at = holder[skew:skew + frame.nbytes].reshape(72, 128)
    at[...] = frame.view(np.uint8)
    assert at.ctypes.data % 2 == skew
    for rect in ((0, 0, 64, 48), (2, 6, 38, 30), (34, 18, 30, 30)):
        got, changed = small.stage_tile_activity(at, rect, word)
        want, _ = small.stage_tile_activity(f8, rect, EIGHT[word])
        assert changed == 0 and got.tobytes() == want.tobytes(), rect


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(engines):
    """Odd width, odd height, base 0x12, an unknown flag bit: ValueError from Python's geometry check, and again from the C ABI
    (submit_device hands the word over unchecked)."""
    eng = engines["pixel"]
    rows = [np.zeros(100, ROW_DTYPE)]
    z16 = lambda *s: np.zeros(s, np.uint16)
    for frame, word in ((z16(720, 641), FMT_P010), (z16(721, 640), FMT_YUV420P10), (z16(720, 640), 0x12), (z16(720, 640), FMT_P010 | 0x400),
                        (z16(720, 640), FMT_NV12)):
        with pytest.raises(ValueError):
            eng.detect_batch([frame], rows, formats=[word])
        with pytest.raises(ValueError):
            eng.submit_host(0, [frame], formats=[word])
    d = eng.upload(z16(721, 642))
    try:
        for w, h, word in ((641, 480, FMT_P010), (640, 481, FMT_P010), (641, 480, FMT_YUV420P10), (640, 481, FMT_YUV420P10 | CSP_BT709),
                           (640, 480, 0x12), (640, 480, 0x0F), (640, 480, FMT_P010 | 0x400), (640, 480, FMT_YUV420P10 | 0x1000)):
            with pytest.raises(ValueError):
                eng.submit_device(0, [d], [w], [h], formats=[word])
        eng.submit_device(0, [d], [640], [480], formats=[FMT_P010 | CSP_BT709 | RANGE_FULL])      # (and a good word is taken)
        eng.wait(0)
    finally:
        eng.sync()
        eng.free(d)
