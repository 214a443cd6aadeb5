"""Tiled detection on the GPU (include/watsor_hip.h: wz_detect_tiled): the crop kernel against numpy slicing, the
merge kernel against tests/tile_oracle.py, and the whole call against `detect_batch` of the same crops merged by the oracle -- all
byte for byte."""
import ctypes as C

import numpy as np
import pytest

import refusal_golden
import tile_oracle as to
from conftest import make_engine
from test_tile_oracle import KNOWN, rows_of
from watsor_amd import _lib
from watsor_amd.filter.hip_filter import HipCameraFilter
from watsor_amd.runtime import (FMT_BGR24, FMT_GRAY8, FMT_I420, FMT_NV12, FMT_RGB24, FMT_UYVY422, FMT_YUYV422, ROW_DTYPE, RANGE_FULL,
                                tile_grid)
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

SIZE = dict(max_batch=8, max_width=640, max_height=480)
EVEN_BOTH, EVEN_X = (FMT_NV12, FMT_I420), (FMT_YUYV422, FMT_UYVY422)


@pytest.fixture(scope="module")
def dev_eng(model_dir_default):
    e = make_engine(model_dir_default, dev=True, **SIZE)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng(model_dir):
    e = make_engine(model_dir, **SIZE)
    yield e
    e.close()


# ---- 1. crop ------------------------------------------------------------------------------------------------------------------------
def crop_cases(fmt):
    """(w, h, rectangles) of the small frame of a format: 1x1 (2x2), the whole frame, odd origin and width where the format takes them,
    tiles touching the right edge, the bottom edge and both"""
    if fmt in EVEN_BOTH:
        w, h = 34, 22
        return w, h, [(0, 0, 2, 2), (16, 10, 2, 2), (0, 0, w, h), (4, 2, 18, 12), (20, 4, 14, 8), (6, 12, 10, 10), (18, 14, 16, 8)]
    if fmt in EVEN_X:
        w, h = 34, 22
        return w, h, [(0, 0, 2, 1), (16, 11, 2, 1), (0, 0, w, h), (4, 3, 18, 11), (20, 5, 14, 7), (6, 13, 10, 9), (18, 15, 16, 7)]
    w, h = 37, 23
    return w, h, [(0, 0, 1, 1), (17, 11, 1, 1), (0, 0, w, h), (5, 3, 17, 11), (3, 1, 21, 19), (20, 5, 17, 7), (7, 13, 9, 10), (19, 15, 18, 8)]


def random_frame(w, h, fmt, seed, skew=0):
    """random bytes of a w x h frame in the shape `frame_geometry` takes, `skew` bytes past an aligned address"""
    shape = to.tile_shape(w, h, fmt)
    n = int(np.prod(shape))
    buf = np.zeros(n + 64, np.uint8)
    start = (-buf.ctypes.data) % 16 + skew
    view = buf[start:start + n]
    view[:] = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    assert view.ctypes.data % 16 == skew
    return view.reshape(shape)


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("fmt", [FMT_RGB24, FMT_BGR24, FMT_GRAY8, FMT_YUYV422, FMT_UYVY422, FMT_NV12, FMT_I420])
def test_crop_is_numpy_slicing(dev_eng, fmt, skew):
    w, h, rects = crop_cases(fmt)
    frame = random_frame(w, h, fmt, 100 + fmt, skew)
    for rect in rects:
        got = dev_eng.stage_crop_tile(frame, rect, fmt)
        want = to.crop(frame, w, h, fmt, rect)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (fmt, rect)


@pytest.mark.parametrize("skew", [0, 3])
def test_crop_of_a_large_rgb_frame(dev_eng, skew):
    frame = random_frame(640, 480, FMT_RGB24, 7, skew)
    rect = (319, 239, 321, 241)
    assert dev_eng.stage_crop_tile(frame, rect).tobytes() == to.crop(frame, 640, 480, FMT_RGB24, rect).tobytes()


# ---- 2. merge -----------------------------------------------------------------------------------------------------------------------
def random_tile_rows(n_tiles, seed):
    """seeded rows: labels 1 .. 5, integer boxes inside a 320 x 240 frame, confidences from 50 values (ties), a few padding rows"""
    rng = np.random.default_rng(seed)
    tiles, rows = [], np.zeros((n_tiles, 100), ROW_DTYPE)
    levels = np.float32(rng.random(50) * 0.9 + 0.05).astype(np.float64)
    for t in range(n_tiles):
        tw, th = int(rng.integers(60, 200)), int(rng.integers(60, 160))
        x0, y0 = int(rng.integers(0, 320 - tw + 1)), int(rng.integers(0, 240 - th + 1))
        tiles.append((x0, y0, tw, th))
        n = int(rng.integers(80, 101))
        bw, bh = rng.integers(4, 60, 100), rng.integers(4, 60, 100)
        bx, by = rng.integers(0, tw - 3, 100), rng.integers(0, th - 3, 100)
        rows[t]["label"] = rng.integers(1, 6, 100)
        rows[t]["confidence"] = np.sort(rng.choice(levels, 100))[::-1]
        rows[t]["x_min"], rows[t]["y_min"] = bx, by
        rows[t]["x_max"], rows[t]["y_max"] = np.minimum(bx + bw, tw - 1), np.minimum(by + bh, th - 1)
        rows[t][n:] = to.padding_row()
    return tiles, rows


@pytest.fixture(scope="module")
def merge_inputs():
    return {t: random_tile_rows(t, 40 + t) for t in (1, 3, 64)}


def check_merge(eng, tiles, rows, iou, ios, what):
    got, ok = eng.stage_merge_tiles(320, 240, tiles, rows, iou, ios)
    want = to.merge_tiles(tiles, rows, iou, ios)
    assert got.tobytes() == want.tobytes(), what
    np.testing.assert_array_equal(ok, (want["label"] > 0).astype(np.uint8), what)
    return want


@pytest.mark.parametrize("iou,ios", [(0.6, 1.0), (0.6, 0.5), (1.0, 1.0), (0.0, 0.0)])
@pytest.mark.parametrize("n_tiles", [1, 3, 64])
def test_merge_matches_the_oracle(dev_eng, merge_inputs, n_tiles, iou, ios):
    tiles, rows = merge_inputs[n_tiles]
    want = check_merge(dev_eng, tiles, rows, iou, ios, (n_tiles, iou, ios))
    kept = int((want["confidence"] > 0).sum())
    assert kept == 100 if (iou, ios) == (1.0, 1.0) and n_tiles > 1 else kept >= 1


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_merge_known_answers_on_the_gpu(dev_eng, name):
    tiles, rows, iou, ios, _ = KNOWN[name]
    check_merge(dev_eng, tiles, rows, iou, ios, name)


def test_merge_crafted_rows(dev_eng):
    rows = rows_of([(1, float("nan"), (1, 1, 50, 50)), (0, 0.9, (1, 1, 50, 50)), (2, -0.5, (1, 1, 50, 50)), (2, 0.4, (-7, 300, 400, 310)),
                    (2, 0.3, (250, 200, 330, 260)), (2, 0.3, (251, 200, 330, 260)), (7, float("inf"), (0, 0, 9, 9)), (7, 0.5, (0, 0, 9, 9)), (8, 5e-324, (0, 0, 9, 9))])
    far = rows_of([(2, 0.35, (-100, -100, -20, -40)), (2, 0.2, (2 ** 30, 5, 2 ** 30 + 80, 65))])
    want = check_merge(dev_eng, [(30, 40, 100, 100), (300, 220, 20, 20)], np.stack([rows, far]), 0.6, 0.5, "crafted")
    assert want["confidence"][0] == np.inf and (want["confidence"] > 0).sum() == 6


def test_merge_applies_the_camera_filter(dev_eng, merge_inputs):
    """zone mask + drop mode: what stays is `filter_rows` of the merged rows -- zones written, failing rows zeroed, pass bytes"""
    alpha = np.zeros((240, 320), np.uint8)
    alpha[:, 160:] = 255
    cfg = {"width": 320, "height": 240, "detect": [{"person": {"area": 1, "confidence": 40, "zones": []}},
                                                   {"bicycle": {"area": 0, "confidence": 10, "zones": [1]}},
                                                   {"car": {"area": 5, "confidence": 60, "zones": []}}]}
    flt = HipCameraFilter(dev_eng, 11, cfg, alpha=alpha, drop=True)
    try:
        for n_tiles in (3, 64):
            tiles, rows = merge_inputs[n_tiles]
            got, ok = dev_eng.stage_merge_tiles(320, 240, tiles, rows, 0.6, 0.5, cam=11)
            want = to.merge_tiles(tiles, rows, 0.6, 0.5)
            want_ok = dev_eng.filter_rows(11, want)
            assert got.tobytes() == want.tobytes()
            np.testing.assert_array_equal(ok, want_ok)
            assert 0 < want_ok.sum() < 100 and want["zones"].any() and (want["label"] == 0).any()
    finally:
        flt.close()


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------
def tiled_and_reference(eng, frames, sizes, formats, tiles, iou, ios, device=False):
    """(rows of the tiled call [n, 100], the oracle's merge of `detect_batch` of the same crops) -- one batch of sum(tiles) images each"""
    n = len(frames)
    got = np.zeros((n, 100), ROW_DTYPE)
    passes = np.full((n, 100), 9, np.uint8)
    if device:
        ptrs = [eng.upload(f) for f in frames]
        eng.submit_tiled_device(1, ptrs, [s[0] for s in sizes], [s[1] for s in sizes], tiles, formats=formats, iou=iou, ios=ios)
        eng.collect(1, list(got), list(passes))
        np.testing.assert_array_equal(eng.slot_rows(1, n).view(np.uint8), got.view(np.uint8))
        for p in ptrs:
            eng.free(p)
    else:
        eng.detect_tiled(frames, tiles, list(got), passes=list(passes), formats=formats, iou=iou, ios=ios)
    eng.sync()
    crops, crop_formats = [], []
    for f, (w, h), fmt, rects in zip(frames, sizes, formats, tiles):
        for r in rects:
            crops.append(to.crop(f, w, h, fmt, r).reshape(to.tile_shape(r[2], r[3], fmt)))
            crop_formats.append(fmt)
    tile_rows = np.zeros((len(crops), 100), ROW_DTYPE)
    eng.detect_batch(crops, list(tile_rows), formats=crop_formats)
    want, k = np.zeros((n, 100), ROW_DTYPE), 0
    for i, rects in enumerate(tiles):
        want[i] = to.merge_tiles(rects, tile_rows[k:k + len(rects)], eng.nms_iou if iou is None else iou, 1.0 if ios is None else ios)
        k += len(rects)
    np.testing.assert_array_equal(passes, (want["label"] > 0).astype(np.uint8))
    return got, want, tile_rows


RECTS = [(0, 0, 64, 48), (31, 15, 65, 49), (0, 0, 96, 64)]
EVEN_RECTS = [(0, 0, 64, 48), (30, 14, 66, 50), (0, 0, 96, 64)]


def nv12_of(rgb):
    from pixfmt_oracle import frame_from_rgb
    return frame_from_rgb(rgb, FMT_NV12)


def test_tiled_equals_batch_of_crops_rgb(eng):
    frame = synthetic_frame(96, 64, 31)
    got, want, tile_rows = tiled_and_reference(eng, [frame], [(96, 64)], [FMT_RGB24], [RECTS], None, 0.6)
    assert got.tobytes() == want.tobytes()
    assert (tile_rows["confidence"] > 0).sum() > (want["confidence"] > 0).sum() > 0      # (the merge had something to merge)


def test_tiled_equals_batch_of_crops_nv12(eng):
    frame = nv12_of(synthetic_frame(96, 64, 32))
    got, want, _ = tiled_and_reference(eng, [frame], [(96, 64)], [FMT_NV12 | RANGE_FULL], [EVEN_RECTS], 0.5, 0.6)
    assert got.tobytes() == want.tobytes() and (want["confidence"] > 0).any()


def test_tiled_two_frames_of_different_sizes_and_formats(eng):
    frames = [synthetic_frame(96, 64, 33), nv12_of(synthetic_frame(128, 80, 34))]
    tiles = [[(0, 0, 64, 48), (33, 17, 63, 47)], [(0, 0, 64, 48), (64, 32, 64, 48), (0, 0, 128, 80)]]
    got, want, _ = tiled_and_reference(eng, frames, [(96, 64), (128, 80)], [FMT_RGB24, FMT_NV12], tiles, None, 0.6)
    assert got.tobytes() == want.tobytes() and (want["confidence"] > 0).any(axis=1).all()


# ---- 4. identity ----------------------------------------------------------------------------------------------------------------------
def test_one_tile_equal_to_the_frame_is_detect_batch(eng):
    """... with the camera's filter: the filter sees frame coordinates"""
    frame = synthetic_frame(320, 240, 35)
    alpha = np.zeros((240, 320), np.uint8)
    alpha[:, :200] = 255
    cfg = {"width": 320, "height": 240, "detect": [{name: {"area": 1, "confidence": 20, "zones": []}}
                                                   for name in ("person", "car", "bench", "bird", "cat", "dog")]}
    flt = HipCameraFilter(eng, 5, cfg, alpha=alpha)
    try:
        want, want_ok = np.zeros(100, ROW_DTYPE), np.full(100, 9, np.uint8)
        eng.detect_batch([frame], [want], cams=[5], out_pass=[want_ok])
        got, ok = np.zeros(100, ROW_DTYPE), np.full(100, 9, np.uint8)
        eng.detect_tiled([frame], [[(0, 0, 320, 240)]], [got], cams=[5], passes=[ok], iou=1.0, ios=1.0)
        assert got.tobytes() == want.tobytes()
        np.testing.assert_array_equal(ok, want_ok)
        assert (want["confidence"] > 0).any()
    finally:
        flt.close()


# ---- 5. device path -------------------------------------------------------------------------------------------------------------------
def test_device_path_and_the_untiled_batch_behind_it(eng):
    frame = synthetic_frame(96, 64, 31)
    other = [synthetic_frame(160, 120, 36), synthetic_frame(96, 64, 37)]
    ptrs = [eng.upload(f) for f in other]

    def untiled():
        rows = np.zeros((2, 100), ROW_DTYPE)
        eng.submit_device(1, ptrs, [160, 96], [120, 64])
        eng.collect(1, list(rows))
        return rows.tobytes(), eng.graph_nodes(1), eng.slot_rows(1, 2).tobytes()

    before = untiled()
    got, want, _ = tiled_and_reference(eng, [frame], [(96, 64)], [FMT_RGB24], [RECTS], None, 0.6, device=True)
    assert got.tobytes() == want.tobytes()
    after = untiled()
    assert after == before and after[0] == after[2]
    for p in ptrs:
        eng.free(p)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_engine_usable(eng):
    frame = synthetic_frame(96, 64, 31)
    nv12 = nv12_of(frame)
    yuyv = np.zeros((64, 96, 2), np.uint8)
    nan = float("nan")
    one = [(0, 0, 64, 48)]
    bad = [   # (frames, tiles, formats, iou, ios, code)
        ([], [], None, 0.6, 1.0, _lib.WZ_ELIMIT),
        ([frame] * 9, [one] * 9, None, 0.6, 1.0, _lib.WZ_ELIMIT),
        ([frame], [[]], None, 0.6, 1.0, _lib.WZ_ELIMIT),
        ([frame], [[(0, 0, 1, 1)] * 65], None, 0.6, 1.0, _lib.WZ_ELIMIT),
        ([frame, frame], [one * 5, one * 4], None, 0.6, 1.0, _lib.WZ_ELIMIT),
        ([frame], [[(0, 0, 0, 10)]], None, 0.6, 1.0, _lib.WZ_EINVAL),
        ([frame], [[(0, 0, 10, 0)]], None, 0.6, 1.0, _lib.WZ_EINVAL),
        ([frame], [[(-1, 0, 10, 10)]], None, 0.6, 1.0, _lib.WZ_EINVAL),
        ([frame], [[(0, -1, 10, 10)]], None, 0.6, 1.0, _lib.WZ_EINVAL),
        ([frame], [[(90, 0, 7, 10)]], None, 0.6, 1.0, _lib.WZ_EINVAL),
        ([frame], [[(0, 60, 10, 5)]], None, 0.6, 1.0, _lib.WZ_EINVAL),
        ([frame], [[(2 ** 31 - 1, 0, 2 ** 31 - 1, 5)]], None, 0.6, 1.0, _lib.WZ_EINVAL),
        ([nv12], [[(1, 0, 10, 10)]], [FMT_NV12], 0.6, 1.0, _lib.WZ_EINVAL),
        ([nv12], [[(0, 1, 10, 10)]], [FMT_I420], 0.6, 1.0, _lib.WZ_EINVAL),
        ([nv12], [[(0, 0, 11, 10)]], [FMT_NV12], 0.6, 1.0, _lib.WZ_EINVAL),
        ([nv12], [[(0, 0, 10, 11)]], [FMT_I420], 0.6, 1.0, _lib.WZ_EINVAL),
        ([yuyv], [[(1, 0, 10, 10)]], [FMT_YUYV422], 0.6, 1.0, _lib.WZ_EINVAL),
        ([yuyv], [[(0, 0, 11, 10)]], [FMT_UYVY422], 0.6, 1.0, _lib.WZ_EINVAL),
        ([frame], [one], None, nan, 1.0, _lib.WZ_EINVAL),
        ([frame], [one], None, 0.6, nan, _lib.WZ_EINVAL),
        ([frame], [one], None, -0.1, 1.0, _lib.WZ_EINVAL),
        ([frame], [one], None, 0.6, -1.0, _lib.WZ_EINVAL),
    ]
    lib, h = eng._lib, eng._h
    good = np.zeros(100, ROW_DTYPE)
    eng.detect_tiled([frame], [RECTS], [good], ios=0.6)
    for case, (frames, tiles, formats, iou, ios, code) in enumerate(bad):
        n = len(frames)
        rows = np.full((max(n, 1), 100 * 72), 0xA5, np.uint8)
        passes = np.full((max(n, 1), 100), 0xA5, np.uint8)
        counts, tptrs, keep, _, _ = eng._tile_args(tiles, n, iou, ios)
        ws = (C.c_int32 * max(n, 1))(*[eng.frame_geometry(f, fm)[0] for f, fm in zip(frames, formats or [FMT_RGB24] * n)])
        hs = (C.c_int32 * max(n, 1))(*[eng.frame_geometry(f, fm)[1] for f, fm in zip(frames, formats or [FMT_RGB24] * n)])
        fptr = (C.c_void_p * max(n, 1))(*[f.ctypes.data for f in frames])
        fmtv = (C.c_int32 * n)(*formats) if formats else None
        outs = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in rows][:max(n, 1)])
        pv = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in passes][:max(n, 1)])
        rc = lib.wz_detect_tiled(h, n, fptr, ws, hs, fmtv, None, counts, tptrs, iou, ios, outs, pv, None)
        assert rc == code, (tiles, formats, iou, ios, _lib.last_error(lib))
        refusal_golden.check("tiled", "%d/wz_detect_tiled" % case, rc, _lib.last_error(lib))
        assert (rows == 0xA5).all() and (passes == 0xA5).all()
        # the device entry point refuses the same way (host pointers stand in: a refused call reads no frame) and enqueues nothing
        rc = lib.wz_submit_tiled_device(h, 2, n, fptr, ws, hs, fmtv, None, counts, tptrs, iou, ios)
        assert rc == code, (tiles, formats, iou, ios, _lib.last_error(lib))
        refusal_golden.check("tiled", "%d/wz_submit_tiled_device" % case, rc, _lib.last_error(lib))
    counts, tptrs, keep, _, _ = eng._tile_args([one * 5, one * 4], 2, 0.6, 1.0)
    rc = lib.wz_detect_tiled(h, 2, (C.c_void_p * 2)(frame.ctypes.data, frame.ctypes.data), (C.c_int32 * 2)(96, 96), (C.c_int32 * 2)(64, 64), None,
                             None, counts, tptrs, 0.6, 1.0, None, None, None)
    assert rc == _lib.WZ_ELIMIT
    assert "9" in _lib.last_error(lib) and "8" in _lib.last_error(lib)               # the message names both numbers
    refusal_golden.check("tiled", "nine_tiles_no_outputs", rc, _lib.last_error(lib))
    again = np.zeros(100, ROW_DTYPE)
    eng.detect_tiled([frame], [RECTS], [again], ios=0.6)
    assert again.tobytes() == good.tobytes()


# ---- 7. plugin ------------------------------------------------------------------------------------------------------------------------
def test_plugin_tiles_option(model_dir_default):
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    from watsor_amd.share import DetectionArray
    frame = synthetic_frame(320, 240, 38)
    rows = DetectionArray()
    with HipObjectDetector(model_dir_default, 0, {"tiles": {"grid": [2, 2], "overlap": 0.25}, "numa": False}, **SIZE) as det:
        det.detect(frame.shape, frame, rows)
        want = np.zeros(100, ROW_DTYPE)
        det.engine.detect_tiled([frame], [tile_grid(320, 240, 2, 2, 0.25)], [want])
        assert bytes(rows) == want.tobytes() and (want["confidence"] > 0).any()
        # several frames: the batch is cut where the tiles no longer fit max_batch (5 tiles per frame, 8 per call)
        frames = [frame, synthetic_frame(320, 240, 39)]
        out = [DetectionArray(), DetectionArray()]
        det.detect_batch([f.shape for f in frames], frames, out)
        assert bytes(out[0]) == want.tobytes()
        det.engine.detect_tiled([frames[1]], [tile_grid(320, 240, 2, 2, 0.25)], [want])
        assert bytes(out[1]) == want.tobytes()

        class FB:
            frames = []
        with pytest.raises(ValueError, match="porch"):
            det.bind_frame_table({"porch": FB()}, {"porch": -1})
        assert det.tiled
        with pytest.raises(ValueError, match="tiles"):                  # the asynchronous host path would detect untiled
            det.submit_host(0, [frame])
