"""Gated tiled detection on the GPU (include/watsor_hip.h: wz_set_camera_tiles / wz_detect_gated): the activity kernel
against tests/gate_oracle.py, the tiles that run against its GateState, and the rows against `detect_batch` of the same crops merged by
tests/tile_oracle.py -- all byte for byte."""
import ctypes as C

import numpy as np
import pytest

import gate_oracle as go
import refusal_golden
import tile_oracle as to
from conftest import make_engine
from test_gpu_tiled import EVEN_RECTS, RECTS, SIZE, crop_cases, nv12_of, random_frame
from watsor_amd import _lib
from watsor_amd.coco import COCO_CLASSES
from watsor_amd.filter.hip_filter import HipCameraFilter
from watsor_amd.runtime import (FMT_BGR24, FMT_GRAY8, FMT_I420, FMT_NV12, FMT_RGB24, FMT_UYVY422, FMT_YUYV422, ROW_DTYPE, RANGE_FULL)
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

IOS = 0.6
ALL = 0b111


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


@pytest.fixture
def cams(eng):
    """camera ids a test may set tiles for; whatever it set is cleared behind it"""
    ids = [21, 22, 23]
    yield ids
    for c in ids:
        eng.clear_camera_tiles(c)


def gated(eng, frame, cam, fmt=None, iou=None):
    """(rows, pass bytes, tiles that ran as a bit mask, activity) of one gated call of one frame"""
    rows, ok = np.zeros(100, ROW_DTYPE), np.full(100, 9, np.uint8)
    eng.detect_gated([frame], [cam], [rows], passes=[ok], formats=None if fmt is None else [fmt], iou=iou, ios=IOS)
    ran, act = eng.gate_stats(0)
    return rows, ok, ran[0], act[0]


def grids_of(frame, w, h, fmt, rects):
    return [go.cell_sums(frame, w, h, fmt, r) for r in rects]


# ---- 1. the activity kernel -----------------------------------------------------------------------------------------------------------
def check_activity(eng, frame, w, h, fmt, rect, seed, thrs=(0, 3), oracle=None):
    """oracle: (frame, format word) the oracle sums instead -- for a 10-bit frame, the 8-bit frame of its samples' top eight bits"""
    want = go.cell_sums(frame, w, h, fmt, rect) if oracle is None else go.cell_sums(oracle[0], w, h, oracle[1], rect)
    got, changed = eng.stage_tile_activity(frame, rect, fmt)
    assert got.dtype == np.uint16 and got.shape == want.shape and got.tobytes() == want.tobytes(), (fmt, rect)
    assert changed == 0
    # a reference whose cells lie at, just below and just above multiples of the cell's pixels away from the frame's sums
    rng = np.random.default_rng(seed)
    ref = want.astype(np.int64) + rng.integers(-4, 5, want.shape) * go.cell_pixels(rect) + rng.integers(-1, 2, want.shape)
    ref = np.clip(ref, 0, 65535).astype(np.uint16)
    for thr in thrs:
        got, changed = eng.stage_tile_activity(frame, rect, fmt, ref=ref, pixel_thr=thr)
        assert got.tobytes() == want.tobytes(), (fmt, rect, thr)
        assert changed == go.activity(want, ref, rect, thr), (fmt, rect, thr)


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("fmt", [FMT_RGB24, FMT_BGR24, FMT_GRAY8, FMT_YUYV422, FMT_UYVY422, FMT_NV12, FMT_I420])
def test_activity_kernel_is_the_oracle(dev_eng, fmt, skew):
    w, h, rects = crop_cases(fmt)
    frame = random_frame(w, h, fmt, 200 + fmt, skew)
    for i, rect in enumerate(rects):
        check_activity(dev_eng, frame, w, h, fmt, rect, 10 * fmt + i)


def test_activity_of_a_rectangle_over_several_workgroups(dev_eng):
    """300 x 200 RGB24 at an odd address, a rectangle with ragged ends on every side: 12 strips of cells, rows of 831 bytes"""
    frame = random_frame(300, 200, FMT_RGB24, 8, 3)
    check_activity(dev_eng, frame, 300, 200, FMT_RGB24, (5, 3, 277, 190), 99)


# ---- 2. the first call is the ungated call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rgb", "nv12"])
def test_first_call_equals_the_ungated_call(eng, cams, kind):
    frame = synthetic_frame(96, 64, 31)
    fmt, rects = FMT_RGB24, RECTS
    if kind == "nv12":
        frame, fmt, rects = nv12_of(frame), FMT_NV12 | RANGE_FULL, EVEN_RECTS
    eng.set_camera_tiles(cams[0], 96, 64, rects, 8, 1, 0, fmt=fmt)
    want, want_ok = np.zeros(100, ROW_DTYPE), np.full(100, 9, np.uint8)
    eng.detect_tiled([frame], [rects], [want], cams=[cams[0]], passes=[want_ok], formats=[fmt], ios=IOS)
    got, ok, ran, act = gated(eng, frame, cams[0], fmt)
    assert got.tobytes() == want.tobytes() and ok.tobytes() == want_ok.tobytes()
    assert ran == ALL and (want["confidence"] > 0).any()


# ---- 3. a still picture ---------------------------------------------------------------------------------------------------------------------
def test_still_picture_runs_nothing_and_repeats_the_rows(eng, cams):
    frame = synthetic_frame(96, 64, 31)
    eng.set_camera_tiles(cams[0], 96, 64, RECTS, 8, 1, 0)
    first, first_ok, ran, _ = gated(eng, frame, cams[0])
    assert ran == ALL
    for _ in range(2):
        rows, ok, ran, act = gated(eng, frame, cams[0])
        assert ran == 0 and act.tolist() == [0, 0, 0]
        assert rows.tobytes() == first.tobytes() and ok.tobytes() == first_ok.tobytes()


# ---- 4. one tile changes ----------------------------------------------------------------------------------------------------------------------
def crops_rows(eng, frame, rects):
    """the rows of one `detect_batch` of these crops of a 96 x 64 RGB frame, in order"""
    crops = [np.ascontiguousarray(frame[y:y + h, x:x + w]) for x, y, w, h in rects]
    rows = np.zeros((len(crops), 100), ROW_DTYPE)
    eng.detect_batch(crops, list(rows))
    return rows


def test_one_changed_tile_runs_and_the_others_keep_their_rows(eng, cams):
    a = synthetic_frame(96, 64, 31)
    b = a.copy()
    b[:48, :30] = synthetic_frame(96, 64, 41)[:48, :30]        # inside tile 0 and the full-frame tile only
    thr = 8
    state = go.GateState(3, thr)
    assert state.step(grids_of(a, 96, 64, FMT_RGB24, RECTS), RECTS)[0] == [0, 1, 2]
    predicted, want_act = state.step(grids_of(b, 96, 64, FMT_RGB24, RECTS), RECTS)
    assert predicted == [0, 2]                                  # (precondition: the change is large enough and misses tile 1)
    eng.set_camera_tiles(cams[0], 96, 64, RECTS, thr, 1, 0)
    _, _, ran, _ = gated(eng, a, cams[0])
    assert ran == ALL
    got, ok, ran, act = gated(eng, b, cams[0])
    assert [t for t in range(3) if ran >> t & 1] == predicted and act.tolist() == want_act
    rows_a = crops_rows(eng, a, RECTS)
    fresh = crops_rows(eng, b, [RECTS[0], RECTS[2]])
    assert fresh[0].tobytes() != rows_a[0].tobytes()            # (precondition: tile 0 sees something else in B)
    want = to.merge_tiles(RECTS, np.stack([fresh[0], rows_a[1], fresh[1]]), eng.nms_iou, IOS)
    assert got.tobytes() == want.tobytes()
    np.testing.assert_array_equal(ok, (want["label"] > 0).astype(np.uint8))


# ---- 5. drift -----------------------------------------------------------------------------------------------------------------------------------
def test_drift_accumulates_against_the_reference(eng, cams):
    a = np.minimum(synthetic_frame(96, 64, 31), 200).astype(np.uint8)
    eng.set_camera_tiles(cams[0], 96, 64, RECTS, 2, 1, 0)
    out = [gated(eng, a + np.uint8(k), cams[0]) for k in range(4)]
    assert [o[2] for o in out] == [ALL, 0, 0, ALL]
    assert out[2][0].tobytes() == out[0][0].tobytes() and out[2][1].tobytes() == out[0][1].tobytes()
    cells = [int(np.prod(go.grid_shape(r))) for r in RECTS]
    assert out[3][3].tolist() == cells and out[2][3].tolist() == [0, 0, 0]      # +3 a pixel moves every cell, +2 none


# ---- 6. max_age, reset, a new layout ------------------------------------------------------------------------------------------------------------
def test_max_age_reset_and_a_new_layout(eng, cams):
    frame = synthetic_frame(96, 64, 31)
    eng.set_camera_tiles(cams[0], 96, 64, RECTS, 8, 1, 2)
    assert [gated(eng, frame, cams[0])[2] for _ in range(5)] == [ALL, 0, 0, ALL, 0]
    eng.reset_camera_tiles(cams[0])
    assert [gated(eng, frame, cams[0])[2] for _ in range(2)] == [ALL, 0]
    eng.set_camera_tiles(cams[0], 96, 64, RECTS[:2], 8, 1, 0)
    assert [gated(eng, frame, cams[0])[2] for _ in range(3)] == [0b11, 0, 0]


# ---- 7. the camera filter -------------------------------------------------------------------------------------------------------------------------
def test_camera_filter_runs_on_cached_rows(eng, cams):
    frame = synthetic_frame(96, 64, 31)
    cam = cams[0]
    cfg = lambda conf: {"width": 96, "height": 64, "detect": [{name: {"area": 0, "confidence": conf, "zones": []}}      # noqa: E731
                                                                for name in COCO_CLASSES[1:]]}
    merged = np.zeros(100, ROW_DTYPE)
    eng.detect_tiled([frame], [RECTS], [merged], ios=IOS)       # the merged rows before any filter
    eng.set_camera_tiles(cam, 96, 64, RECTS, 8, 1, 0)
    flt = HipCameraFilter(eng, cam, cfg(0))
    try:
        assert gated(eng, frame, cam)[2] == ALL
        want = merged.copy()
        want_ok = eng.filter_rows(cam, want)
        rows, ok, ran, _ = gated(eng, frame, cam)
        assert ran == 0 and rows.tobytes() == want.tobytes()
        np.testing.assert_array_equal(ok, want_ok)
    finally:
        flt.close()
    flt = HipCameraFilter(eng, cam, cfg(100), drop=True)       # nothing is that confident: every row fails and is zeroed
    try:
        new = merged.copy()
        new_ok = eng.filter_rows(cam, new)
        assert want_ok.any() and not np.array_equal(new_ok, want_ok)          # (precondition: the two filters disagree)
        rows, ok, ran, _ = gated(eng, frame, cam)
        assert ran == 0 and rows.tobytes() == new.tobytes()
        np.testing.assert_array_equal(ok, new_ok)
    finally:
        flt.close()


# ---- 8. neighbours ----------------------------------------------------------------------------------------------------------------------------------
def test_other_calls_between_two_gated_calls(eng, cams):
    frame, other = synthetic_frame(96, 64, 31), synthetic_frame(128, 80, 34)
    rects2 = [(0, 0, 64, 48), (64, 32, 64, 48)]

    def tiled():
        rows = np.zeros(100, ROW_DTYPE)
        eng.detect_tiled([other], [rects2], [rows], ios=IOS)
        return rows.tobytes()

    def batch():
        rows = np.zeros((2, 100), ROW_DTYPE)
        eng.detect_batch([other, frame], list(rows))
        return rows.tobytes()

    alone = tiled(), batch()
    eng.set_camera_tiles(cams[0], 96, 64, RECTS, 8, 1, 0)
    eng.set_camera_tiles(cams[1], 128, 80, rects2, 8, 1, 0)
    first, first_ok, ran, _ = gated(eng, frame, cams[0])
    assert ran == ALL
    between = tiled(), batch()
    theirs, _, ran, _ = gated(eng, other, cams[1])
    assert ran == 0b11 and theirs.tobytes() == alone[0]        # (the other camera's first call is its ungated call)
    rows, ok, ran, act = gated(eng, frame, cams[0])
    assert ran == 0 and act.tolist() == [0, 0, 0]
    assert rows.tobytes() == first.tobytes() and ok.tobytes() == first_ok.tobytes()
    assert between == alone and (tiled(), batch()) == alone


# ---- 9. lanes -----------------------------------------------------------------------------------------------------------------------------------------
def test_two_lanes_in_flight_and_a_camera_that_changes_lane(eng, cams):
    a0 = synthetic_frame(96, 64, 31)
    a1 = a0.copy()
    a1[:48, :30] = synthetic_frame(96, 64, 41)[:48, :30]
    b0 = synthetic_frame(128, 80, 34)
    rects2 = [(0, 0, 64, 48), (64, 32, 64, 48)]
    eng.set_camera_tiles(cams[0], 96, 64, RECTS, 8, 1, 0)
    eng.set_camera_tiles(cams[1], 128, 80, rects2, 8, 1, 0)
    ptr = {k: eng.upload(v) for k, v in (("a0", a0), ("a1", a1), ("b0", b0))}
    size = {"a0": (96, 64), "a1": (96, 64), "b0": (128, 80)}

    def submit(slot, name, cam):
        eng.submit_gated_device(slot, [ptr[name]], [size[name][0]], [size[name][1]], [cam], ios=IOS)
        return eng.gate_stats(slot)[0][0]

    def collect(slot):
        rows, ok = np.zeros((1, 100), ROW_DTYPE), np.full((1, 100), 9, np.uint8)
        eng.collect(slot, list(rows), list(ok))
        assert eng.slot_rows(slot, 1).tobytes() == rows.tobytes()
        return rows.tobytes(), ok.tobytes()

    try:
        want = []
        for name, cam in (("a0", cams[0]), ("b0", cams[1]), ("a1", cams[0])):
            ran = submit(0, name, cam)
            want.append((ran,) + collect(0))
        assert [w[0] for w in want] == [ALL, 0b11, 0b101]
        eng.reset_camera_tiles(cams[0])
        eng.reset_camera_tiles(cams[1])
        r0 = submit(0, "a0", cams[0])
        r1 = submit(1, "b0", cams[1])          # both in flight
        got = [(r0,) + collect(0), (r1,) + collect(1)]
        r2 = submit(1, "a1", cams[0])          # camera 0 moves to lane 1
        got.append((r2,) + collect(1))
        assert got == want
    finally:
        eng.sync()
        for p in ptr.values():
            eng.free(p)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_keep_the_state(eng, cams):
    frame = synthetic_frame(96, 64, 31)
    small = synthetic_frame(64, 48, 31)
    gray = np.zeros((64, 96), np.uint8)
    nan = float("nan")
    for c in cams:
        eng.set_camera_tiles(c, 96, 64, RECTS, 8, 1, 0)
    lib, h = eng._lib, eng._h
    first, _, ran, _ = gated(eng, frame, cams[0])
    assert ran == ALL
    bad = [   # (frames, cameras, formats, iou, ios, code)
        ([frame], [-1], None, 0.6, 1.0, _lib.WZ_EINVAL),
        ([frame], [77], None, 0.6, 1.0, _lib.WZ_EINVAL),                       # a camera without a layout
        ([frame], None, None, 0.6, 1.0, _lib.WZ_EINVAL),                       # no camera ids at all
        ([small], [cams[0]], None, 0.6, 1.0, _lib.WZ_EINVAL),                  # another size than the layout's
        ([gray], [cams[0]], [FMT_GRAY8], 0.6, 1.0, _lib.WZ_EINVAL),            # another base format
        ([frame, frame], [cams[0], cams[0]], None, 0.6, 1.0, _lib.WZ_EINVAL),  # the same camera twice
        ([frame] * 3, list(cams), None, 0.6, 1.0, _lib.WZ_ELIMIT),             # 9 configured tiles, max_batch 8
        ([frame], [cams[0]], None, nan, 1.0, _lib.WZ_EINVAL),
        ([frame], [cams[0]], None, 0.6, nan, _lib.WZ_EINVAL),
        ([frame], [cams[0]], None, -0.1, 1.0, _lib.WZ_EINVAL),
        ([frame], [cams[0]], None, 0.6, -1.0, _lib.WZ_EINVAL),
        ([], [], None, 0.6, 1.0, _lib.WZ_ELIMIT),
    ]
    for case, (frames, cam_ids, formats, iou, ios, code) in enumerate(bad):
        before = eng.gate_stats(0)
        n, m = len(frames), max(len(frames), 1)
        rows = np.full((m, 100 * ROW_DTYPE.itemsize), 0xA5, np.uint8)
        passes = np.full((m, 100), 0xA5, np.uint8)
        geo = [eng.frame_geometry(f, fm) for f, fm in zip(frames, formats or [FMT_RGB24] * n)]
        ws, hs = (C.c_int32 * m)(*[g[0] for g in geo]), (C.c_int32 * m)(*[g[1] for g in geo])
        fptr = (C.c_void_p * m)(*[f.ctypes.data for f in frames])
        fmtv = (C.c_int32 * m)(*formats) if formats else None
        camv = (C.c_int32 * m)(*cam_ids) if cam_ids is not None else None
        outs = (C.c_void_p * m)(*[r.ctypes.data for r in rows])
        pv = (C.c_void_p * m)(*[p.ctypes.data for p in passes])
        rc = lib.wz_detect_gated(h, n, fptr, ws, hs, fmtv, camv, iou, ios, outs, pv, None)
        assert rc == code, (cam_ids, formats, iou, ios, _lib.last_error(lib))
        refusal_golden.check("gated", "%d/wz_detect_gated" % case, rc, _lib.last_error(lib))
        assert (rows == 0xA5).all() and (passes == 0xA5).all()
        # the device entry point refuses the same way (host pointers stand in: a refused call reads no frame) and enqueues nothing
        rc = lib.wz_submit_gated_device(h, 0, n, fptr, ws, hs, fmtv, camv, iou, ios)
        assert rc == code, (cam_ids, formats, iou, ios, _lib.last_error(lib))
        refusal_golden.check("gated", "%d/wz_submit_gated_device" % case, rc, _lib.last_error(lib))
        after = eng.gate_stats(0)
        assert after[0] == before[0] and [a.tolist() for a in after[1]] == [b.tolist() for b in before[1]]
        rows, _, ran, act = gated(eng, frame, cams[0])                         # the state is intact: a still frame runs nothing
        assert ran == 0 and act.tolist() == [0, 0, 0] and rows.tobytes() == first.tobytes()
    # a layout the engine refuses leaves the camera with the one it had
    for case, (tiles, gate, width) in enumerate((([(0, 0, 200, 10)], (8, 1, 0), 96), (RECTS, (256, 1, 0), 96), (RECTS, (8, 0, 0), 96),
                                                 (RECTS, (8, 1, -1), 96), (RECTS * 3, (8, 1, 0), 96), ([(0, 0, 700, 10)], (8, 1, 0), 800))):
        with pytest.raises(ValueError):
            eng.set_camera_tiles(cams[0], width, 64, tiles, *gate)
        assert gated(eng, frame, cams[0])[2] == 0
        arr = (C.c_int32 * (4 * len(tiles)))(*[v for r in tiles for v in r])
        rc = lib.wz_set_camera_tiles(h, cams[0], width, 64, FMT_RGB24, len(tiles), arr, (C.c_int32 * 4)(*gate, 0))
        refusal_golden.check("gated", "layout/%d" % case, rc, _lib.last_error(lib))
        assert rc != 0 and gated(eng, frame, cams[0])[2] == 0


# ---- 11. plugin -------------------------------------------------------------------------------------------------------------------------------------------
def test_plugin_gate_option(model_dir_default):
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    from watsor_amd.share import DetectionArray
    frames = [synthetic_frame(96, 64, 31), synthetic_frame(96, 64, 32)]
    shapes = [f.shape for f in frames]
    options = {"tiles": {"rects": [list(r) for r in RECTS], "ios": IOS, "gate": {"threshold": 8}}, "numa": False}
    with HipObjectDetector(model_dir_default, 0, options, **SIZE) as det:
        want = [np.zeros(100, ROW_DTYPE), np.zeros(100, ROW_DTYPE)]
        det.engine.detect_tiled(frames, [RECTS, RECTS], want, ios=IOS)
        first = [DetectionArray(), DetectionArray()]
        det.detect_batch(shapes, frames, first, cameras=[0, 1])
        assert det.engine.gate_stats(0)[0] == [ALL, ALL]
        assert [bytes(r) for r in first] == [w.tobytes() for w in want] and (want[0]["confidence"] > 0).any()
        again = [DetectionArray(), DetectionArray()]
        det.detect_batch(shapes, frames, again, cameras=[0, 1])
        assert det.engine.gate_stats(0)[0] == [0, 0]
        assert [bytes(r) for r in again] == [w.tobytes() for w in want]
        # a frame without a camera id: the ungated tiled call, and the cameras' state is not touched
        rows, alone = DetectionArray(), np.zeros(100, ROW_DTYPE)
        det.detect(frames[1].shape, frames[1], rows)
        det.engine.detect_tiled([frames[1]], [RECTS], [alone], ios=IOS)      # (a batch of its own: three tiles, not six)
        assert bytes(rows) == alone.tobytes()
        det.detect_batch(shapes, frames, again, cameras=[0, 1])
        assert det.engine.gate_stats(0)[0] == [0, 0]
