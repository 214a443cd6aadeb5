"""Motion regions on the GPU, end to end (include/watsor_hip.h: wz_set_camera_motion / wz_detect_motion): the tile lists
against tests/motion_oracle.py, and the rows, byte for byte, against ONE `detect_tiled` call on the same frames with the reported lists."""
import ctypes as C

import numpy as np
import pytest

import motion_oracle as mo
import refusal_golden
import tile_oracle as to
from conftest import make_engine
from test_gpu_tiled import nv12_of
from watsor_amd import _lib
from watsor_amd.coco import COCO_CLASSES
from watsor_amd.filter.hip_filter import HipCameraFilter
from watsor_amd.runtime import FMT_GRAY8, FMT_NV12, FMT_RGB24, ROW_DTYPE
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

SIZE = dict(max_batch=8, max_width=640, max_height=480)
W, H = 640, 360
THR, IOS = 20, 0.6
SETTINGS = dict(min_cells=1, dilate=1, max_regions=3, min_side=128, pad=8)
PADDING = np.full(100, to.padding_row(), ROW_DTYPE)


@pytest.fixture(scope="module")
def eng(model_dir):
    e = make_engine(model_dir, **SIZE)
    yield e
    e.close()


@pytest.fixture
def cams(eng):
    """camera ids a test may give motion settings (and gate tiles); whatever it set is cleared behind it"""
    ids = [31, 32, 33]
    yield ids
    for c in ids:
        eng.clear_camera_motion(c)
        eng.clear_camera_tiles(c)


def scene(seed, at):
    """seeded noise with a bright 48 x 48 patch whose top-left corner is `at`"""
    f = np.random.default_rng(seed).integers(0, 48, (H, W, 3), dtype=np.uint8)
    f[at[1]:at[1] + 48, at[0]:at[0] + 48] = (250, 240, 230)
    return f


A, B = scene(7, (100, 60)), scene(7, (400, 200))
OTHER = scene(8, (300, 150))


def setup(eng, cam, whole, fmt=FMT_RGB24, **kw):
    p = dict(SETTINGS, **kw)
    eng.set_camera_motion(cam, W, H, THR, whole_frame=whole, fmt=fmt, **p)
    return mo.MotionState(W, H, fmt, THR, whole_frame=whole, **p)


def motion(eng, frames, cam_ids, fmt=None, iou=None):
    """(rows [n, 100], pass bytes [n, 100], tile lists, the regions' changed cells, components) of one motion call"""
    n = len(frames)
    rows, ok = np.zeros((n, 100), ROW_DTYPE), np.full((n, 100), 9, np.uint8)
    eng.detect_motion(frames, cam_ids, list(rows), passes=list(ok), formats=None if fmt is None else [fmt] * n, iou=iou, ios=IOS)
    return (rows, ok) + eng.motion_stats(0)


def tiled(eng, frames, lists, cam_ids=None, fmt=None, iou=None):
    """what the issue defines a motion call's result to be: one `detect_tiled` call of the frames that have a tile, padding rows and pass 0 for the
    others (which add no tile to the batch)"""
    n = len(frames)
    rows, ok = np.stack([PADDING] * n), np.zeros((n, 100), np.uint8)
    some = [i for i in range(n) if lists[i]]
    if some:
        r, k = np.zeros((len(some), 100), ROW_DTYPE), np.full((len(some), 100), 9, np.uint8)
        eng.detect_tiled([frames[i] for i in some], [lists[i] for i in some], list(r), cams=None if cam_ids is None else [cam_ids[i] for i in some],
                         passes=list(k), formats=None if fmt is None else [fmt] * len(some), iou=iou, ios=IOS)
        rows[some], ok[some] = r, k
    return rows, ok


def check_call(eng, states, frames, cam_ids, fmt=None):
    rows, ok, lists, cells, comps = motion(eng, frames, cam_ids, fmt)
    want = [s.step(f) for s, f in zip(states, frames)]
    assert lists == [w[0] for w in want] and cells == [w[1] for w in want] and comps == [w[2] for w in want]
    want_rows, want_ok = tiled(eng, frames, lists, cam_ids, fmt)
    assert rows.tobytes() == want_rows.tobytes() and ok.tobytes() == want_ok.tobytes()
    return rows, ok, lists


# ---- 1. frame A, the patch moved, the same frame again -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rgb", "nv12"])
@pytest.mark.parametrize("whole", [True, False])
def test_three_calls(eng, cams, whole, kind):
    a, b, fmt = (A, B, None) if kind == "rgb" else (nv12_of(A), nv12_of(B), FMT_NV12)
    state = setup(eng, cams[0], whole, fmt or FMT_RGB24)
    first = [(0, 0, W, H)] if whole else []
    rows, ok, lists = check_call(eng, [state], [a], [cams[0]], fmt)
    assert lists == [first]                                   # no reference: nothing has changed
    if not whole:
        assert rows[0].tobytes() == PADDING.tobytes() and not ok.any()
    rows, ok, lists = check_call(eng, [state], [b], [cams[0]], fmt)
    regions = lists[0][len(first):]
    assert len(regions) == 2 and all(r[2] == 128 and r[3] == 128 for r in regions)        # where the patch was and where it is
    assert any(x <= 400 and y <= 200 and x + w >= 448 and y + h >= 248 for x, y, w, h in regions)
    assert any(x <= 100 and y <= 60 and x + w >= 148 and y + h >= 108 for x, y, w, h in regions)
    assert (rows[0]["confidence"] > 0).any()
    rows, ok, lists = check_call(eng, [state], [b], [cams[0]], fmt)
    assert lists == [first]                                   # a still picture
    if not whole:
        assert rows[0].tobytes() == PADDING.tobytes() and not ok.any()


# ---- 2. two cameras, one moves -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole", [True, False])
def test_two_cameras_one_moves(eng, cams, whole):
    states = [setup(eng, cams[0], whole), setup(eng, cams[1], whole)]
    check_call(eng, states, [A, OTHER], cams[:2])
    rows, ok, lists = check_call(eng, states, [B, OTHER], cams[:2])
    assert len(lists[0]) == 2 + whole and len(lists[1]) == 0 + whole
    rows, ok, lists = check_call(eng, states[::-1], [OTHER, A], cams[1::-1])       # the other order; camera 0 moves back
    assert len(lists[1]) == 2 + whole and len(lists[0]) == 0 + whole


# ---- 3. reset, new settings -----------------------------------------------------------------------------------------------------------------------
def test_reset_and_new_settings(eng, cams):
    state = setup(eng, cams[0], False)
    check_call(eng, [state], [A], [cams[0]])
    eng.reset_camera_motion(cams[0])
    state.reset()
    assert check_call(eng, [state], [B], [cams[0]])[2] == [[]]                     # the reference is forgotten: B is the first picture
    assert len(check_call(eng, [state], [A], [cams[0]])[2][0]) == 2
    state = setup(eng, cams[0], False, max_regions=1, min_side=200, dilate=2)     # settings made anew start without a reference
    assert check_call(eng, [state], [B], [cams[0]])[2] == [[]]
    lists = check_call(eng, [state], [A], [cams[0]])[2]
    assert len(lists[0]) == 1 and lists[0][0][2:] == (200, 200)
    with pytest.raises(ValueError):
        eng.reset_camera_motion(cams[2])


# ---- 4. the camera filter ---------------------------------------------------------------------------------------------------------------------------
def test_camera_filter_runs_on_the_merged_rows(eng, cams):
    cam = cams[0]
    cfg = {"width": W, "height": H, "detect": [{name: {"area": 0, "confidence": 100, "zones": []}} for name in COCO_CLASSES[1:]]}      # nothing is that confident: every row fails and is zeroed
    state = setup(eng, cam, False)
    flt = HipCameraFilter(eng, cam, cfg, drop=True)
    try:
        rows, ok, lists = check_call(eng, [state], [A], [cam])
        assert lists == [[]] and rows[0].tobytes() == PADDING.tobytes() and not ok.any()      # no tile: padding rows whatever the filter says
        rows, ok, lists = check_call(eng, [state], [B], [cam])
        want, plain_ok = tiled(eng, [B], lists)                                               # the same tiles without the camera ...
        want_ok = eng.filter_rows(cam, want[0])                                               # ... then the filter, in place (drop mode)
        assert rows[0].tobytes() == want[0].tobytes()
        np.testing.assert_array_equal(ok[0], want_ok)
        assert not np.array_equal(want_ok, plain_ok[0])                                       # (precondition: the filter says something)
    finally:
        flt.close()


# ---- 5. neighbours --------------------------------------------------------------------------------------------------------------------------------------
def test_gated_and_untiled_calls_between_two_motion_calls(eng, cams):
    small, rects = synthetic_frame(96, 64, 31), [(0, 0, 64, 48), (31, 15, 65, 49), (0, 0, 96, 64)]

    def gated():
        rows = np.zeros(100, ROW_DTYPE)
        eng.detect_gated([small], [cams[0]], [rows], ios=IOS)
        return rows.tobytes(), eng.gate_stats(0)[0]

    def batch():
        rows = np.zeros((2, 100), ROW_DTYPE)
        eng.detect_batch([small, A], list(rows))
        return rows.tobytes()

    eng.set_camera_tiles(cams[0], 96, 64, rects, 8, 1, 0)
    first, alone = gated(), batch()
    assert first[1] == [0b111]
    state = setup(eng, cams[0], True)                          # the camera has gate tiles AND motion settings: two states
    check_call(eng, [state], [A], [cams[0]])
    still = gated()
    assert still == (first[0], [0]) and batch() == alone       # the gate kept its reference through the motion call
    lists = check_call(eng, [state], [B], [cams[0]])[2]
    assert len(lists[0]) == 3                                  # ... and the motion reference survived the gated call and the batch
    assert gated() == (first[0], [0]) and batch() == alone


# ---- 6. lanes -------------------------------------------------------------------------------------------------------------------------------------------
def test_device_frames_on_another_lane(eng, cams):
    state = setup(eng, cams[0], True)
    ptr = {"a": eng.upload(A), "b": eng.upload(B)}
    try:
        for slot, name, frame in ((1, "a", A), (0, "b", B), (1, "b", B)):
            eng.submit_motion_device(slot, [ptr[name]], [W], [H], [cams[0]], ios=IOS)
            lists, cells, comps = eng.motion_stats(slot)
            assert (lists[0], cells[0], comps[0]) == state.step(frame)
            rows, ok = np.zeros((1, 100), ROW_DTYPE), np.full((1, 100), 9, np.uint8)
            eng.collect(slot, list(rows), list(ok))
            want, want_ok = tiled(eng, [frame], lists, [cams[0]])
            assert rows.tobytes() == want.tobytes() and ok.tobytes() == want_ok.tobytes()
    finally:
        eng.sync()
        for p in ptr.values():
            eng.free(p)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_keep_the_state(eng, cams):
    small, gray, nan = synthetic_frame(96, 64, 31), np.zeros((H, W), np.uint8), float("nan")
    states = [setup(eng, c, True) for c in cams]                # 3 x (1 + 3) = 12 configured tiles: more than max_batch together
    lib, h = eng._lib, eng._h
    check_call(eng, states[:1], [A], cams[:1])
    bad = [   # (frames, cameras, formats, iou, ios, code)
        ([A], [-1], None, 0.6, 1.0, _lib.WZ_EINVAL),
        ([A], [77], None, 0.6, 1.0, _lib.WZ_EINVAL),                           # a camera without settings
        ([A], None, None, 0.6, 1.0, _lib.WZ_EINVAL),                           # no camera ids at all
        ([small], [cams[0]], None, 0.6, 1.0, _lib.WZ_EINVAL),                  # another size than the settings'
        ([gray], [cams[0]], [FMT_GRAY8], 0.6, 1.0, _lib.WZ_EINVAL),            # another base format
        ([A, B], [cams[0], cams[0]], None, 0.6, 1.0, _lib.WZ_EINVAL),          # the same camera twice
        ([A, A, A], list(cams), None, 0.6, 1.0, _lib.WZ_ELIMIT),               # configured tiles beyond max_batch, whatever moved
        ([A], [cams[0]], None, nan, 1.0, _lib.WZ_EINVAL),
        ([A], [cams[0]], None, 0.6, nan, _lib.WZ_EINVAL),
        ([A], [cams[0]], None, -0.1, 1.0, _lib.WZ_EINVAL),
        ([A], [cams[0]], None, 0.6, -1.0, _lib.WZ_EINVAL),
        ([], [], None, 0.6, 1.0, _lib.WZ_ELIMIT),
    ]
    for case, (frames, cam_ids, formats, iou, ios, code) in enumerate(bad):
        before = eng.motion_stats(0)
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
        rc = lib.wz_detect_motion(h, n, fptr, ws, hs, fmtv, camv, iou, ios, outs, pv, None)
        assert rc == code and _lib.last_error(lib), (cam_ids, formats, iou, ios, _lib.last_error(lib))
        refusal_golden.check("motion", "%d/wz_detect_motion" % case, rc, _lib.last_error(lib))
        assert (rows == 0xA5).all() and (passes == 0xA5).all()
        # the device entry point refuses the same way (host pointers stand in: a refused call reads no frame) and enqueues nothing
        rc = lib.wz_submit_motion_device(h, 0, n, fptr, ws, hs, fmtv, camv, iou, ios)
        assert rc == code, (cam_ids, formats, iou, ios, _lib.last_error(lib))
        refusal_golden.check("motion", "%d/wz_submit_motion_device" % case, rc, _lib.last_error(lib))
        assert eng.motion_stats(0) == before
    # the reference is intact: it is still A's
    assert len(check_call(eng, states[:1], [B], cams[:1])[2][0]) == 3
    # settings the engine refuses leave the camera with the ones it had
    ok = dict(threshold=THR, min_cells=1, dilate=1, max_regions=3, min_side=128, pad=8, whole_frame=True)
    for case, (change, width, code) in enumerate(((dict(threshold=256), W, _lib.WZ_EINVAL), (dict(threshold=-1), W, _lib.WZ_EINVAL), (dict(min_cells=0), W, _lib.WZ_EINVAL),
                                (dict(dilate=3), W, _lib.WZ_EINVAL), (dict(dilate=-1), W, _lib.WZ_EINVAL), (dict(max_regions=0), W, _lib.WZ_EINVAL),
                                (dict(max_regions=17), W, _lib.WZ_EINVAL), (dict(min_side=15), W, _lib.WZ_EINVAL), (dict(pad=65), W, _lib.WZ_EINVAL),
                                (dict(pad=-1), W, _lib.WZ_EINVAL), (dict(whole_frame=2), W, _lib.WZ_EINVAL), ({}, 0, _lib.WZ_EINVAL),
                                ({}, 656, _lib.WZ_ELIMIT), (dict(max_regions=8), W, _lib.WZ_ELIMIT))):
        p = dict(ok, **change)
        words = (C.c_int32 * 8)(p["threshold"], p["min_cells"], p["dilate"], p["max_regions"], p["min_side"], p["pad"], p["whole_frame"], 0)
        rc = lib.wz_set_camera_motion(h, cams[0], width, H, FMT_RGB24, C.byref(words))
        assert rc == code and _lib.last_error(lib), (change, width, _lib.last_error(lib))
        refusal_golden.check("motion", "settings/%d" % case, rc, _lib.last_error(lib))
    rc = lib.wz_set_camera_motion(h, cams[0], W, H, FMT_NV12 | 0x400, C.byref(words))                         # a format word the engine does not take
    refusal_golden.check("motion", "settings/format", rc, _lib.last_error(lib))
    assert rc == _lib.WZ_EINVAL
    rc = lib.wz_set_camera_motion(h, 256, W, H, FMT_RGB24, C.byref(words))
    refusal_golden.check("motion", "settings/camera", rc, _lib.last_error(lib))
    assert rc == _lib.WZ_ELIMIT
    assert len(check_call(eng, states[:1], [A], cams[:1])[2][0]) == 3          # still B's reference, still the old settings
    eng.clear_camera_motion(cams[0])
    with pytest.raises(ValueError, match="no motion settings"):
        motion(eng, [A], cams[:1])


# ---- 8. plugin --------------------------------------------------------------------------------------------------------------------------------------------
def test_plugin_motion_option(model_dir_default):
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    from watsor_amd.share import DetectionArray
    opt = {"threshold": THR, "min_side": 128, "ios": IOS}
    with HipObjectDetector(model_dir_default, 0, {"motion": opt, "numa": False}, **SIZE) as det:
        states = [mo.MotionState(W, H, FMT_RGB24, THR, **dict(SETTINGS)) for _ in range(3)]
        for frames in ([A, OTHER, A], [B, OTHER, B]):
            rows = [DetectionArray() for _ in frames]
            det.detect_batch([f.shape for f in frames], frames, rows, cameras=[0, 1, 2])      # 3 x (1 + 3) configured tiles: two calls
            lists = det.engine.motion_stats(0)[0]
            assert lists == [states[2].step(frames[2])[0]]                                    # (the last call held camera 2 alone)
            want = [s.step(f)[0] for s, f in zip(states[:2], frames[:2])] + lists
            for i, f in enumerate(frames):
                alone = np.zeros(100, ROW_DTYPE)
                if i < 2:                                                                     # cameras 0 and 1 shared a call: one batch of their tiles
                    pair = np.zeros((2, 100), ROW_DTYPE)
                    det.engine.detect_tiled(frames[:2], want[:2], list(pair), ios=IOS)
                    alone = pair[i]
                else:
                    det.engine.detect_tiled([f], [want[i]], [alone], ios=IOS)
                assert bytes(rows[i]) == alone.tobytes()
        assert len(want[0]) == 3 and len(want[1]) == 1
        with pytest.raises(ValueError, match="camera id"):
            det.detect(A.shape, A, DetectionArray())
        with pytest.raises(ValueError, match="motion configured"):
            det.bind_frame_table({"porch": type("FB", (), {"frames": []})()}, {"porch": 0})
    with pytest.raises(ValueError, match="^motion: .*tiles"):
        HipObjectDetector(model_dir_default, 0, {"motion": opt, "tiles": {"grid": [2, 1]}, "numa": False}, **SIZE)
