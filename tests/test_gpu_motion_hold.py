"""The motion hold on the GPU, end to end (include/watsor_hip.h: wz_set_camera_motion_hold), on both `-p 16` programs:
per call the tile lists, stats and ages against tests/motion_hold_oracle.py -- which is fed the rows and pass bytes the call returned --
and the rows, byte for byte, against ONE `detect_tiled` call on the reported lists.  Frames and sizes are test_gpu_motion.py's."""
import ctypes as C

import numpy as np
import pytest

import motion_hold_oracle as ho
import motion_oracle as mo
from conftest import make_engine
from test_gpu_motion import A, B, H, IOS, OTHER, PADDING, SETTINGS, SIZE, THR, W, scene, tiled
from test_gpu_tiled import nv12_of
from watsor_amd import _lib
from watsor_amd.coco import COCO_CLASSES
from watsor_amd.filter.hip_filter import HipCameraFilter
from watsor_amd.runtime import FMT_NV12, FMT_RGB24, ROW_DTYPE

pytestmark = pytest.mark.gpu

WHOLE = (0, 0, W, H)
OTHER_MOVED = scene(8, (40, 250))


@pytest.fixture(scope="module")
def eng(model_dir):
    e = make_engine(model_dir, dev=True, **SIZE)       # (the development library, for wz_debug_motion_age: the same kernels)
    yield e
    e.close()


@pytest.fixture
def cams(eng):
    ids = [41, 42, 43]
    yield ids
    for c in ids:
        eng.clear_camera_motion(c)


def setup(eng, cam, whole, hold, object_hold, fmt=FMT_RGB24, **kw):
    """motion settings, then -- unless both are 0 -- the hold; the oracle's state of such a camera"""
    p = dict(SETTINGS, **kw)
    eng.set_camera_motion(cam, W, H, THR, whole_frame=whole, fmt=fmt, **p)
    if not (hold or object_hold):
        return mo.MotionState(W, H, fmt, THR, whole_frame=whole, **p)
    eng.set_camera_motion_hold(cam, hold, object_hold)
    return ho.HoldState(W, H, fmt, THR, hold, object_hold, whole_frame=whole, **p)


def expect(state, frame):
    """(tile list, n, components, active, held) of the camera's next call"""
    return state.begin(frame) if isinstance(state, ho.HoldState) else state.step(frame) + (0, 0)


def settle(eng, states, cam_ids, rows, ok):
    """what an accepted call leaves: the oracle stamps the rows the call returned; the engine's ages are the oracle's"""
    for i, s in enumerate(states):
        if isinstance(s, ho.HoldState):
            s.finish(rows[i], ok[i])
            np.testing.assert_array_equal(eng.debug_motion_age(cam_ids[i]), s.G)


def check_call(eng, states, frames, cam_ids, fmt=None):
    n = len(frames)
    rows, ok = np.zeros((n, 100), ROW_DTYPE), np.full((n, 100), 9, np.uint8)
    eng.detect_motion(frames, cam_ids, list(rows), passes=list(ok), formats=None if fmt is None else [fmt] * n, ios=IOS)
    lists, cells, comps = eng.motion_stats(0)
    active, held = eng.motion_hold_stats(0)
    want = [expect(s, f) for s, f in zip(states, frames)]
    assert [(lists[i], cells[i], comps[i], active[i], held[i]) for i in range(n)] == want
    want_rows, want_ok = tiled(eng, frames, lists, cam_ids, fmt)
    assert rows.tobytes() == want_rows.tobytes() and ok.tobytes() == want_ok.tobytes()
    settle(eng, states, cam_ids, rows, ok)
    return rows, ok, lists


# ---- 1. hold: frame A, the patch moved, then the same frame four more times ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rgb", "nv12"])
def test_hold_keeps_the_regions_for_two_further_calls(eng, cams, kind):
    a, b, fmt = (A, B, None) if kind == "rgb" else (nv12_of(A), nv12_of(B), FMT_NV12)
    state = setup(eng, cams[0], False, 2, 0, fmt or FMT_RGB24)
    seen = []
    for k, f in enumerate([a, b, b, b, b, b]):
        rows, ok, lists = check_call(eng, [state], [f], [cams[0]], fmt)
        seen.append(lists[0])
        if not lists[0]:
            assert rows[0].tobytes() == PADDING.tobytes() and not ok.any()
    assert seen[0] == [] and len(seen[1]) == 2 and seen[2] == seen[1] and seen[3] == seen[1]      # changed at call 1, held at 2 and 3
    assert seen[4] == [] and seen[5] == []                                                     # the hold has run out: padding rows
    assert not state.G.any()


# ---- 2. object_hold: a still picture from the first call on ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rgb", "nv12"])
def test_object_hold_follows_the_detections_of_a_still_picture(eng, cams, kind):
    a, fmt = (A, None) if kind == "rgb" else (nv12_of(A), FMT_NV12)
    state = setup(eng, cams[0], True, 0, 3, fmt or FMT_RGB24)
    passed, regions = 0, []
    for k in range(4):
        rows, ok, lists = check_call(eng, [state], [a], [cams[0]], fmt)       # (the regions equal the oracle's, fed the previous rows)
        assert lists[0][0] == WHOLE
        passed += int((ok[0] == 1).sum())
        regions.append(lists[0][1:])
    assert passed > 0, "no row of the still picture passed: the sequence says nothing about the stamp"
    assert regions[0] == [] and regions[1] != []                             # nothing moved, ever: the regions are the detections'
    assert (state.G.max() == 3) == bool((ok[0] == 1).any())


def test_a_filter_that_rejects_everything_stamps_nothing(eng, cams):
    cam = cams[0]
    cfg = {"width": W, "height": H, "detect": [{name: {"area": 0, "confidence": 100, "zones": []}} for name in COCO_CLASSES[1:]]}
    state = setup(eng, cam, True, 0, 3)
    flt = HipCameraFilter(eng, cam, cfg, drop=True)
    try:
        for k in range(3):
            rows, ok, lists = check_call(eng, [state], [A], [cam])
            assert lists == [[WHOLE]] and not ok.any() and not state.G.any()
    finally:
        flt.close()


# ---- 3. two cameras in one call, one with a hold ---------------------------------------------------------------------------------------------
def test_a_camera_without_a_hold_beside_one_with(eng, cams, model_dir_default):
    states = [setup(eng, cams[0], False, 2, 0), setup(eng, cams[1], False, 0, 0)]
    sequence = [(A, OTHER), (B, OTHER_MOVED), (B, OTHER_MOVED), (B, OTHER), (B, OTHER)]
    got = []
    for fa, fb in sequence:
        lists = check_call(eng, states, [fa, fb], cams[:2])[2]
        got.append((lists[1], eng.motion_stats(0)[1][1], eng.motion_stats(0)[2][1]))
        assert (eng.motion_hold_stats(0)[0][1], eng.motion_hold_stats(0)[1][1]) == (0, 0)
    assert len(got[1][0]) == 2 and got[2][0] == [] and len(got[3][0]) == 2
    plain = make_engine(model_dir_default, **SIZE)          # an engine that never set a hold: the same camera, the same frames
    try:
        plain.set_camera_motion(7, W, H, THR, whole_frame=False, **SETTINGS)
        for (_, fb), want in zip(sequence, got):
            plain.detect_motion([fb], [7], [np.zeros(100, ROW_DTYPE)], ios=IOS)
            lists, cells, comps = plain.motion_stats(0)
            assert (lists[0], cells[0], comps[0]) == want and plain.motion_hold_stats(0) == ([0], [0])
    finally:
        plain.close()


# ---- 4. reset, new motion settings, a hold of (0, 0) -----------------------------------------------------------------------------------------
def test_reset_new_settings_and_removal(eng, cams):
    cam = cams[0]
    state = setup(eng, cam, False, 3, 0)
    check_call(eng, [state], [A], [cam])
    assert len(check_call(eng, [state], [B], [cam])[2][0]) == 2 and state.G.max() == 3
    eng.reset_camera_motion(cam)
    state.reset()
    assert not eng.debug_motion_age(cam).any()                                # the ages are zero, the reference is gone
    assert check_call(eng, [state], [B], [cam])[2] == [[]]
    assert len(check_call(eng, [state], [A], [cam])[2][0]) == 2
    assert len(check_call(eng, [state], [A], [cam])[2][0]) == 2               # held
    eng.set_camera_motion_hold(cam, 1, 0)                                     # a new hold starts from zero ages, the reference stays
    state.hold, state.G = 1, np.zeros_like(state.G)
    assert check_call(eng, [state], [A], [cam])[2] == [[]]
    eng.set_camera_motion_hold(cam, 0, 0)                                     # (0, 0) removes the hold and frees its grids
    with pytest.raises(ValueError, match="no motion hold"):
        eng.debug_motion_age(cam)
    eng.detect_motion([B], [cam], [np.zeros(100, ROW_DTYPE)], ios=IOS)
    assert len(eng.motion_stats(0)[0][0]) == 2 and eng.motion_hold_stats(0) == ([0], [0])
    eng.set_camera_motion_hold(cam, 2, 0)
    assert not eng.debug_motion_age(cam).any()
    eng.set_camera_motion(cam, W, H, THR, whole_frame=False, **SETTINGS)      # new motion settings drop the hold
    with pytest.raises(ValueError, match="no motion hold"):
        eng.debug_motion_age(cam)
    plain = mo.MotionState(W, H, FMT_RGB24, THR, whole_frame=False, **SETTINGS)
    for f in (A, B, B):
        check_call(eng, [plain], [f], [cam])


# ---- 5. lanes: the stamp launch of one call is in flight when the next call of the camera starts on another lane ------------------------------
def test_the_next_call_on_another_lane_waits_for_the_stamp(eng, cams):
    cam = cams[0]
    state = setup(eng, cam, True, 2, 3)
    ptr = {"a": eng.upload(A), "b": eng.upload(B)}
    frames = {"a": A, "b": B}
    try:
        for first, second in (("a", "b"), ("b", "b"), ("a", "a")):
            eng.submit_motion_device(0, [ptr[first]], [W], [H], [cam], ios=IOS)
            eng.submit_motion_device(1, [ptr[second]], [W], [H], [cam], ios=IOS)          # (nothing collected in between)
            for slot, name in ((0, first), (1, second)):
                lists, cells, comps = eng.motion_stats(slot)
                active, held = eng.motion_hold_stats(slot)
                assert (lists[0], cells[0], comps[0], active[0], held[0]) == state.begin(frames[name])
                rows, ok = np.zeros((1, 100), ROW_DTYPE), np.full((1, 100), 9, np.uint8)
                eng.collect(slot, list(rows), list(ok))
                want, want_ok = tiled(eng, [frames[name]], lists, [cam])
                assert rows.tobytes() == want.tobytes() and ok.tobytes() == want_ok.tobytes()
                state.finish(rows[0], ok[0])
            np.testing.assert_array_equal(eng.debug_motion_age(cam), state.G)
    finally:
        eng.sync()
        for p in ptr.values():
            eng.free(p)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_the_ages_and_the_setter_refuses(eng, cams):
    cam = cams[0]
    state = setup(eng, cam, True, 2, 3)
    check_call(eng, [state], [A], [cam])
    check_call(eng, [state], [B], [cam])
    before = eng.debug_motion_age(cam)
    assert before.any()
    for frames, ids in (([A[:64, :96].copy()], [cam]), ([B], [77]), ([A, B], [cam, cam])):      # another size; no settings; the camera twice
        with pytest.raises(ValueError):
            eng.detect_motion(frames, ids, [np.zeros(100, ROW_DTYPE) for _ in frames], ios=IOS)
        np.testing.assert_array_equal(eng.debug_motion_age(cam), before)
    lib, h = eng._lib, eng._h
    words = lambda a, b: (C.c_int32 * 4)(a, b, 0, 0)      # noqa: E731
    for args in ((h, cam, None), (None, cam, C.byref(words(1, 1))), (h, 77, C.byref(words(1, 1))), (h, -1, C.byref(words(1, 1))),
                 (h, cam, C.byref(words(-1, 1))), (h, cam, C.byref(words(256, 1))), (h, cam, C.byref(words(1, -1))), (h, cam, C.byref(words(1, 256)))):
        assert lib.wz_set_camera_motion_hold(*args) == _lib.WZ_EINVAL and _lib.last_error(lib)
    a, b = (C.c_int32 * 1)(), (C.c_int32 * 1)()
    for args in ((h, 0, 1, None, C.byref(b)), (h, 0, 1, C.byref(a), None), (None, 0, 1, C.byref(a), C.byref(b)), (h, 0, 2, C.byref(a), C.byref(b)),
                 (h, 99, 1, C.byref(a), C.byref(b))):
        assert lib.wz_motion_hold_stats(*args) == _lib.WZ_EINVAL
    np.testing.assert_array_equal(eng.debug_motion_age(cam), before)      # the refused setters left the hold as it was
    check_call(eng, [state], [B], [cam])


# ---- 7. plugin ---------------------------------------------------------------------------------------------------------------------------------------
def test_plugin_motion_hold_option(model_dir_default):
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    from watsor_amd.share import DetectionArray
    opt = {"threshold": THR, "min_side": 128, "ios": IOS, "whole_frame": False}
    with HipObjectDetector(model_dir_default, 0, {"motion": opt, "motion_hold": {"hold": 2}, "numa": False}, **SIZE) as det:
        state = ho.HoldState(W, H, FMT_RGB24, THR, 2, 0, whole_frame=False, **dict(SETTINGS))
        seen = []
        for f in (A, B, B, B, B):
            rows = DetectionArray()
            det.detect_batch([f.shape], [f], [rows], cameras=[0])
            lists, cells, comps = det.engine.motion_stats(0)
            active, held = det.engine.motion_hold_stats(0)
            assert (lists[0], cells[0], comps[0], active[0], held[0]) == state.begin(f)
            state.finish(np.zeros(100, ROW_DTYPE), np.zeros(100, np.uint8))                   # (object_hold 0: the rows do not matter)
            seen.append(len(lists[0]))
        assert seen == [0, 2, 2, 2, 0]
    with pytest.raises(ValueError, match="^motion_hold: .*no motion option"):
        HipObjectDetector(model_dir_default, 0, {"motion_hold": {"hold": 2}, "numa": False}, **SIZE)
