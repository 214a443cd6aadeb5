"""Motion regions through the worker's frame table on the GPU (include/watsor_hip.h: wz_bind_motion / wz_submit_bound / wz_collect_bound;
DESIGN.md section 17b).  The yardstick is never the code under test: camera 0 goes through `detect_motion`, call by call -- a path pinned to
tests/motion_oracle.py by test_gpu_motion.py --, camera 1, with identical settings, through the table on the SAME engine with the same frame
sequence; after every step the rows, `motion_stats` (tile lists, cells, components), `motion_hold_stats` and `motion_ignore_stats` are
compared byte for byte.  The sequence is test_gpu_bound_tiles.py's `moved_patch_sequence` -- [a, a, b, b] -- with threshold 8, max_regions 2,
min_side 64, pad 8: by tests/motion_oracle.py its tile lists are [], [], [one region], [] with whole_frame 0, and gain the whole frame in
front with whole_frame 1.  Every sequence test asserts those shapes from the oracle and a row with confidence > 0."""
import ctypes as C
import itertools

import numpy as np
import pytest

import conftest
import motion_oracle as mo
import tile_oracle as to
from pixfmt_oracle import frame_from_rgb
from test_gpu_bound_tiles import GRID, IOS, NV12_HD, ROI, Table, drive_worker, moved_patch_sequence, raw_submit, tiled_rows
from watsor_amd import _lib
from watsor_amd.runtime import FMT_NV12, FMT_RGB24, ROW_DTYPE
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

SIZE = dict(max_batch=8, max_width=640, max_height=480)
W, H = 320, 240
THR = 8
P = dict(min_cells=1, dilate=1, max_regions=2, min_side=64, pad=8)
PADDING = np.full(100, to.padding_row(), ROW_DTYPE)
WHOLE = (0, 0, W, H)


@pytest.fixture(scope="module")
def eng(model_dir_default):
    e = conftest.make_engine(model_dir_default, dev=True, **SIZE)      # (the development library, for bound_source and wz_debug_motion_age: the same kernels)
    yield e
    e.close()


@pytest.fixture
def cams(eng):
    """whatever a test gave the cameras 0 .. 15 is cleared behind it"""
    yield list(range(16))
    eng.sync()
    for c in range(16):
        eng.clear_camera_motion(c)
        eng.clear_camera_tiles(c)


def set_cam(e, cam, whole, fmt=FMT_RGB24, w=W, h=H, hold=None, mask=None):
    """motion settings, then the hold, then the mask: the order the plugin uses"""
    e.set_camera_motion(cam, w, h, THR, whole_frame=whole, fmt=fmt, **P)
    if hold is not None:
        e.set_camera_motion_hold(cam, *hold)
    if mask is not None:
        e.set_camera_ignore(cam, mask)


def stats(e, lane):
    return e.motion_stats(lane), e.motion_hold_stats(lane), e.motion_ignore_stats(lane)


def gate(e, lane):
    ran, act = e.gate_stats(lane)
    return ran, [a.tolist() for a in act]


def by_call(e, cam_ids, frames, fmts=None):
    """(rows [n, 100], stats) of ONE detect_motion call (lane 0): the yardstick"""
    rows = np.zeros((len(frames), 100), ROW_DTYPE)
    e.detect_motion(list(frames), list(cam_ids), list(rows), formats=fmts, ios=IOS)
    return rows, stats(e, 0)


def oracle_lists(frames, whole, fmt=FMT_RGB24, w=W, h=H):
    s = mo.MotionState(w, h, fmt, THR, whole_frame=whole, **P)
    return [s.step(f)[0] for f in frames]


def assert_shapes(lists, whole):
    """[], [], [one region], [] -- with the whole frame in front of each when whole_frame is set"""
    first = [WHOLE] if whole else []
    assert [l[:len(first)] for l in lists] == [first] * 4 and [len(l) - len(first) for l in lists] == [0, 0, 1, 0], lists


def raw_bind_motion(e, first, count, iou, ios, handle=True):
    rc = e._lib.wz_bind_motion(e._h if handle else None, first, count, iou, ios)
    return rc, _lib.last_error(e._lib)


# ---- 1. one camera, step by step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("register", [True, False])
@pytest.mark.parametrize("whole", [1, 0])
@pytest.mark.parametrize("kind", ["rgb24", "nv12"])
def test_a_bound_motion_camera_equals_detect_motion(eng, cams, kind, whole, register):
    fmt, lead = (FMT_RGB24, 3) if kind == "rgb24" else (NV12_HD, 8)
    frames = [frame_from_rgb(f, fmt) for f in moved_patch_sequence(65)]
    assert_shapes(oracle_lists(frames, whole, fmt), whole)
    for cam in (0, 1):
        set_cam(eng, cam, whole, fmt)
    t = Table(eng, [frames[0]], [fmt], cams=[1], lead=lead, register=register)
    try:
        assert kind != "rgb24" or t.views[0].ctypes.data % 2 == 1
        eng.bind_motion(0, 1, ios=IOS)
        lists, seen = [], False
        for step, f in enumerate(frames):
            want, want_stats = by_call(eng, [0], [f], [fmt])
            t.views[0][...] = f
            t.rows.view(np.uint8)[...] = 0xA5
            got = t.run(1, [0])[0]                                       # (a still step with whole_frame 0: no batch ran, WZ_OK and the padding rows all the same)
            assert eng.bound_source(1) == [0], step                      # always staged, registered or not
            assert stats(eng, 1) == want_stats, step
            assert got.tobytes() == want[0].tobytes(), step
            lists.append(want_stats[0][0][0])
            seen = seen or bool((got["confidence"] > 0).any())
            if not lists[-1]:
                assert got.tobytes() == PADDING.tobytes(), step
        assert lists == oracle_lists(frames, whole, fmt) and seen
    finally:
        t.close()


# ---- 2. two cameras of different size and format in one submit ----------------------------------------------------------------------------
def small_sequence(seed, w=160, h=96):
    a = synthetic_frame(w, h, seed)
    b = a.copy()
    b[40:64, 72:96] = a[24:48, 40:64]
    b[24:48, 40:64] = synthetic_frame(w, h, seed + 1)[24:48, 40:64]
    return [frame_from_rgb(f, FMT_NV12) for f in (a, a, b, b)]


def test_two_motion_cameras_of_different_size_and_format_in_one_submit(eng, cams):
    from watsor_amd.coco import COCO_CLASSES
    from watsor_amd.filter.hip_filter import HipCameraFilter
    big, small = moved_patch_sequence(66), small_sequence(77)
    assert_shapes(oracle_lists(big, 1), 1)
    assert [len(l) for l in oracle_lists(small, 1, FMT_NV12, 160, 96)] == [1, 1, 2, 1]
    alpha = np.zeros((H, W), np.uint8)
    alpha[:, :200] = 255
    cfg = {"width": W, "height": H, "detect": [{name: {"area": 1, "confidence": 20, "zones": []}} for name in dict.fromkeys(COCO_CLASSES[1:])]}
    filters = [HipCameraFilter(eng, cam, cfg, alpha=alpha, drop=True) for cam in (0, 2)]      # the same zone mask, drop mode, on the yardstick's camera and the table's
    for cam in (0, 2):
        set_cam(eng, cam, 1)
    for cam in (1, 3):
        set_cam(eng, cam, 1, FMT_NV12, 160, 96)
    fmts = [FMT_RGB24, FMT_NV12]
    t = Table(eng, [big[0], small[0]], fmts, cams=[2, 3], lead=8)
    try:
        eng.bind_motion(0, 1, ios=IOS)
        eng.bind_motion(1, 1, ios=IOS)
        dropped = seen = False
        for step in range(4):
            want, want_stats = by_call(eng, [0, 1], [big[step], small[step]], fmts)
            t.views[0][...], t.views[1][...] = big[step], small[step]
            got = t.run(3, [0, 1])
            assert eng.bound_source(3) == [0, 0]
            assert stats(eng, 3) == want_stats, step
            assert got.tobytes() == want.tobytes(), step
            assert (got[1]["confidence"] > 0).any(), step
            seen = seen or bool((got[0]["confidence"] > 0).any())
            dropped = dropped or bool((got[0]["label"] == 0).any())
        assert dropped and seen                                          # the drop-mode filter ran on the merged rows of its camera, and let some through
    finally:
        t.close()
        for f in filters:
            f.close()


# ---- 3. four consecutive frames of one camera on four lanes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", [None, (2, 3)])
def test_a_motion_camera_over_four_lanes_equals_the_one_lane_sequence(eng, cams, hold):
    """with a hold and an object_hold every call leaves its stamp launch in flight: the next lane's call waits for it (motion_enqueue)"""
    frames = moved_patch_sequence(66)
    assert_shapes(oracle_lists(frames, 1), 1)
    for cam in (0, 1):
        set_cam(eng, cam, 1, hold=hold)
    want = [by_call(eng, [0], [f]) for f in frames]
    t = Table(eng, frames, cams=[1] * 4, lead=8)
    try:
        assert eng.num_slots >= 4
        eng.bind_motion(0, 4, ios=IOS)
        seen = []
        for lane in range(4):                                            # consecutive frames of the camera on different lanes, none collected yet
            eng.submit_bound(lane, [lane])
            seen.append(stats(eng, lane))
        for lane in range(4):
            eng.collect_bound(lane)
        for step in range(4):
            assert seen[step] == want[step][1], step
            assert t.rows[step].tobytes() == want[step][0][0].tobytes(), step
        assert len(want[2][1][0][0][0]) >= 2 and (t.rows[2]["confidence"] > 0).any()      # a step with a region
        if hold is not None:
            np.testing.assert_array_equal(eng.debug_motion_age(1), eng.debug_motion_age(0))
            assert eng.debug_motion_age(0).any()
    finally:
        t.close()


# ---- 4. a hold and an ignore mask -------------------------------------------------------------------------------------------------------------
def test_a_hold_and_an_ignore_mask_that_covers_the_moved_patch(eng, cams):
    a, _, b, _ = moved_patch_sequence(90)
    c = b.copy()
    c[150:174, 200:224] = a[24:48, 40:64]                                # a second patch, outside the mask
    frames = [a, a, b, b, c, c, c, c]
    mask = np.zeros((H, W), np.uint8)
    mask[24:64, 40:96] = 1                                               # where the first patch was and where it went
    assert_shapes(oracle_lists(frames[:4], 0), 0)                        # without the mask: a region at step 2
    for cam in (0, 1):
        set_cam(eng, cam, 0, hold=(2, 0), mask=mask)
    t = Table(eng, [a], cams=[1], lead=8)
    try:
        eng.bind_motion(0, 1, ios=IOS)
        lists, ignored, held, seen = [], [], [], False
        for step, f in enumerate(frames):
            want, want_stats = by_call(eng, [0], [f])
            t.views[0][...] = f
            got = t.run(2, [0])[0]
            assert stats(eng, 2) == want_stats, step
            assert got.tobytes() == want[0].tobytes(), step
            np.testing.assert_array_equal(eng.debug_motion_age(1), eng.debug_motion_age(0))
            lists.append(want_stats[0][0][0])
            held.append(want_stats[1][1][0])
            ignored.append(want_stats[2][0])
            seen = seen or bool((got["confidence"] > 0).any())
        assert lists[2] == [] and ignored[2] > 0                         # the region of step 2 is gone: its cells are ignored
        assert [len(l) for l in lists] == [0, 0, 0, 0, 1, 1, 1, 0]        # the second patch: changed at step 4, held at 5 and 6
        assert held[5] > 0 and held[6] > 0 and seen
    finally:
        t.close()


# ---- 5. the four kinds in one table -----------------------------------------------------------------------------------------------------------
def test_motion_gated_tiled_and_untiled_entries_in_one_table(eng, cams):
    frames = moved_patch_sequence(65)
    assert_shapes(oracle_lists(frames, 1), 1)
    other = synthetic_frame(W, H, 81)
    for cam in (0, 1):
        set_cam(eng, cam, 1)
    for cam in (2, 3):
        eng.set_camera_tiles(cam, W, H, [ROI, WHOLE], 8, 1, 0)
    # 0, 1: motion camera 1   2: gated camera 3   3: tiled   4: untiled
    t = Table(eng, [frames[0], frames[2], frames[0], other, other], cams=[1, 1, 3, -1, -1], lead=8)
    try:
        eng.bind_motion(0, 2, ios=IOS)
        eng.bind_tiles(2, 1, None, ios=IOS, gated=True)
        eng.bind_tiles(3, 1, GRID, ios=IOS)
        tiled = tiled_rows(eng, [other], [GRID])[0]
        plain = np.zeros((1, 100), ROW_DTYPE)
        eng.detect_batch([other], list(plain))
        plain_a = np.zeros((1, 100), ROW_DTYPE)
        eng.detect_batch([frames[0]], list(plain_a))
        for step, f in enumerate(frames):
            want, want_stats = by_call(eng, [0], [f])
            gated = np.zeros(100, ROW_DTYPE)
            eng.detect_gated([f], [2], [gated], ios=IOS)
            ran = gate(eng, 0)
            entry = 0 if step < 2 else 1                                 # (entry 0 shows a, entry 1 shows b)
            t.views[2][...] = f
            t.rows.view(np.uint8)[...] = 0xA5
            eng.submit_bound(0, [entry])                                 # every kind in a submit of its own, all four in flight
            got_stats = stats(eng, 0)
            eng.submit_bound(1, [2])
            got_ran = gate(eng, 1)
            eng.submit_bound(2, [3])
            eng.submit_bound(3, [4])
            for lane in range(4):
                eng.collect_bound(lane)
            assert got_stats == want_stats and t.rows[entry].tobytes() == want[0].tobytes(), step
            assert got_ran == ran and t.rows[2].tobytes() == gated.tobytes(), step
            assert t.rows[3].tobytes() == tiled.tobytes() and t.rows[4].tobytes() == plain[0].tobytes(), step
            assert (t.rows[1 - entry].view(np.uint8) == 0xA5).all()
        assert len(want_stats[0][0][0]) == 1 and (want[0]["confidence"] > 0).any()
        eng.bind_tiles(0, 2, None)                                       # wz_bind_tiles(.., 0, NULL, .., 0): the motion entries are untiled again
        assert t.run(1, [0])[0].tobytes() == plain_a[0].tobytes()
        pair = np.zeros((2, 100), ROW_DTYPE)
        eng.detect_batch([frames[0], other], list(pair))
        assert t.run(1, [0, 4]).tobytes() == pair.tobytes()              # ... and share a batch with an untiled entry
        eng.bind_motion(0, 2, ios=IOS)
        assert raw_submit(eng, 1, [0, 4])[0] == _lib.WZ_EINVAL
        t.bind()                                                         # wz_bind_frames replaces the table: the descriptions are gone
        assert t.run(3, [0])[0].tobytes() == plain_a[0].tobytes()
        assert t.run(3, [3])[0].tobytes() == plain[0].tobytes()
    finally:
        t.close()


# ---- 6. every refusal ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_numbers_and_change_nothing(eng, cams):
    frames = moved_patch_sequence(90)
    assert_shapes(oracle_lists(frames, 1), 1)
    a = frames[0]
    for cam in (0, 1, 8, 9, 10):
        set_cam(eng, cam, 1)                                             # 1 + 2 configured tiles each: four such cameras exceed max_batch 8
    set_cam(eng, 7, 1, w=96, h=64)                                       # settings of another size than its frames
    # 0, 1: motion camera 1   2: no camera   3: camera 4   4: tiled, camera 5   5: camera 6, no settings   6: camera 7   7, 8, 9: cameras 8, 9, 10
    t = Table(eng, [a] * 10, cams=[1, 1, -1, 4, 5, 6, 7, 8, 9, 10], lead=8)
    try:
        eng.bind_motion(0, 2, ios=IOS)
        eng.bind_motion(3, 1, iou=0.5, ios=IOS)
        eng.bind_tiles(4, 1, GRID, ios=IOS)
        for entry in (5, 6, 7, 8, 9):
            eng.bind_motion(entry, 1, ios=IOS)
        steps = itertools.count()

        def good_call():
            """the next frame of the sequence through both cameras: camera 1's decisions are what camera 0's are"""
            f = frames[next(steps) % 4]
            want, want_stats = by_call(eng, [0], [f])
            t.views[0][...] = f
            got = t.run(2, [0])[0]
            assert stats(eng, 2) == want_stats and got.tobytes() == want[0].tobytes()
            t.rows.view(np.uint8)[...] = 0xA5
            return want_stats[0][0][0]

        lists = [good_call()]
        t.views[0][...] = a

        def refused(rc_msg, code, *names):
            rc, msg = rc_msg
            assert rc == code, (rc, msg)
            assert all(str(n) in msg for n in names), msg
            assert t.untouched()
            with pytest.raises(ValueError):
                eng.collect_bound(2)                                     # nothing is in flight on the lane
            lists.append(good_call())

        nan = float("nan")
        # bind
        refused(raw_bind_motion(eng, 0, 1, 0.6, 1.0, handle=False), _lib.WZ_EINVAL, "null engine")
        refused(raw_bind_motion(eng, 8, 3, 0.6, 1.0), _lib.WZ_EINVAL, "8 .. 10", "10 entries")                  # first / count outside the table
        refused(raw_bind_motion(eng, -1, 1, 0.6, 1.0), _lib.WZ_EINVAL, "-1", "10 entries")
        refused(raw_bind_motion(eng, 2, 0, 0.6, 1.0), _lib.WZ_EINVAL, "10 entries")
        refused(raw_bind_motion(eng, 3, 2, 0.6, 1.0), _lib.WZ_EINVAL, "entries 3 .. 4", "entry 3 has 4", "entry 4 has 5")      # two camera ids
        refused(raw_bind_motion(eng, 1, 2, 0.6, 1.0), _lib.WZ_EINVAL, "entries 1 .. 2", "entry 1 has 1", "entry 2 has -1")
        refused(raw_bind_motion(eng, 2, 1, 0.6, 1.0), _lib.WZ_EINVAL, "entries 2 .. 2", "entry 2 has -1")       # no camera id
        refused(raw_bind_motion(eng, 4, 1, nan, 1.0), _lib.WZ_EINVAL, "thresholds", "nan")
        refused(raw_bind_motion(eng, 4, 1, 0.6, -0.5), _lib.WZ_EINVAL, "thresholds", "-0.5")
        refused(raw_bind_motion(eng, 4, 1, -1.0, 1.0), _lib.WZ_EINVAL, "thresholds", "-1")
        # no refused bind changed an entry: 2 is still untiled, 4 still tiled
        want = np.zeros((1, 100), ROW_DTYPE)
        eng.detect_batch([a], list(want))
        assert t.run(2, [2])[0].tobytes() == want[0].tobytes()
        assert t.run(2, [4])[0].tobytes() == tiled_rows(eng, [a], [GRID], cams=[5])[0].tobytes()
        t.rows.view(np.uint8)[...] = 0xA5
        # submit
        refused(raw_submit(eng, 2, [0, 4]), _lib.WZ_EINVAL, "entry 0", "entry 4", "motion", "tiled")             # motion beside tiled
        refused(raw_submit(eng, 2, [4, 1]), _lib.WZ_EINVAL, "entry 4", "entry 1", "tiled", "motion")
        refused(raw_submit(eng, 2, [0, 2]), _lib.WZ_EINVAL, "entry 0", "entry 2", "motion", "untiled")
        refused(raw_submit(eng, 2, [0, 3]), _lib.WZ_EINVAL, "entry 0", "entry 3", "0.5")                         # two threshold pairs
        refused(raw_submit(eng, 2, [0, 1]), _lib.WZ_EINVAL, "camera 1", "frames 0 and 1", "motion")              # the same camera twice
        refused(raw_submit(eng, 2, [5]), _lib.WZ_EINVAL, "camera 6", "no motion settings")                       # a camera without settings
        refused(raw_submit(eng, 2, [0, 6]), _lib.WZ_EINVAL, "frame 1", "320x240", "camera 7", "96x64")           # settings of another size
        refused(raw_submit(eng, 2, [0, 7, 8, 9]), _lib.WZ_ELIMIT, "12 tiles", "whole_frame + max_regions", "max_batch 8")
        refused(raw_submit(eng, 2, [10]), _lib.WZ_EINVAL, "entry 10", "[0,10)")
        # the camera went through its sequence as camera 0 did, whatever was refused in between
        # (a, a, b, b, a, a, b, b, ...: from the fifth call on the patch moves back and forth)
        assert len(lists) == 20 and [len(l) for l in lists] == [1, 1, 2, 1] + [2, 1, 2, 1] * 4
    finally:
        t.close()


# ---- 7. plugin and worker ---------------------------------------------------------------------------------------------------------------------
CLOCK = (240, 200, 48, 16)                                               # x, y, w, h: a burnt-in clock, ignored


def with_clock(f, k):
    f = f.copy()
    x, y, w, h = CLOCK
    f[y:y + h, x:x + w] = (230, 230, 230) if k % 2 else (15, 15, 15)
    return f


def shm_camera(pictures):
    """{"porch": a FrameBuffer with one Frame per picture}"""
    import shm_standins as shm
    ctx = shm.spawn_context()
    fb = shm.FrameBuffer(ctx, len(pictures), W, H)
    for f, pic in zip(fb.frames, pictures):
        np.frombuffer(f.image.get_obj(), np.uint8)[:] = pic.reshape(-1)
    return {"porch": fb}


def test_plugin_and_worker_with_motion_hold_and_ignore(model_dir_default):
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    from watsor_amd.share import DetectionArray
    a, _, b, _ = moved_patch_sequence(65)
    pictures = [with_clock(f, k) for k, f in enumerate([a, a, b, b])]
    back = with_clock(a, 4)                                              # the fifth step: the patch moves back
    assert_shapes(oracle_lists([a, a, b, b], 1), 1)
    options = {"motion": {"threshold": THR, "max_regions": 2, "min_side": 64, "pad": 8, "ios": IOS}, "motion_hold": {"hold": 2, "object_hold": 3},
               "ignore": {"porch": [list(CLOCK)]}, "numa": False}
    with HipObjectDetector(model_dir_default, 0, options, **SIZE) as sync, HipObjectDetector(model_dir_default, 0, options, **SIZE) as det:
        # the yardstick: a second detector, every step through detect_batch()
        sync_cams = shm_camera(pictures)                                 # (bind_cameras page-locks them: they live as long as the detector)
        assert sync.bind_cameras(sync_cams) == {"porch": 0}
        want = []
        for pic in pictures + [back]:
            rows = DetectionArray()
            sync.detect_batch([pic.shape], [pic], [rows], cameras=[0])
            want.append((bytes(rows), stats(sync.engine, 0)))
        # the whole frame first; a region at step 2 and, the patch moving back, at step 4 (the object_hold may add regions of its own); the
        # clock's 3 x 2 cells are ignored from the second step on
        assert all(s[0][0][0][0] == WHOLE for _, s in want) and len(want[2][1][0][0][0]) >= 2 and len(want[4][1][0][0][0]) >= 2
        assert [s[2] for _, s in want] == [[0]] + [[6]] * 4
        # the worker: four payloads of the camera, one piece each, on four lanes
        cams = shm_camera(pictures)
        fps = drive_worker(det, cams, [[("porch", i)] for i in range(4)])
        assert fps.count.value == 4
        assert det.bound_descriptions == [("motion", det.engine.nms_iou, IOS, 3, 0)] * 4
        assert det.plan_bound([0, 1]) == [[0], [1]]                      # one frame of a motion camera per call
        for i, f in enumerate(cams["porch"].frames):
            assert stats(det.engine, i) == want[i][1], i                 # (payload i went to lane i)
            assert bytes(f.header.get_obj().detections) == want[i][0], i
            assert f.latch.steps.value == 1
        assert (np.frombuffer(want[2][0], ROW_DTYPE)["confidence"] > 0).any()
        # one detect_batch() of the same camera continues the sequence: the layout was recorded, reference, ages and mask were not dropped
        rows = DetectionArray()
        det.detect_batch([back.shape], [back], [rows], cameras=[0])
        assert stats(det.engine, 0) == want[4][1]
        assert bytes(rows) == want[4][0]
        with pytest.raises(ValueError, match="motion configured"):
            det.bind_frame_table(cams, {"porch": 0})
        with pytest.raises(ValueError, match="motion configured"):
            det.submit_host(0, [back], [0])
