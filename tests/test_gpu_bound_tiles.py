"""Tiled and gated detection through the worker's frame table on the GPU (include/watsor_hip.h: wz_bind_tiles / wz_submit_bound /
wz_collect_bound).  Rows are compared byte for byte with what `detect_tiled` / `detect_gated` of the SAME engine give for
the same frames -- calls that are themselves pinned to tests/tile_oracle.py and tests/gate_oracle.py (test_gpu_tiled.py, test_gpu_gated.py)
-- whether a frame was staged whole by DMA or read in place from page-locked memory by the crop and activity kernels."""
import ctypes as C
import os

import numpy as np
import pytest

import conftest
import refusal_golden
from pixfmt_oracle import frame_from_rgb
from test_gpu_bound_frames import arena_with_frames
from watsor_amd import _lib
from watsor_amd.runtime import CSP_BT709, FMT_NV12, FMT_RGB24, FMT_YUYV422, RANGE_FULL, ROW_DTYPE, tile_grid
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

SIZE = dict(max_batch=8, max_width=640, max_height=480)
NV12_HD = FMT_NV12 | CSP_BT709 | RANGE_FULL
GRID = tile_grid(320, 240, 2, 2, 0.25)                       # 2 x 2 with overlap + the full frame
GRID_EVEN = tile_grid(320, 240, 2, 2, 0.25, even=True)
ROI = (32, 16, 96, 64)                                       # 2 * its bytes <= half a 320 x 240 frame's in every format: read in place, gated too
IOS = 0.6


def _dev_engine(model_dir, env):
    saved = {k: os.environ.get(k) for k in ("WZ_PRE_ROWS", "WZ_HOST_READ")}
    for k in saved:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return conftest.make_engine(model_dir, dev=True, **SIZE)      # (the knobs are read when the engine is created)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def dev_eng(model_dir_default):
    """the development library, default settings (host_read 2): `bound_source` tells which leg a frame took"""
    e = _dev_engine(model_dir_default, {})
    yield e
    e.close()


@pytest.fixture(scope="module")
def dev_staged(model_dir_default):
    """... and with WZ_HOST_READ=0: nothing is read in place"""
    e = _dev_engine(model_dir_default, {"WZ_HOST_READ": "0"})
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng(model_dir_default):
    e = conftest.make_engine(model_dir_default, **SIZE)
    yield e
    e.close()


class Table:
    """Frames back to back in one arena (the first `lead` bytes in), bound as one frame table; rows pre-filled with 0xA5."""

    def __init__(self, e, frames, fmts=None, cams=None, lead=0, register=True):
        self.e, self.n, self.register = e, len(frames), register
        self.fmts = list(fmts) if fmts is not None else [FMT_RGB24] * self.n
        self.cams = list(cams) if cams is not None else [-1] * self.n
        self.arena, self.views = arena_with_frames(frames, lead)
        if register:
            e.host_register(self.arena)
        self.rows = np.zeros((self.n, 100), ROW_DTYPE)
        self.rows.view(np.uint8)[...] = 0xA5
        self.sizes = [e.frame_geometry(v, f) for v, f in zip(self.views, self.fmts)]
        self.bind()

    def bind(self):
        self.e.bind_frames([v.ctypes.data for v in self.views], [s[0] for s in self.sizes], [s[1] for s in self.sizes], self.fmts, self.cams,
                           [self.rows[i].ctypes.data for i in range(self.n)])

    def run(self, lane, entries):
        self.e.submit_bound(lane, entries)
        self.e.collect_bound(lane)
        return self.rows[entries].copy()

    def untouched(self):
        return bool((self.rows.view(np.uint8) == 0xA5).all())

    def close(self):
        self.e.sync()
        self.e.bind_frames([], [], [], [], [], [])
        if self.register:
            self.e.host_unregister(self.arena)


def tiled_rows(e, frames, rects, fmts=None, cams=None, iou=None, ios=IOS):
    want = np.zeros((len(frames), 100), ROW_DTYPE)
    e.detect_tiled(list(frames), list(rects), list(want), cams=cams, formats=fmts, iou=iou, ios=ios)
    return want


def raw_submit(e, lane, entries):
    """(return code, message) of wz_submit_bound, without the binding's exception in between"""
    rc = e._lib.wz_submit_bound(e._h, lane, len(entries), (C.c_int32 * len(entries))(*entries))
    return rc, _lib.last_error(e._lib)


def raw_bind_tiles(e, first, count, rects, iou, ios, gated, n=None):
    arr = (C.c_int32 * (4 * max(1, len(rects or []))))(*[v for r in (rects or []) for v in r])
    rc = e._lib.wz_bind_tiles(e._h, first, count, len(rects or []) if n is None else n, C.byref(arr) if rects is not None else None,
                              iou, ios, 1 if gated else 0)
    return rc, _lib.last_error(e._lib)


# ---- 1. the staged leg ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("register", [True, False])
@pytest.mark.parametrize("kind", ["rgb24", "nv12"])
def test_staged_frames_equal_detect_tiled(dev_eng, kind, register):
    """5 tiles that cover the frame more than once: staged whole, registered or not"""
    frame, fmt, rects = synthetic_frame(320, 240, 61), FMT_RGB24, GRID
    if kind == "nv12":
        frame, fmt, rects = frame_from_rgb(frame, NV12_HD), NV12_HD, GRID_EVEN
    assert len(rects) == 5
    t = Table(dev_eng, [frame, frame], [fmt, fmt], lead=8, register=register)
    try:
        dev_eng.bind_tiles(0, 2, rects, ios=IOS)
        got = t.run(2, [1])
        assert dev_eng.bound_source(2) == [0]
        want = tiled_rows(dev_eng, [frame], [rects], [fmt])
        assert got[0].tobytes() == want[0].tobytes() and (want[0]["confidence"] > 0).any()
        assert (t.rows[0].view(np.uint8) == 0xA5).all()                  # the other entry's rows were not written
    finally:
        t.close()


def test_two_cameras_of_different_size_and_format_in_one_call(dev_eng):
    from watsor_amd.coco import COCO_CLASSES
    from watsor_amd.filter.hip_filter import HipCameraFilter
    a = synthetic_frame(320, 240, 62)
    b = frame_from_rgb(synthetic_frame(96, 64, 63), FMT_NV12)
    ra, rb = tile_grid(320, 240, 2, 2, 0.25, full_frame=False), [(0, 0, 64, 48), (30, 14, 66, 50), (0, 0, 96, 64)]
    alpha = np.zeros((240, 320), np.uint8)
    alpha[:, :200] = 255
    cfg = {"width": 320, "height": 240, "detect": [{name: {"area": 1, "confidence": 20, "zones": []}}
                                                   for name in dict.fromkeys(COCO_CLASSES[1:])]}
    flt = HipCameraFilter(dev_eng, 5, cfg, alpha=alpha, drop=True)
    t = Table(dev_eng, [a, b], [FMT_RGB24, FMT_NV12], cams=[5, -1])
    try:
        dev_eng.bind_tiles(0, 1, ra, ios=IOS)
        dev_eng.bind_tiles(1, 1, rb, ios=IOS)
        got = t.run(1, [0, 1])
        assert dev_eng.bound_source(1) == [0, 0]
        want = tiled_rows(dev_eng, [a, b], [ra, rb], [FMT_RGB24, FMT_NV12], cams=[5, -1])
        assert got.tobytes() == want.tobytes()
        assert (got[0]["label"] == 0).any()                              # the drop-mode filter ran on the merged rows of its camera ...
        assert got[0].tobytes() != tiled_rows(dev_eng, [a, b], [ra, rb], [FMT_RGB24, FMT_NV12])[0].tobytes() and (got[1]["label"] > 0).all()
    finally:
        t.close()
        flt.close()


# ---- 2. the in-place leg ----------------------------------------------------------------------------------------------------------------
IN_PLACE = {
    # a rectangle with ragged ends in a frame whose rows are 966 bytes, at an odd address: the crop kernel's byte-wise and five-dword paths
    "rgb24_odd": (322, 242, FMT_RGB24, (33, 17, 97, 63), 3),
    "rgb24_1x1": (322, 242, FMT_RGB24, (201, 119, 1, 1), 3),
    "nv12": (320, 240, NV12_HD, ROI, 8),
    "yuyv422": (320, 240, FMT_YUYV422, ROI, 8),
}


@pytest.mark.parametrize("case", sorted(IN_PLACE))
def test_frames_read_in_place_equal_staged_frames(dev_eng, dev_staged, case):
    w, h, fmt, rect, lead = IN_PLACE[case]
    frame = frame_from_rgb(synthetic_frame(w, h, 64), fmt)
    got = {}
    for name, e, source in (("in place", dev_eng, 1), ("staged", dev_staged, 0)):
        t = Table(e, [frame], [fmt], lead=lead)
        try:
            if case == "rgb24_odd":
                assert t.views[0].ctypes.data % 2 == 1 and t.views[0].strides[0] == 966
            e.bind_tiles(0, 1, [rect], ios=IOS)
            got[name] = t.run(3, [0])[0]
            assert e.bound_source(3) == [source], name
            want = tiled_rows(e, [frame], [[rect]], [fmt])[0]
            assert got[name].tobytes() == want.tobytes(), name
        finally:
            t.close()
    assert got["in place"].tobytes() == got["staged"].tobytes()
    assert case == "rgb24_1x1" or (got["staged"]["confidence"] > 0).any()


# ---- 3. gated ---------------------------------------------------------------------------------------------------------------------------
def moved_patch_sequence(seed):
    """first frame, the same again, a 24 x 24 patch moved inside the rectangle (32, 16, 96, 64) -- which lies inside tile 0 of GRID --, the same again"""
    a = synthetic_frame(320, 240, seed)
    b = a.copy()
    b[40:64, 72:96] = a[24:48, 40:64]
    b[24:48, 40:64] = synthetic_frame(320, 240, seed + 1)[24:48, 40:64]
    return [a, a, b, b]


def gated_by_call(e, cam, frames):
    """[(rows, ran mask, activity)] of one detect_gated per frame (lane 0)"""
    out = []
    for f in frames:
        rows = np.zeros(100, ROW_DTYPE)
        e.detect_gated([f], [cam], [rows], ios=IOS)
        ran, act = e.gate_stats(0)
        out.append((rows, ran[0], act[0].tolist()))
    return out


@pytest.mark.parametrize("leg", ["staged", "in place"])
def test_gated_bound_camera_equals_detect_gated(dev_eng, leg):
    rects = GRID if leg == "staged" else [ROI]
    frames = moved_patch_sequence(65)
    for cam in (0, 1):
        dev_eng.set_camera_tiles(cam, 320, 240, rects, 8, 1, 0)
    want = gated_by_call(dev_eng, 0, frames)
    t = Table(dev_eng, [frames[0]], cams=[1], lead=3)
    try:
        dev_eng.bind_tiles(0, 1, None, ios=IOS, gated=True)
        for step, f in enumerate(frames):
            t.views[0][...] = f
            t.rows.view(np.uint8)[...] = 0xA5
            got = t.run(1, [0])[0]                                       # (a still step: no batch ran, the rows come all the same)
            ran, act = dev_eng.gate_stats(1)
            assert dev_eng.bound_source(1) == [1 if leg == "in place" else 0]
            assert (ran[0], act[0].tolist()) == want[step][1:], step
            assert got.tobytes() == want[step][0].tobytes(), step
        assert want[0][1] == (1 << len(rects)) - 1 and want[1][1] == 0 and want[2][1] != 0 and want[3][1] == 0
        assert (want[0][0]["confidence"] > 0).any()
    finally:
        t.close()
        for cam in (0, 1):
            dev_eng.clear_camera_tiles(cam)


# ---- 4. lanes -----------------------------------------------------------------------------------------------------------------------------
def test_four_tiled_batches_in_flight_equal_the_serial_answers(eng):
    frames = [synthetic_frame(320, 240, 70 + i) for i in range(4)]
    t = Table(eng, frames, lead=8)
    try:
        assert eng.num_slots >= 4
        eng.bind_tiles(0, 4, GRID, ios=IOS)
        for lane in range(4):
            eng.submit_bound(lane, [lane])
        for lane in range(4):
            eng.collect_bound(lane)
        for i, f in enumerate(frames):
            assert t.rows[i].tobytes() == tiled_rows(eng, [f], [GRID])[0].tobytes(), i
    finally:
        t.close()


def test_gated_camera_over_four_lanes_equals_the_one_lane_sequence(eng):
    frames = moved_patch_sequence(66)
    for cam in (0, 1):
        eng.set_camera_tiles(cam, 320, 240, GRID, 8, 1, 0)
    want = gated_by_call(eng, 0, frames)
    t = Table(eng, frames, cams=[1] * 4, lead=8)
    try:
        eng.bind_tiles(0, 4, None, ios=IOS, gated=True)
        stats = []
        for lane in range(4):                                            # consecutive frames of the camera on different lanes, none collected yet
            eng.submit_bound(lane, [lane])
            stats.append(eng.gate_stats(lane))
        for lane in range(4):
            eng.collect_bound(lane)
        for step in range(4):
            ran, act = stats[step]
            assert (ran[0], act[0].tolist()) == want[step][1:], step
            assert t.rows[step].tobytes() == want[step][0].tobytes(), step
    finally:
        t.close()
        for cam in (0, 1):
            eng.clear_camera_tiles(cam)


# ---- 5. untouched ground --------------------------------------------------------------------------------------------------------------------
def test_untiled_entries_beside_tiled_ones_and_a_new_table(eng):
    frames = [synthetic_frame(320, 240, 80 + i) for i in range(3)]
    t = Table(eng, frames, lead=8)
    try:
        eng.bind_tiles(0, 1, GRID, ios=IOS)
        got = t.run(0, [1, 2])
        want = np.zeros((2, 100), ROW_DTYPE)
        eng.detect_batch(frames[1:], list(want))
        assert got.tobytes() == want.tobytes()
        assert t.run(1, [0])[0].tobytes() == tiled_rows(eng, frames[:1], [GRID])[0].tobytes()
        eng.bind_tiles(0, 1, None)                                       # untiled again
        eng.detect_batch(frames[:1], list(want[:1]))
        assert t.run(2, [0])[0].tobytes() == want[0].tobytes()
        eng.bind_tiles(0, 3, GRID, ios=IOS)
        t.bind()                                                         # wz_bind_frames replaces the table: the descriptions are gone
        assert t.run(3, [0])[0].tobytes() == want[0].tobytes()
    finally:
        t.close()


# ---- 6. every refusal -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_numbers_and_change_nothing(eng):
    rgb = synthetic_frame(320, 240, 90)
    nv = frame_from_rgb(rgb, FMT_NV12)
    # 0: 5 tiles   1: 4 tiles   2: untiled   3: 2 tiles, another threshold   4, 5: gated camera 3   6: gated camera 4, no layout   7: NV12, untiled
    t = Table(eng, [rgb] * 7 + [nv], [FMT_RGB24] * 7 + [FMT_NV12], cams=[-1, -1, -1, -1, 3, 3, 4, -1], lead=8)
    try:
        eng.set_camera_tiles(3, 320, 240, [ROI, (0, 0, 320, 240)], 8, 1, 2)
        eng.bind_tiles(0, 1, GRID, ios=IOS)
        eng.bind_tiles(1, 1, GRID[:4], ios=IOS)
        eng.bind_tiles(3, 1, GRID[:2], iou=0.5, ios=IOS)
        eng.bind_tiles(4, 2, None, ios=IOS, gated=True)
        eng.bind_tiles(6, 1, None, ios=IOS, gated=True)
        good = tiled_rows(eng, [rgb], [GRID])[0]
        first = t.run(0, [4])[0]                                         # camera 3: every tile runs, then a still frame is skipped
        assert eng.gate_stats(0)[0] == [0b11]
        assert t.run(0, [5])[0].tobytes() == first.tobytes() and eng.gate_stats(0)[0] == [0]
        t.rows.view(np.uint8)[...] = 0xA5

        seen = []

        def refused(rc_msg, code, *names):
            rc, msg = rc_msg
            assert rc == code, (rc, msg)
            assert all(str(n) in msg for n in names), msg
            refusal_golden.check("bound_tiles", len(seen), rc, msg)      # (the cases in the order they stand below)
            seen.append(msg)
            assert t.untouched()
            with pytest.raises(ValueError):
                eng.collect_bound(2)                                     # nothing is in flight on the lane
            assert t.run(2, [0])[0].tobytes() == good.tobytes()          # a good call behind it gives the good bytes
            t.rows.view(np.uint8)[...] = 0xA5

        refused(raw_submit(eng, 2, [0, 2]), _lib.WZ_EINVAL, "entry 0", "entry 2", "tiled", "untiled")           # mixed kinds
        refused(raw_submit(eng, 2, [4, 1]), _lib.WZ_EINVAL, "entry 4", "entry 1", "gated", "tiled")
        refused(raw_submit(eng, 2, [1, 3]), _lib.WZ_EINVAL, "entry 1", "entry 3", "0.5")                        # unequal thresholds
        refused(raw_submit(eng, 2, [0, 1]), _lib.WZ_ELIMIT, "9 tiles", "max_batch 8")                           # 5 + 4 tiles
        refused(raw_submit(eng, 2, [4, 5]), _lib.WZ_EINVAL, "camera 3", "frames 0 and 1")                       # a gated camera twice
        refused(raw_submit(eng, 2, [6]), _lib.WZ_EINVAL, "camera 4", "no tiles")                                # gated without a layout
        eng.set_camera_tiles(4, 96, 64, [(0, 0, 96, 64)], 8, 1, 0)
        refused(raw_submit(eng, 2, [6]), _lib.WZ_EINVAL, "320x240", "camera 4", "96x64")                        # ... with one of another size
        refused(raw_submit(eng, 2, [8]), _lib.WZ_EINVAL, "entry 8", "[0,8)")
        nan = float("nan")
        refused(raw_bind_tiles(eng, 6, 3, GRID, 0.6, 1.0, False), _lib.WZ_EINVAL, "6 .. 8", "8 entries")        # first / count outside the table
        refused(raw_bind_tiles(eng, -1, 1, GRID, 0.6, 1.0, False), _lib.WZ_EINVAL, "-1")
        refused(raw_bind_tiles(eng, 2, 0, GRID, 0.6, 1.0, False), _lib.WZ_EINVAL, "8 entries")
        refused(raw_bind_tiles(eng, 1, 2, [ROI, (300, 200, 21, 40)], 0.6, 1.0, False), _lib.WZ_EINVAL, "entry 1", "(300, 200, 21 x 40)", "leaves the frame")
        refused(raw_bind_tiles(eng, 7, 1, [(31, 16, 96, 64)], 0.6, 1.0, False), _lib.WZ_EINVAL, "entry 7", "(31, 16, 96 x 64)", "even")   # odd NV12 origin
        refused(raw_bind_tiles(eng, 2, 1, GRID, nan, 1.0, False), _lib.WZ_EINVAL, "thresholds", "nan")
        refused(raw_bind_tiles(eng, 2, 1, GRID, 0.6, -0.5, False), _lib.WZ_EINVAL, "thresholds", "-0.5")
        refused(raw_bind_tiles(eng, 4, 2, [ROI], 0.6, 1.0, True), _lib.WZ_EINVAL, "gated", "1 rectangles")      # gated together with rectangles
        refused(raw_bind_tiles(eng, 3, 2, None, 0.6, 1.0, True), _lib.WZ_EINVAL, "entries 3 .. 4", "entry 3 has -1")  # gated: one camera id >= 0
        refused(raw_bind_tiles(eng, 2, 1, GRID * 2, 0.6, 1.0, False), _lib.WZ_ELIMIT, "10 tiles", "1 to 8")
        refused(raw_bind_tiles(eng, 2, 1, None, 0.6, 1.0, False, n=3), _lib.WZ_EINVAL, "3 tiles")
        # no refused bind changed an entry: 1 is still 4 tiles, 2 untiled, 3 on its own threshold, 7 untiled
        assert t.run(2, [1])[0].tobytes() == tiled_rows(eng, [rgb], [GRID[:4]])[0].tobytes()
        assert t.run(2, [3])[0].tobytes() == tiled_rows(eng, [rgb], [GRID[:2]], iou=0.5)[0].tobytes()
        want = np.zeros((1, 100), ROW_DTYPE)
        eng.detect_batch([nv], list(want), formats=[FMT_NV12])
        assert t.run(2, [7])[0].tobytes() == want[0].tobytes()
        # ... and camera 3's gate is where it was: one still frame skipped (max_age 2), so the next one is skipped too and the third runs
        assert t.run(0, [4])[0].tobytes() == first.tobytes() and eng.gate_stats(0)[0] == [0]
        assert t.run(0, [5])[0].tobytes() == first.tobytes() and eng.gate_stats(0)[0] == [0b11]
    finally:
        t.close()
        eng.clear_camera_tiles(3)
        eng.clear_camera_tiles(4)


# ---- 7. plugin and worker ------------------------------------------------------------------------------------------------------------------------
def drive_worker(det, cams, batches):
    import shm_standins as shm
    from test_worker_logic import Worker, drive
    w = Worker()
    fps, it = drive(w, det, cams, [[shm.Payload(n, i) for n, i in b] for b in batches], hip_tiled_table=True, hip_metric_interval=0)
    assert w._hip_worker_state["asynchronous"] and w._hip_worker_state["plan"] is not None
    return fps


def frame_buffers(pictures):
    """{camera: FrameBuffer of two frames}, every frame of a camera showing its picture"""
    import shm_standins as shm
    ctx = shm.spawn_context()
    cams = {name: shm.FrameBuffer(ctx, 2, 320, 240) for name in pictures}
    for name, pic in pictures.items():
        for f in cams[name].frames:
            np.frombuffer(f.image.get_obj(), np.uint8)[:] = pic.reshape(-1)
    return cams


def test_plugin_and_worker_with_tiles(model_dir_default):
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    pictures = {"porch": synthetic_frame(320, 240, 95), "yard": synthetic_frame(320, 240, 96)}
    cams = frame_buffers(pictures)
    with HipObjectDetector(model_dir_default, 0, {"tiles": {"grid": [2, 2], "overlap": 0.25}, "numa": False}, **SIZE) as det:
        fps = drive_worker(det, cams, [[("porch", 0), ("yard", 0)], [("yard", 1), ("porch", 1)]])
        assert fps.count.value == 4
        assert det.plan_bound([0, 2]) == [[0], [2]]                      # 5 + 5 tiles do not fit max_batch 8
        assert [d[0] for d in det.bound_descriptions] == ["tiled"] * 4
        for name, pic in pictures.items():
            want = tiled_rows(det.engine, [pic], [GRID], ios=None)[0]
            assert (want["confidence"] > 0).any()
            for f in cams[name].frames:
                assert bytes(f.header.get_obj().detections) == want.tobytes(), name
                assert f.latch.steps.value == 1


def test_plugin_and_worker_with_a_gate_over_a_still_sequence(model_dir_default):
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    pictures = {"porch": synthetic_frame(320, 240, 97)}
    cams = frame_buffers(pictures)
    options = {"tiles": {"grid": [2, 2], "overlap": 0.25, "gate": {"threshold": 8}}, "numa": False}
    with HipObjectDetector(model_dir_default, 0, options, **SIZE) as det:
        drive_worker(det, cams, [[("porch", 0)], [("porch", 1)], [("porch", 0)]])
        assert [d[0] for d in det.bound_descriptions] == ["gated"] * 2 and det.bound_descriptions[0][3:] == (5, 0)
        assert det.plan_bound([0, 1]) == [[0], [1]]                      # one frame of a gated camera per call
        assert det.engine.gate_stats(2)[0] == [0]                        # the third payload went to lane 2: a still picture, nothing ran
        want = tiled_rows(det.engine, [pictures["porch"]], [GRID], cams=[0], ios=None)[0]
        assert (want["confidence"] > 0).any()
        assert [f.latch.steps.value for f in cams["porch"].frames] == [2, 1]
        for f in cams["porch"].frames:
            assert bytes(f.header.get_obj().detections) == want.tobytes()
