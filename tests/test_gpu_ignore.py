"""Ignore masks on the GPU, end to end (include/watsor_hip.h: wz_set_camera_ignore / wz_motion_ignore_stats): a camera
whose picture carries a "clock" -- a 48 x 16 block of pixels that changes on every call -- as a motion camera, as a gated camera, through
the worker's frame table, and through the lifecycle of its settings.  320 x 240 RGB24 frames, 20 x 15 cells.  Tile lists and gate decisions
are tests/ignore_oracle.py's; rows are, byte for byte, ONE `detect_tiled` call on the reported lists."""
import numpy as np
import pytest

import gate_oracle as go
import ignore_oracle as io
import motion_hold_oracle as ho
import tile_oracle as to
from conftest import make_engine
from test_gpu_bound_tiles import Table
from watsor_amd.runtime import FMT_RGB24, ROW_DTYPE
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

SIZE = dict(max_batch=8, max_width=640, max_height=480)
W, H = 320, 240
THR, IOS = 20, 0.6
SETTINGS = dict(min_cells=1, dilate=1, max_regions=3, min_side=128, pad=8)
PADDING = np.full(100, to.padding_row(), ROW_DTYPE)
CLOCK = (16, 8, 48, 16)                                         # x, y, w, h: cells 1 .. 3 of cell rows 0 and 1
CLOCK_CELLS = 6
BASE = synthetic_frame(W, H, 31)
# 2 x 2 tiles that overlap: origins 152 and 112 are no multiples of 16 -- a tile's cells are its own.  The clock lies in tile 0 only.
TILES = [(0, 0, 168, 128), (152, 0, 168, 128), (0, 112, 168, 128), (152, 112, 168, 128)]


def plane_of(*rects):
    p = np.zeros((H, W), np.uint8)
    for x, y, w, h in rects:
        p[y:y + h, x:x + w] = 255
    return p


MASK = plane_of(CLOCK)


def clock(k, blob=None, base=BASE):
    """the scene at call k: the clock shows something else on every call; blob = (x, y): a bright 32 x 32 patch"""
    f = base.copy()
    x, y, w, h = CLOCK
    f[y:y + h, x:x + w] = (230, 230, 230) if k % 2 else (15, 15, 15)
    if blob is not None:
        f[blob[1]:blob[1] + 32, blob[0]:blob[0] + 32] = (250, 240, 230)
    return f


@pytest.fixture(scope="module")
def eng(model_dir_default):
    e = make_engine(model_dir_default, dev=True, **SIZE)       # (the development library, for wz_debug_motion_age: the same kernels)
    yield e
    e.close()


@pytest.fixture
def cams(eng):
    ids = [51, 52, 53]
    yield ids
    for c in ids:
        eng.clear_camera_motion(c)
        eng.clear_camera_tiles(c)


def motion(eng, frames, cam_ids):
    """(rows [n, 100], pass bytes [n, 100], tile lists, the regions' n, components, ignored) of one motion call"""
    n = len(frames)
    rows, ok = np.zeros((n, 100), ROW_DTYPE), np.full((n, 100), 9, np.uint8)
    eng.detect_motion(frames, cam_ids, list(rows), passes=list(ok), ios=IOS)
    return (rows, ok) + eng.motion_stats(0) + (eng.motion_ignore_stats(0),)


def tiled(eng, frames, lists, cam_ids):
    """one `detect_tiled` call of the frames that have a tile, padding rows and pass 0 for the others"""
    n = len(frames)
    rows, ok = np.stack([PADDING] * n), np.zeros((n, 100), np.uint8)
    some = [i for i in range(n) if lists[i]]
    if some:
        r, k = np.zeros((len(some), 100), ROW_DTYPE), np.full((len(some), 100), 9, np.uint8)
        eng.detect_tiled([frames[i] for i in some], [lists[i] for i in some], list(r), cams=[cam_ids[i] for i in some], passes=list(k), ios=IOS)
        rows[some], ok[some] = r, k
    return rows, ok


def set_motion(eng, cam, mask, whole=False, **kw):
    p = dict(SETTINGS, **kw)
    eng.set_camera_motion(cam, W, H, THR, whole_frame=whole, **p)
    if mask is not None:
        eng.set_camera_ignore(cam, mask)
    return io.IgnoreMotionState(W, H, FMT_RGB24, THR, mask, whole_frame=whole, **p)


def check_call(eng, states, frames, cam_ids):
    rows, ok, lists, cells, comps, ignored = motion(eng, frames, cam_ids)
    want = [s.step(f) for s, f in zip(states, frames)]
    assert [(lists[i], cells[i], comps[i], ignored[i]) for i in range(len(frames))] == want
    want_rows, want_ok = tiled(eng, frames, lists, cam_ids)
    assert rows.tobytes() == want_rows.tobytes() and ok.tobytes() == want_ok.tobytes()
    return rows, ok, lists, ignored


# ---- 1. a motion camera ----------------------------------------------------------------------------------------------------------------------
def test_an_ignored_clock_costs_nothing_and_an_unmasked_one_a_region(eng, cams):
    masked, plain = set_motion(eng, cams[0], MASK), set_motion(eng, cams[1], None)
    for k in range(4):
        rows, ok, lists, ignored = check_call(eng, [masked, plain], [clock(k), clock(k)], cams[:2])
        assert lists[0] == [] and rows[0].tobytes() == PADDING.tobytes() and not ok[0].any()      # no tile: the padding rows, pass 0
        assert ignored == [CLOCK_CELLS if k else 0, 0]
        assert (lists[1] != []) == (k > 0)                      # the same frames without the mask: a region around the clock
    x, y, w, h = lists[1][0]
    assert len(lists[1]) == 1 and x <= CLOCK[0] and y <= CLOCK[1] and x + w >= CLOCK[0] + CLOCK[2] and y + h >= CLOCK[1] + CLOCK[3]


def test_a_blob_outside_the_mask_moves_as_ever(eng, cams):
    state = set_motion(eng, cams[0], MASK)
    seen = []
    for k, blob in enumerate([(200, 100), (200, 100), (230, 150), (60, 30), (60, 30)]):      # (60, 30): beside the clock, its region covers the clock
        rows, ok, lists, ignored = check_call(eng, [state], [clock(k, blob)], [cams[0]])
        seen.append(lists[0])
        assert ignored == [CLOCK_CELLS if k else 0]
    assert seen[0] == [] and seen[1] == [] and seen[2] != [] and seen[3] != [] and seen[4] == []
    assert (rows[0].tobytes() == PADDING.tobytes()) and not ok.any()


def test_two_masked_cameras_and_one_without_in_one_call(eng, cams):
    other = plane_of((200, 96, 64, 64))
    states = [set_motion(eng, cam, mask, max_regions=2) for cam, mask in zip(cams, (MASK, None, other))]      # (3 x 2 tiles fit max_batch 8)
    for k, blob in enumerate([(210, 100), (226, 116), (120, 170)]):
        frames = [clock(k, blob)] * 3
        rows, ok, lists, ignored = check_call(eng, states, frames, cams)
    assert ignored[0] == CLOCK_CELLS and ignored[1] == 0 and ignored[2] > 0 and lists[0] != [] and lists[2] != lists[1]


def test_object_hold_stamps_under_a_passing_row_inside_the_mask(eng, cams):
    """the whole frame ignored: no change ever counts, yet the cells under the whole-frame tile's passing rows are held and become regions"""
    cam, hold, object_hold = cams[0], 2, 3
    everything = plane_of((0, 0, W, H))
    p = dict(SETTINGS)
    eng.set_camera_motion(cam, W, H, THR, whole_frame=True, **p)
    eng.set_camera_motion_hold(cam, hold, object_hold)
    eng.set_camera_ignore(cam, everything)
    M, G, ref = io.cells(everything), np.zeros((15, 20), np.uint8), None
    passed, regions = [], []
    for k in range(3):
        f = clock(k)
        now = go.cell_sums(f, W, H, FMT_RGB24, (0, 0, W, H))
        rects, n, comps, act, held, G1, ignored = io.hold_step(now, ref, G, M, W, H, FMT_RGB24, THR, hold, **p)
        rows, ok, lists, cells, got_comps, got_ignored = motion(eng, [f], [cam])
        assert (lists[0], cells[0], got_comps[0], got_ignored[0]) == ([(0, 0, W, H)] + rects, n, comps, ignored)
        assert eng.motion_hold_stats(0) == ([act], [held]) and act == held      # never a changed cell
        assert ignored == (CLOCK_CELLS if k else 0)
        want_rows, want_ok = tiled(eng, [f], lists, [cam])
        assert rows.tobytes() == want_rows.tobytes() and ok.tobytes() == want_ok.tobytes()
        G, ref = ho.stamp(G1, rows[0], ok[0], W, H, object_hold), now
        np.testing.assert_array_equal(eng.debug_motion_age(cam), G)
        passed.append(int((ok[0] == 1).sum()))
        regions.append(lists[0][1:])
    assert passed[0] > 0, "no row of the first picture passed: the sequence says nothing about the stamp"
    assert regions[0] == [] and regions[1] != []                 # the regions are the detections': nothing else is active
    assert G.max() == object_hold and (G[M] == object_hold).any()


# ---- 2. a gated camera, 2 x 2 tiles --------------------------------------------------------------------------------------------------------------
def gated(eng, frame, cam):
    rows, ok = np.zeros(100, ROW_DTYPE), np.full(100, 9, np.uint8)
    eng.detect_gated([frame], [cam], [rows], passes=[ok], ios=IOS)
    ran, act = eng.gate_stats(0)
    return rows, ok, ran[0], act[0].tolist()


def grids_of(frame):
    return [go.cell_sums(frame, W, H, FMT_RGB24, r) for r in TILES]


SPOT = (96, 64)                                                  # one whole cell of tile 0 (and of no other tile), outside the mask
SEQUENCE = [(0, None), (1, None), (2, None), (3, SPOT), (4, SPOT), (5, None)]      # (clock, a change outside the mask inside tile 0)


def frames_of_sequence():
    out = []
    for k, at in SEQUENCE:
        f = clock(k)
        if at is not None:
            f[at[1]:at[1] + 16, at[0]:at[0] + 16] = 255 if BASE[at[1]:at[1] + 16, at[0]:at[0] + 16].mean() < 128 else 0
        out.append(f)
    return out


def test_the_clocks_tile_is_skipped_and_runs_on_a_change_outside_the_mask(eng, cams):
    masked, plain = cams[:2]
    for cam in (masked, plain):
        eng.set_camera_tiles(cam, W, H, TILES, THR, 1, 0)
    eng.set_camera_ignore(masked, MASK)
    want, bare = io.IgnoreGateState(TILES, MASK, THR), io.IgnoreGateState(TILES, None, THR)
    decisions = []
    for step, f in enumerate(frames_of_sequence()):
        ran, acts = want.step(grids_of(f), TILES)
        rows, ok, got_ran, got_acts = gated(eng, f, masked)
        assert [t for t in range(4) if got_ran >> t & 1] == ran and got_acts == acts, step
        decisions.append((got_ran, got_acts))
        ran, acts = bare.step(grids_of(f), TILES)
        _, _, got_ran, got_acts = gated(eng, f, plain)
        assert [t for t in range(4) if got_ran >> t & 1] == ran and got_acts == acts, step
        if step in (1, 2):
            assert got_ran == 0b0001 and got_acts[0] == CLOCK_CELLS      # without the mask the clock runs its tile on every call
    assert decisions[0] == (0b1111, [0, 0, 0, 0])
    assert decisions[1] == decisions[2] == (0, [0, 0, 0, 0])            # the bit clear, activity 0
    assert decisions[3][0] == 0b0001 and decisions[3][1][0] > 0         # a change outside the mask, in the same tile
    assert decisions[4] == (0, [0, 0, 0, 0]) and decisions[5][0] == 0b0001


def test_the_frame_table_honours_the_mask(eng, cams):
    """wz_bind_tiles(gated = 1) + wz_submit_bound look the camera's layout up at submit time: the same decisions and rows as wz_detect_gated"""
    direct, bound = cams[:2]
    for cam in (direct, bound):
        eng.set_camera_tiles(cam, W, H, TILES, THR, 1, 0)
        eng.set_camera_ignore(cam, MASK)
    frames = frames_of_sequence()
    t = Table(eng, [frames[0]], cams=[bound], lead=3)
    try:
        eng.bind_tiles(0, 1, None, ios=IOS, gated=True)
        seen = []
        for step, f in enumerate(frames):
            want_rows, _, want_ran, want_acts = gated(eng, f, direct)
            t.views[0][...] = f
            got = t.run(1, [0])[0]
            ran, act = eng.gate_stats(1)
            assert (ran[0], act[0].tolist()) == (want_ran, want_acts), step
            assert got.tobytes() == want_rows.tobytes(), step
            seen.append(ran[0])
        assert seen == [0b1111, 0, 0, 0b0001, 0, 0b0001]
        eng.set_camera_ignore(bound, None)                      # ... and its removal
        t.views[0][...] = clock(6)
        t.run(1, [0])
        ran, act = eng.gate_stats(1)
        assert ran[0] == 0b0001 and act[0].tolist() == [CLOCK_CELLS, 0, 0, 0]
    finally:
        t.close()


# ---- 3. lifecycle ------------------------------------------------------------------------------------------------------------------------------
def tiles_and_ignored(eng, cam, k):
    _, _, lists, _, _, ignored = motion(eng, [clock(k)], [cam])
    return lists[0], ignored[0]


def test_motion_lifecycle(eng, cams):
    cam = cams[0]
    set_motion(eng, cam, MASK)
    assert tiles_and_ignored(eng, cam, 0) == ([], 0) and tiles_and_ignored(eng, cam, 1) == ([], CLOCK_CELLS)
    eng.reset_camera_motion(cam)                                # keeps the mask
    assert tiles_and_ignored(eng, cam, 2) == ([], 0) and tiles_and_ignored(eng, cam, 3) == ([], CLOCK_CELLS)
    eng.set_camera_motion_hold(cam, 2, 0)                       # a hold behind the mask keeps it (and the reference)
    assert tiles_and_ignored(eng, cam, 4) == ([], CLOCK_CELLS) and tiles_and_ignored(eng, cam, 5) == ([], CLOCK_CELLS)
    assert eng.motion_hold_stats(0) == ([0], [0]) and not eng.debug_motion_age(cam).any()      # an ignored cell never receives `hold` from change
    eng.set_camera_motion_hold(cam, 0, 0)
    # refusals leave the camera as it was
    for bad in (np.zeros((H, W - 1), np.uint8), np.zeros((H + 1, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8)):
        with pytest.raises(ValueError, match="ignore plane is %dx%d but the camera's motion settings were made for 320x240" % bad.shape[::-1]):
            eng.set_camera_ignore(cam, bad)
    with pytest.raises(ValueError, match="camera 99 has neither motion settings nor tiles"):
        eng.set_camera_ignore(99, MASK)
    with pytest.raises(ValueError, match="camera 99 has neither motion settings nor tiles"):
        eng.set_camera_ignore(99, None)
    with pytest.raises(ValueError):
        eng.set_camera_ignore(cam, MASK.astype(np.int32))
    assert tiles_and_ignored(eng, cam, 6) == ([], CLOCK_CELLS) and tiles_and_ignored(eng, cam, 7) == ([], CLOCK_CELLS)
    eng.set_camera_ignore(cam, plane_of((200, 100, 8, 8)))      # another mask replaces the first: the clock is motion again
    tiles, ignored = tiles_and_ignored(eng, cam, 8)
    assert len(tiles) == 1 and ignored == 0
    eng.set_camera_ignore(cam, MASK)
    assert tiles_and_ignored(eng, cam, 9) == ([], CLOCK_CELLS)
    eng.set_camera_ignore(cam, None)                            # NULL removes it
    tiles, ignored = tiles_and_ignored(eng, cam, 10)
    assert len(tiles) == 1 and ignored == 0
    eng.set_camera_ignore(cam, MASK)
    eng.set_camera_motion(cam, W, H, THR, whole_frame=False, **SETTINGS)      # new motion settings drop the mask
    assert tiles_and_ignored(eng, cam, 11) == ([], 0)
    tiles, ignored = tiles_and_ignored(eng, cam, 12)
    assert len(tiles) == 1 and ignored == 0
    eng.set_camera_ignore(cam, MASK)
    eng.clear_camera_motion(cam)                                # frees it with the camera
    with pytest.raises(ValueError, match="camera %d has neither" % cam):
        eng.set_camera_ignore(cam, MASK)


def test_gate_lifecycle_and_a_camera_that_has_both(eng, cams):
    cam = cams[0]
    ran_of = lambda k: gated(eng, clock(k), cam)[2:]            # noqa: E731
    eng.set_camera_tiles(cam, W, H, TILES, THR, 1, 0)
    eng.set_camera_ignore(cam, MASK)
    assert ran_of(0) == (0b1111, [0, 0, 0, 0]) and ran_of(1) == (0, [0, 0, 0, 0])
    eng.reset_camera_tiles(cam)                                 # keeps the mask
    assert ran_of(2) == (0b1111, [0, 0, 0, 0]) and ran_of(3) == (0, [0, 0, 0, 0])
    with pytest.raises(ValueError, match="ignore plane is 319x240 but the camera's tiles were set for 320x240"):
        eng.set_camera_ignore(cam, np.zeros((H, W - 1), np.uint8))
    assert ran_of(4) == (0, [0, 0, 0, 0])
    # motion settings of another size beside the tiles: the plane fits one of them only, and neither part changes
    eng.set_camera_motion(cam, 2 * W, H, THR, whole_frame=False, **SETTINGS)
    for bad in (MASK, np.zeros((H, 2 * W), np.uint8)):
        with pytest.raises(ValueError, match="ignore plane is"):
            eng.set_camera_ignore(cam, bad)
    assert ran_of(5) == (0, [0, 0, 0, 0])
    # ... of the same size: one call gives both parts their bits
    eng.set_camera_motion(cam, W, H, THR, whole_frame=False, **SETTINGS)
    eng.set_camera_ignore(cam, MASK)
    assert tiles_and_ignored(eng, cam, 0) == ([], 0) and tiles_and_ignored(eng, cam, 1) == ([], CLOCK_CELLS) and ran_of(6) == (0, [0, 0, 0, 0])
    eng.set_camera_tiles(cam, W, H, TILES, THR, 1, 0)           # a new layout drops the gate part, the motion part stays
    assert ran_of(7)[0] == 0b1111 and ran_of(8) == (0b0001, [CLOCK_CELLS, 0, 0, 0])
    assert tiles_and_ignored(eng, cam, 2) == ([], CLOCK_CELLS)
    eng.clear_camera_tiles(cam)
    eng.set_camera_ignore(cam, None)
    assert len(tiles_and_ignored(eng, cam, 3)[0]) == 1


def test_plugin_option(model_dir_default):
    """options["ignore"] through bind_cameras: the rectangle form on one of two motion cameras"""
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    from watsor_amd.share import DetectionArray

    class Buffers:
        frames = []

    motion = {"threshold": THR, "whole_frame": False, "min_side": 128, "ios": IOS}
    with HipObjectDetector(model_dir_default, 0, {"motion": motion, "ignore": {"garage": [list(CLOCK)]}, "numa": False}, **SIZE) as det:
        with pytest.raises(ValueError, match=r"^ignore\['garage'\]: unknown camera, this detector's cameras are 'porch', 'yard'"):
            det.bind_cameras({"porch": Buffers(), "yard": Buffers()})
    with HipObjectDetector(model_dir_default, 0, {"motion": motion, "ignore": {"porch": [list(CLOCK)]}, "numa": False}, **SIZE) as det:
        ids = det.bind_cameras({"porch": Buffers(), "yard": Buffers()})
        for k in range(3):
            f = clock(k)
            rows = [DetectionArray(), DetectionArray()]
            det.detect_batch([f.shape, f.shape], [f, f], rows, cameras=[ids["porch"], ids["yard"]])
            lists = det.engine.motion_stats(0)[0]
            assert lists[0] == [] and (lists[1] != []) == (k > 0)            # porch ignores its clock, yard runs a region around it
            assert det.engine.motion_ignore_stats(0) == [CLOCK_CELLS if k else 0, 0]
            assert np.frombuffer(rows[0], dtype=ROW_DTYPE).tobytes() == PADDING.tobytes()
    with HipObjectDetector(model_dir_default, 0, {"motion": motion, "ignore": {"porch": [[300, 0, 48, 16]]}, "numa": False}, **SIZE) as det:
        ids = det.bind_cameras({"porch": Buffers()})
        f = clock(0)
        with pytest.raises(ValueError, match=r"^ignore\['porch'\]: rectangle \[300, 0, 48, 16\] does not lie inside the camera's 320x240 frame"):
            det.detect_batch([f.shape], [f], [DetectionArray()], cameras=[ids["porch"]])
