"""wz_k_tile_activity (csrc/k_gate.hip) on tile rows longer than one trip of its 64-word loop: the second and later trips, the load
issued one trip ahead and carry63, which hands a three-byte pixel's first bytes from lane 63 of one trip to lane 0 of the next --
none of which a row of at most 1024 bytes reaches.  The cases are tests/gate_cases.py's NEW table; tests/test_gate_walk_cpu.py shows
without a GPU which paths the table reaches and that every seeded defect of tests/gate_walk.py changes its bytes.  Every comparison
is byte for byte against tests/gate_oracle.py / tests/tile_oracle.py."""
import numpy as np
import pytest

import gate_cases as gc
import gate_oracle as go
import gate_walk as gw
import tile_oracle as to
from conftest import make_engine
from test_gpu_gated import IOS, check_activity, gated, grids_of
from test_gpu_tiled import SIZE, nv12_of
from watsor_amd.runtime import FMT_NV12, FMT_RGB24, ROW_DTYPE
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev_eng(model_dir_default):
    e = make_engine(model_dir_default, dev=True, **SIZE)       # (the stage entry takes any frame: max_width plays no part)
    yield e
    e.close()


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.NEW, ids=[c.name for c in gc.NEW])
def test_activity_kernel_is_the_oracle_on_long_rows(dev_eng, case):
    frame = gc.frame_of(case)
    oracle = gc.oracle_view(case)
    want = go.cell_sums(oracle[0], case.w, case.h, oracle[1], case.rect)
    got, _ = dev_eng.stage_tile_activity(frame, case.rect, case.fmt)
    if got.tobytes() != want.tobytes():                        # a finding: name the seeded defects that give the kernel's bytes
        like = [d for d in gw.DEFECTS if gw.walk(*gc.walk_args(case), defect=d)[0].tobytes() == got.tobytes()]
        bad = np.argwhere(got != want)
        pytest.fail("%s: %d of %d cells differ, the first at %s; the walk gives these bytes under %s"
                    % (case.name, len(bad), want.size, bad[0].tolist(), like or "no seeded defect"))
    check_activity(dev_eng, frame, case.w, case.h, case.fmt, case.rect, case.seed, thrs=(0, 3, 255), oracle=oracle)
    if case.fill != "random":
        # the threshold's far end: against a grid that is 255 a pixel away in every cell, |dS| == 255 * pixels is no change, and is one
        # under 254 (thr * 16 * 16 = 65280 in the kernel's int)
        pixels = go.cell_pixels(case.rect)
        ref = (255 * pixels - want.astype(np.int64)).astype(np.uint16)
        assert (np.abs(want.astype(np.int64) - ref) == 255 * pixels).all()
        for thr, cells in ((255, 0), (254, want.size)):
            got, changed = dev_eng.stage_tile_activity(frame, case.rect, case.fmt, ref=ref, pixel_thr=thr)
            assert got.tobytes() == want.tobytes() and changed == cells == go.activity(want, ref, case.rect, thr), (case.name, thr)


# ---- 2. several multi-trip tiles of unequal grids in one launch, three calls ----------------------------------------------------------------------
W, H, THR = 704, 64, 8
LAYOUT = [(0, 0, 352, 64), (352, 0, 352, 64), (0, 0, 704, 64), (5, 3, 343, 30)]
LAYOUT_EVEN = LAYOUT[:3] + [(4, 2, 344, 30)]                  # 4:2:0 takes even rectangles only: the same grid of 2 x 22 cells
CAM = 27


@pytest.fixture(scope="module")
def wide_eng(model_dir_default):
    e = make_engine(model_dir_default, max_batch=8, max_width=W, max_height=H)
    yield e
    e.close()


def crops_rows(eng, frame, fmt, rects):
    """the rows of one `detect_batch` of these crops of a W x H frame, in order"""
    crops = [to.crop(frame, W, H, fmt, r).reshape(to.tile_shape(r[2], r[3], fmt)) for r in rects]
    rows = np.zeros((len(crops), 100), ROW_DTYPE)
    eng.detect_batch(crops, list(rows), formats=[fmt] * len(crops))
    return rows


@pytest.mark.parametrize("kind", ["rgb", "nv12"])
def test_three_gated_calls_on_multi_trip_tiles(wide_eng, kind):
    """RGB24: rows of 1056 bytes (two trips), 2112 (three) and 1029 (a word or two into the second) in one launch, grids of 4 x 22, 4 x 22, 4 x 44 and
    2 x 22 cells -- LDS sized by the widest, the strips past a tile's last return early, the counters go from strip to strip and back
    to zero for the next call.  NV12: the same picture in rows of at most 704 bytes, one trip: the several-tiles half of it only."""
    eng = wide_eng
    a = synthetic_frame(W, H, 31)
    b = a.copy()
    b[:, 600:640] = synthetic_frame(W, H, 41)[:, 600:640]      # inside tile 1 and the full-frame tile; there past byte 1024 of a row
    fmt, rects = FMT_RGB24, LAYOUT
    if kind == "nv12":
        a, b, fmt, rects = nv12_of(a), nv12_of(b), FMT_NV12, LAYOUT_EVEN
    assert [go.grid_shape(r) for r in rects] == [(4, 22), (4, 22), (4, 44), (2, 22)]
    state = go.GateState(len(rects), THR)
    eng.set_camera_tiles(CAM, W, H, rects, THR, 1, 0, fmt=fmt)
    try:
        rows_a = crops_rows(eng, a, fmt, rects)
        fresh_b = crops_rows(eng, b, fmt, [rects[1], rects[2]])
        assert fresh_b[0].tobytes() != rows_a[1].tobytes()     # (precondition: tile 1 sees something else in B)
        wants = [rows_a, rows_a, np.stack([rows_a[0], fresh_b[0], fresh_b[1], rows_a[3]])]
        for step, (frame, runs) in enumerate(((a, [0, 1, 2, 3]), (a, []), (b, [1, 2]))):
            predicted, want_act = state.step(grids_of(frame, W, H, fmt, rects), rects)
            assert predicted == runs, step                     # (precondition: what the oracle says runs is what this test is about)
            got, ok, ran, act = gated(eng, frame, CAM, fmt)
            assert [t for t in range(len(rects)) if ran >> t & 1] == predicted and act.tolist() == want_act, step
            want = to.merge_tiles(rects, wants[step], eng.nms_iou, IOS)
            assert got.tobytes() == want.tobytes(), step
            np.testing.assert_array_equal(ok, (want["label"] > 0).astype(np.uint8))
        assert want_act[1] > 0 and want_act[2] > 0 and want_act[0] == want_act[3] == 0
    finally:
        eng.clear_camera_tiles(CAM)
