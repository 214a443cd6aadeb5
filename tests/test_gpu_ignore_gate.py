"""The activity kernel's masked instantiation on the GPU, alone (csrc/k_gate.hip: wz_k_tile_activity<true> through
wz_stage_tile_activity_ignore) against tests/ignore_oracle.py and tests/gate_oracle.py: the count leaves the ignored
cells out, the sums are the unmasked call's bytes.  Tiles of 33 x 2 and 65 x 9 cells: the edges of 32- and 64-bit mask words, and -- 65
columns over 9 strips -- a cell index strip * cols + c that is no multiple of anything; partial last cells; a tile at (7, 5) of a
larger frame, whose cells are anchored at the tile's origin."""
import numpy as np
import pytest

import gate_oracle as go
import ignore_oracle as io
from conftest import make_engine
from watsor_amd.runtime import FMT_GRAY8, FMT_RGB24, ignore_cells

pytestmark = pytest.mark.gpu

THR = 3
GRIDS = [(2, 33), (9, 65)]                  # (cell rows, cell columns)


@pytest.fixture(scope="module")
def dev_eng(model_dir_default):
    e = make_engine(model_dir_default, dev=True, max_batch=8, max_width=640, max_height=480)      # (the stage entry takes any frame)
    yield e
    e.close()


def frames_of(w, h, fmt, seed):
    """two random w x h frames: against the first one's sums about half of the second one's cells change by more than THR a pixel"""
    rng = np.random.default_rng(seed)
    shape = (h, w) if fmt == FMT_GRAY8 else (h, w, 3)
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)


def case(crows, cols, fmt, at_origin):
    tw, th = 16 * cols - 5, 16 * crows - 3                      # an 11-pixel last column, a 13-pixel last row
    rect = (0, 0, tw, th) if at_origin else (7, 5, tw, th)
    w, h = (tw, th) if at_origin else (tw + 13, th + 9)
    a, b = frames_of(w, h, fmt, 1000 * crows + cols + fmt)
    assert go.grid_shape(rect) == (crows, cols)
    return w, h, rect, a, b


@pytest.mark.parametrize("fmt", [FMT_GRAY8, FMT_RGB24], ids=["gray8", "rgb24"])
@pytest.mark.parametrize("crows,cols", GRIDS)
@pytest.mark.parametrize("at_origin", [True, False], ids=["whole", "at_7_5"])
def test_the_count_leaves_the_ignored_cells_out_and_the_sums_stay(dev_eng, fmt, crows, cols, at_origin):
    w, h, rect, a, b = case(crows, cols, fmt, at_origin)
    ref, want = go.cell_sums(a, w, h, fmt, rect), go.cell_sums(b, w, h, fmt, rect)
    C = go.changed_cells(want, ref, rect, THR)
    assert 0 < C.sum() < C.size                                 # (precondition: changed and unchanged cells)
    plain_sums, plain = dev_eng.stage_tile_activity(b, rect, fmt, ref=ref, pixel_thr=THR)
    assert plain == int(C.sum()) and plain_sums.tobytes() == want.tobytes()
    rng = np.random.default_rng(cols)
    edges = np.zeros((crows, cols), bool)
    for i in (31, 32, 63, 64, crows * cols - 1):                # the last bit of a 32- and a 64-bit word, the first of the next, the last cell
        edges.ravel()[i] = True
    masks = [rng.random((crows, cols)) < 0.4, edges, ~edges, C.copy(), ~C, np.zeros((crows, cols), bool), np.ones((crows, cols), bool)]
    for M in masks:
        sums, count = dev_eng.stage_tile_activity_ignore(b, rect, M.astype(np.uint8), fmt, ref=ref, pixel_thr=THR)
        assert count == io.activity(want, ref, M, rect, THR) == int((C & ~M).sum())
        assert sums.tobytes() == plain_sums.tobytes()
    # a tile without a mask inside a launch that has one
    sums, count = dev_eng.stage_tile_activity_ignore(b, rect, None, fmt, ref=ref, pixel_thr=THR)
    assert count == plain and sums.tobytes() == plain_sums.tobytes()
    # without a reference nothing has changed, mask or not
    sums, count = dev_eng.stage_tile_activity_ignore(b, rect, masks[0].astype(np.uint8), fmt)
    assert count == 0 and sums.tobytes() == plain_sums.tobytes()


@pytest.mark.parametrize("crows,cols", GRIDS)
def test_all_cells_ignored_gives_zero_at_every_threshold(dev_eng, crows, cols):
    w, h, rect, a, b = case(crows, cols, FMT_RGB24, False)
    ref = go.cell_sums(a, w, h, FMT_RGB24, rect)
    every = np.ones((crows, cols), np.uint8)
    for thr in (0, THR, 255):
        assert dev_eng.stage_tile_activity_ignore(b, rect, every, FMT_RGB24, ref=ref, pixel_thr=thr)[1] == 0


def test_a_painted_plane_through_the_cell_rule_of_the_tile(dev_eng):
    """wz_ignore_cells of the tile's rectangle -> the kernel: a painted block that straddles the tile's cell borders (which lie at 7 + 16 k,
    5 + 16 k of the frame) silences exactly the tile's cells it touches"""
    w, h, rect, a, b = case(9, 65, FMT_GRAY8, False)
    a = np.minimum(a, 200)
    b = a.copy()
    b[40:60, 100:160] = 255                                     # a change inside the tile (at least 55 a pixel) ...
    b[5 + 128:5 + 133, 7 + 1024:7 + 1035] = 255                 # ... and one in its last (partial) cell
    plane = np.zeros((h, w), np.uint8)
    plane[40:60, 100:160] = 1
    ref, want = go.cell_sums(a, w, h, FMT_GRAY8, rect), go.cell_sums(b, w, h, FMT_GRAY8, rect)
    M = ignore_cells(plane, rect)
    assert np.array_equal(M.astype(bool), io.cells(plane, rect)) and M.sum() == 2 * 5      # rows (40 - 5) // 16 .. (59 - 5) // 16, columns (100 - 7) // 16 .. (159 - 7) // 16
    C = go.changed_cells(want, ref, rect, THR)
    assert C.sum() == 11 and C[-1, -1] and (C & ~M.astype(bool)).sum() == 1
    assert dev_eng.stage_tile_activity(b, rect, FMT_GRAY8, ref=ref, pixel_thr=THR)[1] == int(C.sum())
    assert dev_eng.stage_tile_activity_ignore(b, rect, M, FMT_GRAY8, ref=ref, pixel_thr=THR)[1] == 1
    # the frame's own cells are another grid: as a mask of this tile they would leave changed cells of the block uncovered or cover others
    assert not np.array_equal(ignore_cells(plane)[:9, :65], M)


def test_refused_arguments(dev_eng):
    frame = np.zeros((64, 64), np.uint8)
    with pytest.raises(ValueError):
        dev_eng.stage_tile_activity_ignore(frame, (0, 0, 64, 64), np.zeros((4, 5), np.uint8), FMT_GRAY8)
    with pytest.raises(ValueError):
        dev_eng.stage_tile_activity_ignore(frame, (0, 0, 65, 64), np.zeros((4, 5), np.uint8), FMT_GRAY8)
