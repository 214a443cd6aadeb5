"""tests/gate_oracle.py against answers worked out by hand (no GPU): the luma of every format, cell sums with partial edge cells, the
threshold's boundary and the rule which tiles run."""
import numpy as np
import pytest

import gate_oracle as go

RGB, NV12, I420, YUYV, UYVY, GRAY, BGR = range(7)


def test_luma_known_answers():
    # (77 * 255 + 128) >> 8 = 77, (150 * 255 + 128) >> 8 = 149, (29 * 255 + 128) >> 8 = 29; white: (256 * 255 + 128) >> 8 = 255
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [10, 20, 30]]], np.uint8)
    want = [77, 149, 29, 255, (770 + 3000 + 870 + 128) >> 8]
    assert go.luma(px, 5, 1, RGB).tolist() == [want]
    assert go.luma(px[:, :, ::-1].copy(), 5, 1, BGR).tolist() == [want]
    assert go.luma(np.array([[7, 9]], np.uint8), 2, 1, GRAY).tolist() == [[7, 9]]
    assert go.luma(np.array([[[1, 200], [2, 201]]], np.uint8), 2, 1, YUYV).tolist() == [[1, 2]]          # Y0 U Y1 V
    assert go.luma(np.array([[[200, 1], [201, 2]]], np.uint8), 2, 1, UYVY).tolist() == [[1, 2]]          # U Y0 V Y1
    planar = np.array([1, 2, 3, 4, 250, 251], np.uint8)                                                   # 2 x 2 luma, then chroma
    assert go.luma(planar, 2, 2, NV12).tolist() == [[1, 2], [3, 4]]
    assert go.luma(planar, 2, 2, I420).tolist() == [[1, 2], [3, 4]]
    assert go.luma(px, 5, 1, RGB | 0x100).tolist() == [want]                                              # colour flags play no part


@pytest.mark.parametrize("fmt", [RGB, BGR])
def test_rgb_plus_k_on_every_channel_is_luma_plus_k(fmt):
    """the weights sum to 256"""
    rng = np.random.default_rng(3)
    px = rng.integers(0, 200, (9, 11, 3), dtype=np.uint8)
    base = go.luma(px, 11, 9, fmt).astype(int)
    for k in (1, 2, 55):
        assert (go.luma(px + np.uint8(k), 11, 9, fmt).astype(int) == base + k).all()


def test_cell_sums_one_pixel_tile():
    frame = np.arange(6 * 5, dtype=np.uint8).reshape(5, 6)
    got = go.cell_sums(frame, 6, 5, GRAY, (4, 3, 1, 1))
    assert got.dtype == np.uint16 and got.tolist() == [[3 * 6 + 4]]
    assert go.cell_pixels((4, 3, 1, 1)).tolist() == [[1]]


def test_cell_sums_partial_edge_cells():
    """a 37 x 23 tile at (2, 1) of a frame of ones, twos in the frame's last column: 3 x 2 cells, anchored at the tile's origin"""
    frame = np.ones((30, 40), np.uint8)
    frame[:, 38] = 2                       # tile column 36: the third cell column, which is 5 pixels wide
    rect = (2, 1, 37, 23)
    assert go.grid_shape(rect) == (2, 3)
    assert go.cell_pixels(rect).tolist() == [[256, 256, 80], [112, 112, 35]]
    assert go.cell_sums(frame, 40, 30, GRAY, rect).tolist() == [[256, 256, 80 + 16], [112, 112, 35 + 7]]
    full = np.full((16, 16), 255, np.uint8)
    assert go.cell_sums(full, 16, 16, GRAY, (0, 0, 16, 16)).tolist() == [[65280]]      # the largest signature fits uint16


def test_cells_follow_the_tile_not_the_frame():
    frame = np.zeros((32, 32), np.uint8)
    frame[16, 16] = 9
    assert go.cell_sums(frame, 32, 32, GRAY, (0, 0, 32, 32)).tolist() == [[0, 0], [0, 9]]
    assert go.cell_sums(frame, 32, 32, GRAY, (1, 1, 31, 31)).tolist() == [[9, 0], [0, 0]]


def test_threshold_boundary():
    """|dS| = thr * npix is not a change, one more is -- in a full cell (256 pixels) and in a partial one (5 x 7 = 35)"""
    rect = (0, 0, 21, 23)                                      # cells: 256, 80 / 112, 35 pixels
    ref = np.array([[1000, 500], [700, 300]], np.uint16)
    thr = 3
    at = ref + np.array([[3 * 256, 0], [0, 3 * 35]], np.uint16)
    assert go.activity(at, ref, rect, thr) == 0
    over = at + np.array([[1, 0], [0, 0]], np.uint16)
    assert go.changed_cells(over, ref, rect, thr).tolist() == [[True, False], [False, False]]
    under = ref - np.array([[0, 0], [0, 3 * 35 + 1]], np.uint16)
    assert go.changed_cells(under, ref, rect, thr).tolist() == [[False, False], [False, True]]
    assert go.activity(ref + np.uint16(1), ref, rect, 0) == 4  # threshold 0: any difference counts ...
    assert go.activity(ref, ref, rect, 0) == 0                 # ... none does not


def grids_of(frame, rects):
    h, w = frame.shape
    return [go.cell_sums(frame, w, h, GRAY, r) for r in rects]


def test_age_rule_on_a_still_picture():
    rects = [(0, 0, 20, 20), (4, 4, 16, 16)]
    grids = grids_of(np.full((20, 20), 7, np.uint8), rects)
    state = go.GateState(2, pixel_thr=1, min_cells=1, max_age=2)
    assert [state.step(grids, rects)[0] for _ in range(8)] == [[0, 1], [], [], [0, 1], [], [], [0, 1], []]
    state = go.GateState(2, pixel_thr=1, min_cells=1, max_age=0)              # max_age 0: never for age
    assert [state.step(grids, rects)[0] for _ in range(4)] == [[0, 1], [], [], []]
    state.reset()
    assert state.step(grids, rects)[0] == [0, 1]


def test_drift_accumulates_against_the_reference():
    """+1 a pixel per call under threshold 2: the reference stays the first picture's until the third step crosses it"""
    rects = [(0, 0, 20, 20)]
    state = go.GateState(1, pixel_thr=2)
    ran = [state.step(grids_of(np.full((20, 20), 50 + k, np.uint8), rects), rects) for k in range(5)]
    assert [r[0] for r in ran] == [[0], [], [], [0], []]
    assert [r[1] for r in ran] == [[0], [0], [0], [4], [0]]


def test_min_cells_and_per_tile_state():
    rects = [(0, 0, 32, 16), (16, 0, 16, 16)]
    a = np.zeros((16, 32), np.uint8)
    b = a.copy()
    b[:, :16] = 200                                                           # only tile 0's first cell moves
    state = go.GateState(2, pixel_thr=5, min_cells=2)
    assert state.step(grids_of(a, rects), rects) == ([0, 1], [0, 0])
    assert state.step(grids_of(b, rects), rects) == ([], [1, 0])              # one changed cell < min_cells 2
    b[:, 16:] = 200
    assert state.step(grids_of(b, rects), rects) == ([0], [2, 1])             # tile 1's single cell moved: 1 < 2
    state2 = go.GateState(2, pixel_thr=5, min_cells=1)
    state2.step(grids_of(a, rects), rects)
    b2 = a.copy()
    b2[:, :16] = 200
    assert state2.step(grids_of(b2, rects), rects) == ([0], [1, 0])           # tile 1 keeps its own reference and is skipped
