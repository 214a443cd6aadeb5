"""wz_ignore_cells (include/watsor_hip.h, csrc/wz_ignore.cpp; no GPU needed) against tests/ignore_oracle.py: the cell rule of an ignore
mask -- a 16 x 16-pixel cell is ignored iff at least one of its pixels is -- on whole frames and on a tile-anchored rectangle, and the
oracle's wrappers by hand on a 4 x 3-cell grid."""
import numpy as np
import pytest

import ignore_oracle as io
import motion_oracle as mo
from watsor_amd.runtime import ignore_cells

# (width, height) -> cells: one cell; 63 x 5 with an 11-pixel last column and row; 65 x 9
FRAMES = [(16, 16), (1003, 75), (1040, 144)]
RECT, RECT_FRAME = (7, 5, 100, 50), (128, 64)      # tile-anchored cells, odd origin, partial last cells (7 x 4 cells, 4 x 2 pixels the last)


def seeded(w, h, seed, density):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8) * 255


@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("density", [0.0005, 0.01, 1.0])
def test_whole_frame_against_the_oracle(w, h, density):
    mask = seeded(w, h, 7 * w + h, density)
    got = ignore_cells(mask)
    assert got.dtype == np.uint8 and got.shape == (-(-h // 16), -(-w // 16)) and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), io.cells(mask))
    assert density < 1.0 or got.all()


@pytest.mark.parametrize("density", [0.001, 0.02])
def test_a_rectangle_has_cells_of_its_own(density):
    w, h = RECT_FRAME
    mask = seeded(w, h, 99, density)
    got = ignore_cells(mask, RECT)
    assert got.shape == (4, 7)
    assert np.array_equal(got.astype(bool), io.cells(mask, RECT))
    # tile-anchored: cell (0, 0) of the rectangle is pixels x 7 .. 22, y 5 .. 20 of the frame -- no window of the frame's cells
    one = np.zeros((h, w), np.uint8)
    one[5, 7] = 1
    assert ignore_cells(one, RECT).nonzero() == ((0,), (0,))
    one[:] = 0
    one[4, 7] = one[5, 6] = 1                       # the frame's cell (0, 0) too, but outside the rectangle
    assert not ignore_cells(one, RECT).any() and ignore_cells(one)[0, 0] == 1
    one[:] = 0
    one[5 + 49, 7 + 99] = 1                         # the rectangle's last pixel: its partial last cell
    assert ignore_cells(one, RECT).nonzero() == ((3,), (6,))
    one[:] = 0
    one[5 + 50, 7 + 99] = one[5 + 49, 7 + 100] = 1  # one pixel below, one to the right: outside
    assert not ignore_cells(one, RECT).any()


@pytest.mark.parametrize("w,h", FRAMES[1:])
def test_one_pixel_at_each_corner_of_a_cell_marks_exactly_that_cell(w, h):
    cy, cx = 2, 5
    for y, x in ((16 * cy, 16 * cx), (16 * cy, 16 * cx + 15), (16 * cy + 15, 16 * cx), (16 * cy + 15, 16 * cx + 15)):
        mask = np.zeros((h, w), np.uint8)
        mask[y, x] = 1                              # (any nonzero value ignores)
        got = ignore_cells(mask)
        assert got.sum() == 1 and got[cy, cx] == 1
    # the partial last cell, by its last pixel
    mask = np.zeros((h, w), np.uint8)
    mask[h - 1, w - 1] = 200
    got = ignore_cells(mask)
    assert got.sum() == 1 and got[-1, -1] == 1


def test_neighbouring_pixels_across_a_cell_border_mark_different_cells():
    mask = np.zeros((64, 64), np.uint8)
    mask[15, 15] = 1
    assert ignore_cells(mask).nonzero() == ((0,), (0,))
    mask[:] = 0
    mask[16, 16] = 1
    assert ignore_cells(mask).nonzero() == ((1,), (1,))


@pytest.mark.parametrize("w,h", FRAMES)
def test_an_all_zero_plane_marks_none(w, h):
    assert not ignore_cells(np.zeros((h, w), np.uint8)).any()
    assert not ignore_cells(np.zeros(RECT_FRAME[::-1], np.uint8), RECT).any()


@pytest.mark.parametrize("rect", [(0, 0, 0, 16), (0, 0, 16, 0), (-1, 0, 16, 16), (0, -1, 16, 16), (120, 0, 9, 16), (0, 60, 16, 5),
                                  (128, 0, 1, 1), (0, 0, 129, 64), (2 ** 31 - 1, 0, 2, 1)])
def test_a_rectangle_outside_the_frame_or_empty_is_refused(rect):
    with pytest.raises(ValueError, match="empty or lies outside the 128x64"):
        ignore_cells(np.zeros((64, 128), np.uint8), rect)


def test_the_c_function_refuses_null_and_sizes_below_one():
    import ctypes as C
    from watsor_amd import _lib
    lib = _lib.load()
    plane, out = np.zeros((16, 16), np.uint8), np.zeros((1, 1), np.uint8)
    p, o = C.c_void_p(plane.ctypes.data), C.c_void_p(out.ctypes.data)
    assert lib.wz_ignore_cells(p, 16, 16, None, o) == _lib.WZ_OK
    for args in ((None, 16, 16, None, o), (p, 16, 16, None, None), (p, 0, 16, None, o), (p, 16, 0, None, o), (p, -3, 16, None, o)):
        assert lib.wz_ignore_cells(*args) == _lib.WZ_EINVAL


def test_the_python_wrapper_refuses_what_is_no_plane():
    for bad in (np.zeros((4, 4, 1), np.uint8), np.zeros((4, 4), np.int32), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError, match="ignore mask is a \\(height, width\\) uint8 array"):
            ignore_cells(bad)


# ---- the oracle's wrappers, by hand: 64 x 48 GRAY8, 4 x 3 cells, every cell its own region (dilate 0, min_side 16, pad 0)
W, H, THR = 64, 48, 20
KW = dict(min_cells=1, dilate=0, max_regions=16, min_side=16, pad=0)


def grid(*cells):
    C = np.zeros((3, 4), bool)
    for cy, cx in cells:
        C[cy, cx] = True
    return C


def test_regions_read_c_and_not_m():
    now, ref = mo.grids_for(grid((0, 0), (2, 3), (1, 2)), W, H, THR)
    rects, n, comps, ignored = io.regions(now, ref, grid((2, 3), (0, 2)), W, H, 5, THR, **KW)
    assert sorted(rects) == [(0, 0, 16, 16), (32, 16, 16, 16)] and n == [1, 1] and comps == 2 and ignored == 1
    # without the mask (2, 3) joins its neighbour (1, 2): one region of two cells, ranked first
    assert io.regions(now, ref, None, W, H, 5, THR, **KW) == ([(32, 16, 32, 32), (0, 0, 16, 16)], [2, 1], 2, 0)
    assert io.regions(now, None, grid((2, 3)), W, H, 5, THR, **KW) == ([], [], 0, 0)      # no reference: nothing changed, nothing removed


def test_hold_step_never_gives_hold_to_an_ignored_cell_but_keeps_its_age():
    now, ref = mo.grids_for(grid((0, 0), (2, 3)), W, H, THR)
    G = np.zeros((3, 4), np.uint8)
    G[2, 3], G[0, 2] = 3, 1                                       # (2, 3): ignored, changed, and held by a stamp of an earlier call
    rects, n, comps, act, held, G1, ignored = io.hold_step(now, ref, G, grid((2, 3), (1, 0)), W, H, 5, THR, hold=5, **KW)
    assert ignored == 1 and act == 3 and held == 2                # active: (0, 0) changed; (2, 3) and (0, 2) by their ages
    assert G1[0, 0] == 5 and G1[2, 3] == 2 and G1[0, 2] == 0      # the ignored cell decays, it is not raised to hold
    assert sorted(rects) == [(0, 0, 16, 16), (32, 0, 16, 16), (48, 32, 16, 16)]


def test_activity_leaves_the_ignored_cells_out():
    rect = (0, 0, W, H)
    now, ref = mo.grids_for(grid((0, 0), (0, 1), (2, 3)), W, H, THR)
    assert io.activity(now, ref, None, rect, THR) == 3
    assert io.activity(now, ref, grid((0, 1), (1, 1)), rect, THR) == 2
    assert io.activity(now, ref, np.ones((3, 4), bool), rect, THR) == 0
