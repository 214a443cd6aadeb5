"""tests/motion_oracle.py against scipy's labelling and against cases worked out by hand (include/watsor_hip.h: motion regions; DESIGN.md
section 19).  No GPU."""
import numpy as np
import pytest

import gate_oracle as go
import motion_oracle as mo

RGB, NV12, YUYV = 0, 1, 3


def grid(gh, gw, cells):
    C = np.zeros((gh, gw), bool)
    for y, x in cells:
        C[y, x] = True
    return C


# ---- components ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gw,gh", [(1, 1), (63, 5), (64, 3), (65, 9), (120, 68), (240, 135)])
def test_partition_is_scipys(gw, gh):
    from scipy import ndimage
    C = np.random.default_rng(1000 * gw + gh).random((gh, gw)) < 0.08
    D = mo.dilated(C, 1)
    ids = mo.components(D)
    lab, count = ndimage.label(D, structure=np.ones((3, 3), int))
    assert ((ids >= 0) == D).all() and len(np.unique(ids[D])) == count
    linear = np.arange(gh * gw).reshape(gh, gw)
    for k in range(1, count + 1):                     # every scipy component carries one id: the smallest linear index of its cells
        assert (ids[lab == k] == linear[lab == k].min()).all()


def test_serpentine_and_comb_are_one_component():
    for C in (mo.serpentine(23, 40), mo.serpentine(68, 120), mo.comb(9, 17)):
        ids = mo.components(C)
        assert set(np.unique(ids[C])) == {0}


def test_corner_contact_gap_and_dilation():
    corner = grid(6, 6, [(1, 1), (2, 2)])
    assert [c[:2] for c in mo.candidates(corner, mo.dilated(corner, 0), 1)] == [(2, 7)]       # touching at a corner: one component
    gap = grid(6, 8, [(2, 1), (2, 3)])
    assert [c[:2] for c in mo.candidates(gap, mo.dilated(gap, 0), 1)] == [(1, 17), (1, 19)]   # a one-cell gap: two at dilate 0 ...
    one = mo.candidates(gap, mo.dilated(gap, 1), 1)
    assert one == [(2, 8, 0, 4, 1, 3)]                # ... one at dilate 1: n counts C (2), the box spans D (15 cells), the id is D's first cell
    assert int(mo.dilated(gap, 1).sum()) == 15
    assert mo.candidates(gap, mo.dilated(gap, 1), 3) == []                                     # min_cells looks at n, not at the 15


def test_dilation_stays_inside_the_grid():
    C = grid(3, 4, [(0, 0), (2, 3)])
    assert mo.dilated(C, 2).all() and mo.dilated(C, 0).sum() == 2


# ---- the changed test --------------------------------------------------------------------------------------------------------------------------
def test_threshold_is_strict_on_full_and_partial_cells():
    W, H, thr = 40, 24, 7                             # 3 x 2 cells; the last column is 8 pixels wide, the last row 8 high
    npix = go.cell_pixels((0, 0, W, H))
    assert npix.tolist() == [[256, 256, 128], [128, 128, 64]]
    ref = np.full((2, 3), 30000, np.uint16)
    for y, x in ((0, 0), (1, 2), (0, 2), (1, 0)):
        for sign in (1, -1):
            now = ref.copy()
            now[y, x] = 30000 + sign * thr * npix[y, x]
            assert not mo.changed(now, ref, W, H, thr).any()
            now[y, x] = 30000 + sign * (thr * npix[y, x] + 1)
            assert mo.changed(now, ref, W, H, thr).tolist() == grid(2, 3, [(y, x)]).tolist()
    assert not mo.changed(ref + 999, None, W, H, 0).any()      # no reference: nothing has changed
    now, zero = mo.grids_for(grid(2, 3, [(1, 1)]), W, H, thr)
    assert mo.changed(now, zero, W, H, thr).tolist() == grid(2, 3, [(1, 1)]).tolist()


# ---- the walk ----------------------------------------------------------------------------------------------------------------------------------
def one_region(cell, W=640, H=360, fmt=RGB, min_side=128, pad=8):
    gh, gw = mo.grid_shape(W, H)
    rects, cells, comps = mo.regions_of(grid(gh, gw, [cell]), W, H, fmt, dilate=0, min_side=min_side, pad=pad)
    assert cells == [1] and comps == 1
    return rects[0]


def test_grow_at_corners_and_edges():
    # a cell in the middle: 16 + 2 * 8 = 32 pixels, grown by 96 -- 48 on each side
    assert one_region((10, 20)) == (320 - 8 - 48, 160 - 8 - 48, 128, 128)
    assert one_region((0, 0)) == (0, 0, 128, 128)                              # shifted right and down
    assert one_region((0, 39)) == (512, 0, 128, 128)
    assert one_region((22, 0)) == (0, 232, 128, 128)                           # the last row of cells is 8 pixels high: [352, 360), padded [344, 360)
    assert one_region((22, 39)) == (512, 232, 128, 128)
    assert one_region((10, 0)) == (0, 104, 128, 128)                           # an edge: one axis shifted
    assert one_region((0, 20)) == (264, 0, 128, 128)
    # an odd difference: the odd pixel goes right / down
    assert one_region((10, 20), min_side=129) == (320 - 8 - 48, 160 - 8 - 48, 129, 129)
    # already larger than min_side: the tight rectangle stays
    assert one_region((10, 20), min_side=16) == (312, 152, 32, 32)
    assert one_region((10, 20), min_side=16, pad=0) == (320, 160, 16, 16)


def test_frame_narrower_than_min_side():
    assert one_region((1, 1), W=100, H=360, min_side=128) == (0, 0, 100, 128)
    assert one_region((1, 1), W=100, H=90, min_side=128) == (0, 0, 100, 90)


def test_even_rule_for_nv12_and_yuyv():
    # pad 7: x in [320 - 7, 336 + 7) = [313, 343), 30 wide; min_side 33 grows by 3: [312, 345); y the same from 160: [152, 185)
    assert one_region((10, 20), fmt=RGB, min_side=33, pad=7) == (312, 152, 33, 33)
    assert one_region((10, 20), fmt=NV12, min_side=33, pad=7) == (312, 152, 34, 34)
    assert one_region((10, 20), fmt=YUYV, min_side=33, pad=7) == (312, 152, 34, 33)
    assert one_region((10, 20), fmt=NV12, min_side=16, pad=7) == (312, 152, 32, 32)          # [313, 343) -> [312, 344)
    assert one_region((22, 39), fmt=NV12, min_side=16, pad=7) == (616, 344, 24, 16)          # clipped at the frame: [617, 640) -> [616, 640), [345, 360) -> [344, 360)
    for fmt in (2, 0x10, 0x11):
        assert one_region((10, 20), fmt=fmt, min_side=33, pad=7) == (312, 152, 34, 34)
    assert one_region((10, 20), fmt=4, min_side=33, pad=7) == (312, 152, 34, 33)


def test_covered_rule_looks_at_the_final_rectangle():
    gh, gw = mo.grid_shape(640, 360)
    big = [(10, x) for x in range(20, 23)]            # n = 3, tight [312, 376) x [152, 184), grown to 128 x 128: [280, 408) x [104, 232)
    inside = (13, 24)                                 # n = 1, tight [376, 408) x [200, 232): inside the GROWN rectangle, not the tight one
    outside = (13, 26)                                # n = 1, tight [408, 440): leaves it
    C = grid(gh, gw, big + [inside, outside])
    rects, cells, comps = mo.regions_of(C, 640, 360, RGB, dilate=0, min_side=128, pad=8, max_regions=5)
    assert comps == 3 and cells == [3, 1]
    assert rects == [(280, 104, 128, 128), (360, 152, 128, 128)]
    # a dropped candidate does not use up max_regions
    rects2, cells2, _ = mo.regions_of(C, 640, 360, RGB, dilate=0, min_side=128, pad=8, max_regions=2)
    assert (rects2, cells2) == (rects, cells)


def test_ties_more_than_64_and_more_than_max_regions():
    gh, gw = mo.grid_shape(1920, 1080)
    cells = [(y, x) for y in range(0, 20, 2) for x in range(0, 14, 2)]          # 70 isolated cells, n = 1 each: ranked by id
    C = grid(gh, gw, cells)
    C[40, 60:63] = True                                                         # ... behind one component of three
    cands = mo.candidates(C, mo.dilated(C, 0), 1)
    assert len(cands) == 71 and cands[0][:2] == (3, 40 * gw + 60)
    assert [c[1] for c in cands[1:]] == sorted(y * gw + x for y, x in cells)
    rects, n, comps = mo.regions_of(C, 1920, 1080, RGB, dilate=0, min_side=16, pad=0, max_regions=16)
    assert comps == 71 and n == [3] + [1] * 15
    assert rects[1:4] == [(0, 0, 16, 16), (32, 0, 16, 16), (64, 0, 16, 16)]
    # only the first 64 by rank are looked at: a heavier component whose rectangle covers the 70 drops 63 of them one by one, and the three far
    # cells ranked behind never get their turn although one region was accepted
    F = grid(gh, gw, cells + [(60, 100), (62, 110), (64, 118)])
    F[5, 20:24] = True
    rects, n, comps = mo.regions_of(F, 1920, 1080, RGB, dilate=0, min_side=1000, pad=0, max_regions=16)
    assert comps == 74 and rects == [(0, 0, 1000, 1000)] and n == [4]
    uncut = mo.walk(mo.candidates(F, F, 1) * 1, 1920, 1080, RGB, 16, 1000, 0)
    assert uncut == (rects, n)
    far = [c for c in mo.candidates(F, F, 1) if c[1] > 60 * gw]
    assert len(far) == 3 and len(mo.walk(far, 1920, 1080, RGB, 16, 1000, 0)[0]) >= 1       # (on their own they would be regions)
    # min_cells 2 leaves the one
    assert mo.regions_of(C, 1920, 1080, RGB, min_cells=2, dilate=0, min_side=16, pad=0)[1:] == ([3], 1)


def test_state_replays_the_reference():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 40, (360, 640, 3), dtype=np.uint8)
    b = a.copy()
    b[100:148, 200:248] = 255
    st = mo.MotionState(640, 360, RGB, 20, whole_frame=False, dilate=1, min_side=128, max_regions=3, pad=8, min_cells=1)
    assert st.step(a) == ([], [], 0)
    tiles, cells, comps = st.step(b)
    assert comps == 1 and len(tiles) == 1 and cells[0] >= 4
    x0, y0, w, h = tiles[0]
    assert x0 <= 200 and y0 <= 100 and x0 + w >= 248 and y0 + h >= 148 and w == 128 and h == 128
    assert st.step(b) == ([], [], 0)
    st.reset()
    assert st.step(a) == ([], [], 0)
    whole = mo.MotionState(640, 360, RGB, 20, whole_frame=True)
    assert whole.step(a)[0] == [(0, 0, 640, 360)]
