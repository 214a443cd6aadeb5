"""tests/motion_hold_oracle.py by hand (no GPU needed): the semantics of the motion hold on grids small enough to
work out on paper.  GRAY8 frames of 64 x 48 pixels, 4 x 3 cells; a cell is dark (0) or bright (200)."""
import numpy as np

import motion_hold_oracle as ho
import motion_oracle as mo
from watsor_amd.runtime import FMT_GRAY8, ROW_DTYPE

W, H, THR = 64, 48, 20
KW = dict(min_cells=1, dilate=0, max_regions=16, min_side=16, pad=0)
NO_ROWS = (np.zeros(100, ROW_DTYPE), np.zeros(100, np.uint8))


def frame(*bright):
    f = np.zeros((H, W), np.uint8)
    for cy, cx in bright:
        f[16 * cy:16 * cy + 16, 16 * cx:16 * cx + 16] = 200
    return f


def rows_of(*boxes, passes=None):
    """100 rows, the first of them with these (x_min, y_min, x_max, y_max); every given row passes unless `passes` says otherwise"""
    rows, ok = np.zeros(100, ROW_DTYPE), np.zeros(100, np.uint8)
    for i, b in enumerate(boxes):
        rows[i]["label"] = 1
        rows[i]["x_min"], rows[i]["y_min"], rows[i]["x_max"], rows[i]["y_max"] = b
        ok[i] = 1 if passes is None else passes[i]
    return rows, ok


def state(hold, object_hold, **kw):
    return ho.HoldState(W, H, FMT_GRAY8, THR, hold, object_hold, whole_frame=False, **dict(KW, **kw))


def cells_of(tiles):
    """the cells the (cell-aligned, unpadded) rectangles cover"""
    out = set()
    for x0, y0, w, h in tiles:
        out |= {(cy, cx) for cy in range(y0 // 16, (y0 + h + 15) // 16) for cx in range(x0 // 16, (x0 + w + 15) // 16)}
    return out


def test_hold_2_keeps_a_changed_cell_for_two_further_calls():
    s = state(2, 0)
    assert s.begin(frame()) == ([], [], 0, 0, 0)                     # the first picture: no reference
    s.finish(*NO_ROWS)
    moved = frame((1, 2))
    want = [([(32, 16, 16, 16)], [1], 1, 1, 0),                      # call 0: changed
            ([(32, 16, 16, 16)], [1], 1, 1, 1),                      # calls 1 and 2: held
            ([(32, 16, 16, 16)], [1], 1, 1, 1),
            ([], [], 0, 0, 0)]                                       # call 3: gone
    ages = [2, 1, 0, 0]
    for k in range(4):
        assert s.begin(moved) == want[k], k
        s.finish(*NO_ROWS)
        assert s.G[1, 2] == ages[k] and s.G.sum() == ages[k]


def test_object_hold_3_keeps_a_stamped_cell_for_three_further_calls():
    s = state(0, 3)
    still = frame((0, 0))
    assert s.begin(still)[0] == []                                   # call 0: nothing active ...
    s.finish(*rows_of((40, 20, 44, 30)))                             # ... but a detection inside cell (1, 2)
    assert s.G[1, 2] == 3 and s.G.sum() == 3
    for k in (1, 2, 3):
        assert s.begin(still) == ([(32, 16, 16, 16)], [1], 1, 1, 1), k
        s.finish(*NO_ROWS)
    assert s.begin(still) == ([], [], 0, 0, 0)                       # call 4
    assert not s.G.any()


def test_a_changed_cell_under_an_older_larger_age_keeps_it():
    C = np.zeros((3, 4), bool)
    C[1, 2] = True
    G = np.zeros((3, 4), np.uint8)
    G[1, 2], G[0, 0], G[2, 3] = 9, 1, 255
    G1 = ho.decay(G, C, 2)
    assert G1[1, 2] == 8 and G1[0, 0] == 0 and G1[2, 3] == 254 and G1.sum() == 8 + 254       # G - 1 wins over hold; 1 ends; 255 does not wrap
    assert ho.decay(G, C, 200)[1, 2] == 200 and ho.decay(G, C, 8)[1, 2] == 8
    assert ho.decay(np.zeros((3, 4), np.uint8), C, 0).sum() == 0


def test_a_recurring_row_refreshes_the_age():
    s = state(0, 2)
    still, row = frame(), rows_of((0, 0, 15, 15))
    for k in range(6):
        tiles = s.begin(still)[0]
        assert tiles == ([] if k == 0 else [(0, 0, 16, 16)]), k
        s.finish(*row)
        assert s.G[0, 0] == 2
    for want in ([(0, 0, 16, 16)], [(0, 0, 16, 16)], []):            # the detection stops: two further calls
        assert s.begin(still)[0] == want
        s.finish(*NO_ROWS)


def test_regions_without_a_reference():
    s = state(0, 5)
    s.begin(frame())
    s.finish(*rows_of((16, 32, 31, 47)))
    s.ref = None                                                     # (what a call without a reference sees: C = 0 everywhere)
    assert s.begin(frame((0, 3))) == ([(16, 32, 16, 16)], [1], 1, 1, 1)
    now = np.zeros((3, 4), np.uint16)
    G = np.zeros((3, 4), np.uint8)
    G[2, 1] = 1
    assert ho.step(now, None, G, W, H, FMT_GRAY8, THR, 7, **KW)[:5] == ([(16, 32, 16, 16)], [1], 1, 1, 1)
    assert ho.step(now, None, None, W, H, FMT_GRAY8, THR, 7, **KW)[:5] == ([], [], 0, 0, 0)


def test_n_counts_held_cells_and_a_held_cell_beside_a_changed_one_is_one_component():
    s = state(3, 0, min_cells=2)
    s.begin(frame())
    s.finish(*NO_ROWS)
    assert s.begin(frame((1, 1)))[:3] == ([], [], 0)                 # one changed cell: below min_cells = 2
    s.finish(*NO_ROWS)
    tiles, n, comps, act, held = s.begin(frame((1, 1), (1, 2)))      # its neighbour changes, (1, 1) is held: one component of n = 2
    assert (tiles, n, comps, act, held) == ([(16, 16, 32, 16)], [2], 1, 2, 1)
    s.finish(*NO_ROWS)
    assert s.G[1, 1] == 2 and s.G[1, 2] == 3
    # diagonal contact joins too (8-connected); two cells apart does not at dilate 0 and does at dilate 1
    G = np.zeros((3, 4), np.uint8)
    G[0, 0] = 4
    now, ref = mo.grids_for(np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]], bool), W, H, THR)
    assert ho.step(now, ref, G, W, H, FMT_GRAY8, THR, 1, **KW)[1:5] == ([2], 1, 2, 1)
    now, ref = mo.grids_for(np.array([[0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]], bool), W, H, THR)
    assert ho.step(now, ref, G, W, H, FMT_GRAY8, THR, 1, **KW)[1:5] == ([1, 1], 2, 2, 1)
    assert ho.step(now, ref, G, W, H, FMT_GRAY8, THR, 1, **dict(KW, dilate=1))[1:5] == ([2], 1, 2, 1)


def stamped(*boxes, W=W, H=H, to=7, passes=None, age=None):
    gh, gw = mo.grid_shape(W, H)
    age = np.zeros((gh, gw), np.uint8) if age is None else age
    out = ho.stamp(age, *rows_of(*boxes, passes=passes), W, H, to)
    return {(int(y), int(x)) for y, x in zip(*np.nonzero(out == to))} if not age.any() else out


def test_box_to_cells():
    assert stamped((0, 0, 15, 15)) == {(0, 0)}                                   # x_max = 15 stays in column 0 ...
    assert stamped((0, 0, 16, 15)) == {(0, 0), (0, 1)}                           # ... 16 is column 1
    assert stamped((15, 15, 16, 16)) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert stamped((-40, -3, 3, 3)) == {(0, 0)}                                  # a negative x_min is clamped to 0
    assert stamped((50, 40, 900, 900)) == {(2, 3)}                               # x_max >= W, y_max >= H are clamped to the last pixel
    assert stamped((-5, -5, -1, 10)) == set() and stamped((64, 0, 80, 10)) == set() and stamped((0, 48, 10, 60)) == set()      # wholly outside: x0 > x1
    assert stamped((30, 10, 20, 20)) == set() and stamped((10, 30, 20, 20)) == set()                                          # inverted boxes
    assert stamped((0, 0, 63, 47), passes=[0]) == set()                          # pass 0
    assert stamped((0, 0, 63, 47), (20, 20, 21, 21), passes=[0, 1]) == {(1, 1)}
    assert stamped((0, 0, 63, 47)) == {(y, x) for y in range(3) for x in range(4)}
    some = np.array([[0, 1, 2, 3]] * 3, np.uint8)
    assert (stamped((0, 0, 63, 47), to=0, age=some) == some).all()               # object_hold 0 stamps nothing
    # 70 x 40 pixels: 5 x 3 cells, the last column 6 pixels wide, the last row 8 high
    assert stamped((64, 32, 69, 39), W=70, H=40) == {(2, 4)}
    assert stamped((63, 31, 200, 200), W=70, H=40) == {(1, 3), (1, 4), (2, 3), (2, 4)}
    age = np.array([[1, 7, 9, 0]] * 3, np.uint8)
    out = stamped((0, 0, 63, 15), age=age)
    assert out[0].tolist() == [7, 7, 9, 7] and out[1:].tolist() == [[1, 7, 9, 0]] * 2 and age[0, 0] == 1      # below, equal, above; the input is left alone


def test_reset_and_refused_calls():
    s = state(2, 2)
    s.begin(frame())
    s.finish(*rows_of((0, 0, 5, 5)))
    s.begin(frame((2, 3)))
    s.finish(*NO_ROWS)
    assert s.G[0, 0] == 1 and s.G[2, 3] == 2 and s.ref is not None
    before = s.G.copy()
    s.begin(frame((1, 1)))                                           # a call that is refused never finishes: nothing has changed
    assert (s.G == before).all()
    assert cells_of(s.begin(frame((2, 3)))[0]) == {(0, 0), (2, 3)}
    s.reset()
    assert not s.G.any() and s.ref is None
    assert s.begin(frame((2, 3))) == ([], [], 0, 0, 0)
