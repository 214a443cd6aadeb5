"""The two kernels of the motion hold on the GPU, alone (csrc/k_motion.hip: wz_k_motion_regions<true> through wz_stage_motion_hold,
wz_k_motion_stamp through wz_stage_motion_stamp) against tests/motion_hold_oracle.py: regions, their n, the component
count, active, held and EVERY byte of the ages, equal.  Grids are built as in test_gpu_motion_regions.py: ref = 0 and now = thr * npix + 1
where a change is wanted, thr * npix where it is not."""
import numpy as np
import pytest

import motion_hold_oracle as ho
import motion_oracle as mo
from conftest import make_engine
from watsor_amd.runtime import FMT_NV12, FMT_RGB24, ROW_DTYPE

pytestmark = pytest.mark.gpu

THR = 9
KW = dict(dilate=1, max_regions=16, min_side=48, pad=3)
SHAPES = [(1, 1), (5, 63), (3, 64), (9, 65), (68, 120)]      # (gh, gw): a wave's and a bit-map word's edges, as the region tests use them


@pytest.fixture(scope="module")
def dev_eng(model_dir_default):
    e = make_engine(model_dir_default, dev=True, max_batch=8, max_width=640, max_height=480)
    yield e
    e.close()


def bits(gh, gw, cells=()):
    C = np.zeros((gh, gw), bool)
    for y, x in cells:
        C[y, x] = True
    return C


def ages(gh, gw, cells=None):
    G = np.zeros((gh, gw), np.uint8)
    for (y, x), v in (cells or {}).items():
        G[y, x] = v
    return G


def check(eng, C, G, hold=2, W=None, H=None, fmt=FMT_RGB24, ref=True, **kw):
    """the kernel on the grids of C and the ages G (None: no age grid) against the oracle; ref False: without a reference"""
    gh, gw = C.shape
    W, H = W or 16 * gw, H or 16 * gh
    assert mo.grid_shape(W, H) == (gh, gw)
    p = dict(mo.DEFAULTS, **dict(KW, **kw))
    now, zero = mo.grids_for(C, W, H, THR)
    zero = zero if ref else None
    want = ho.step(now, zero, G, W, H, fmt, THR, hold, **p)
    got = eng.stage_motion_hold(now, zero, G, W, H, THR, hold, fmt=fmt, **p)
    assert got[:5] == want[:5], (C.shape, W, H, hold, p)
    np.testing.assert_array_equal(got[5], want[5])
    return got


@pytest.mark.parametrize("gh,gw", SHAPES)
def test_no_ages_zero_ages_and_held_corners(dev_eng, gh, gw):
    C = np.random.default_rng(gw).random((gh, gw)) < 0.12
    for W, H in ((16 * gw, 16 * gh), (16 * gw - 5, 16 * gh - 11)):      # whole cells; a partial last column and row
        none = check(dev_eng, C, None, W=W, H=H)
        zero = check(dev_eng, C, ages(gh, gw), W=W, H=H)
        assert none[:5] == zero[:5] and (none[5] == zero[5]).all() and none[4] == 0 and none[3] == int(C.sum())
        corners = ages(gh, gw, {(0, 0): 3, (0, gw - 1): 1, (gh - 1, 0): 255, (gh - 1, gw - 1): 2})
        got = check(dev_eng, C, corners, W=W, H=H, dilate=0, min_side=16, pad=0)
        assert got[3] == int((C | (corners > 0)).sum())
        empty = check(dev_eng, bits(gh, gw), corners, W=W, H=H, dilate=0, min_side=16, pad=0)      # a still picture: the held cells alone
        assert empty[3] == empty[4] == int((corners > 0).sum()) and empty[2] == len({(0, 0), (0, gw - 1), (gh - 1, 0), (gh - 1, gw - 1)})


@pytest.mark.parametrize("dilate", [0, 1])
def test_a_held_cell_diagonal_to_a_changed_cell(dev_eng, dilate):
    got = check(dev_eng, bits(9, 9, [(3, 3)]), ages(9, 9, {(4, 4): 1}), dilate=dilate, min_side=16, pad=0)
    assert got[1] == [2] and got[2:5] == (1, 2, 1)                   # 8-connected: one component of n = 2, one of its cells held
    got = check(dev_eng, bits(9, 9, [(3, 3)]), ages(9, 9, {(5, 5): 1}), dilate=dilate, min_side=16, pad=0)
    assert got[2] == (2, 1)[dilate]                                  # a gap of one cell: joined by the dilation only


def test_decay_edges(dev_eng):
    """ages 1 / 2 / 255 under changed and unchanged cells, hold 0 / 1 / 255: 1 ends, 255 does not wrap, the larger of hold and age - 1 stays"""
    G = ages(5, 63, {(0, 0): 1, (0, 1): 2, (0, 2): 255, (2, 10): 1, (2, 11): 2, (2, 12): 255, (4, 62): 255})
    C = bits(5, 63, [(2, 10), (2, 11), (2, 12), (3, 40)])
    for hold, want in ((0, [0, 1, 254, 0, 1, 254, 0]), (1, [0, 1, 254, 1, 1, 254, 1]), (255, [0, 1, 254, 255, 255, 255, 255])):
        out = check(dev_eng, C, G, hold=hold)[5]
        assert [int(out[c]) for c in ((0, 0), (0, 1), (0, 2), (2, 10), (2, 11), (2, 12), (3, 40))] == want
        assert out[4, 62] == 254


def test_seeded_ages_over_seeded_changes(dev_eng):
    rng = np.random.default_rng(6812)
    C = rng.random((68, 120)) < 0.02
    G = np.where(rng.random((68, 120)) < 0.02, rng.integers(1, 256, (68, 120)), 0).astype(np.uint8)
    got = check(dev_eng, C, G, hold=7, dilate=0, max_regions=16, min_side=300, pad=8)
    assert got[2] > 64 and got[3] > got[4] > 0                      # more components than candidates
    check(dev_eng, C, G, hold=7, fmt=FMT_NV12, dilate=1, max_regions=3, min_side=300, pad=8, min_cells=2)
    check(dev_eng, C, G, hold=7, W=1915, H=1077, dilate=1, max_regions=5, min_side=128, pad=8)


@pytest.mark.parametrize("gh,gw", SHAPES)
def test_without_a_reference_the_ages_alone_make_regions(dev_eng, gh, gw):
    G = ages(gh, gw, {(gh // 2, gw // 2): 4, (gh - 1, gw - 1): 1})
    C = np.ones((gh, gw), bool)                                      # sums that WOULD be changes against a reference of zeros
    got = check(dev_eng, C, G, ref=False, dilate=0, min_side=16, pad=0)
    assert got[3] == got[4] == int((G > 0).sum()) and len(got[0]) == got[2] == int((G > 0).sum())
    assert int(got[5].sum()) == 3 if gh * gw > 1 else True
    assert check(dev_eng, C, None, ref=False)[:5] == ([], [], 0, 0, 0)
    assert not check(dev_eng, C, ages(gh, gw), ref=False, hold=9)[5].any()


def test_without_ages_and_hold_the_regions_are_the_plain_kernels(dev_eng):
    for gh, gw in SHAPES:
        C = np.random.default_rng(gh).random((gh, gw)) < 0.1
        now, ref = mo.grids_for(C, 16 * gw, 16 * gh, THR)
        p = dict(mo.DEFAULTS, **KW)
        got = dev_eng.stage_motion_hold(now, ref, None, 16 * gw, 16 * gh, THR, 0, **p)
        assert got[:3] == dev_eng.stage_motion_regions(now, ref, 16 * gw, 16 * gh, THR, **p)
        assert not got[5].any() and got[4] == 0


def test_refused_settings(dev_eng):
    now = np.zeros((23, 40), np.uint16)
    for hold in (-1, 256):
        with pytest.raises(ValueError):
            dev_eng.stage_motion_hold(now, now, None, 640, 360, 5, hold)
    with pytest.raises(ValueError):
        dev_eng.stage_motion_hold(now, now, np.zeros((23, 41), np.uint8), 640, 360, 5, 2)
    for to in (-1, 256):
        with pytest.raises(ValueError):
            dev_eng.stage_motion_stamp(np.zeros((23, 40), np.uint8), np.zeros(100, ROW_DTYPE), np.zeros(100, np.uint8), 640, 360, to)


# ---- the stamp kernel -------------------------------------------------------------------------------------------------------------------------
def rows_of(boxes, passes=None):
    """100 rows whose first len(boxes) hold these (x_min, y_min, x_max, y_max) and pass (or `passes`); the others hold a box over the whole
    frame and pass byte 0"""
    rows, ok = np.zeros(100, ROW_DTYPE), np.zeros(100, np.uint8)
    rows["x_max"], rows["y_max"] = 100000, 100000
    for i, b in enumerate(boxes):
        rows[i]["label"] = 1
        rows[i]["x_min"], rows[i]["y_min"], rows[i]["x_max"], rows[i]["y_max"] = b
        ok[i] = 1 if passes is None else passes[i]
    return rows, ok


def check_stamp(eng, G, boxes, W, H, to, passes=None):
    rows, ok = rows_of(boxes, passes)
    want = ho.stamp(G, rows, ok, W, H, to)
    got = eng.stage_motion_stamp(G, rows, ok, W, H, to)
    np.testing.assert_array_equal(got, want)
    return got


@pytest.mark.parametrize("W,H", [(16, 16), (1003, 75), (1024, 48), (1040, 144), (1915, 1077)])      # 1 x 1, 63 x 5, 64 x 3, 65 x 9 and 120 x 68 cells
def test_stamp_boxes(dev_eng, W, H):
    gh, gw = mo.grid_shape(W, H)
    G = (np.arange(gh * gw).reshape(gh, gw) % 5).astype(np.uint8)      # ages 0 .. 4 under object_hold 3: below, equal, above
    assert (check_stamp(dev_eng, G, [], W, H, 3) == G).all()                                        # no passing row
    one = check_stamp(dev_eng, G, [(W - 1, H - 1, W - 1, H - 1)], W, H, 3)                          # one row, one (partial) cell
    assert one[-1, -1] == max(3, G[-1, -1]) and (one.ravel()[:-1] == G.ravel()[:-1]).all()
    assert (check_stamp(dev_eng, G, [(0, 0, W - 1, H - 1)], W, H, 3) == np.maximum(G, 3)).all()     # the whole frame
    assert (check_stamp(dev_eng, G, [(-7, -7, W + 50, H + 50)], W, H, 200) == 200).all()            # ... clamped
    assert (check_stamp(dev_eng, G, [(0, 0, W - 1, H - 1)], W, H, 0) == G).all()                    # object_hold 0
    assert (check_stamp(dev_eng, G, [(0, 0, W - 1, H - 1)], W, H, 3, passes=[0]) == G).all()        # pass 0
    assert (check_stamp(dev_eng, G, [(0, 0, W - 1, H - 1)], W, H, 3, passes=[2]) == G).all()        # (a pass byte is 0 or 1)
    outside = [(-9, 0, -1, 5), (W, 0, W + 5, 5), (0, H, 5, H + 5), (0, -5, 5, -1), (5, 0, 4, 5), (0, 5, 5, 4), (W - 1, H - 1, 0, 0)]
    assert (check_stamp(dev_eng, G, outside, W, H, 9) == G).all()                                   # wholly outside, inverted


def test_stamp_cell_borders(dev_eng):
    W, H = 1040, 144
    G = np.zeros(mo.grid_shape(W, H), np.uint8)
    for box, cells in (((0, 0, 15, 15), 1), ((0, 0, 16, 15), 2), ((15, 15, 16, 16), 4), ((16, 16, 31, 31), 1), ((1023, 0, 1024, 0), 2),
                       ((1008, 128, 1039, 143), 2), ((1024, 143, 5000, 5000), 1)):
        assert int((check_stamp(dev_eng, G, [box], W, H, 5) == 5).sum()) == cells, box


def test_stamp_100_overlapping_rows(dev_eng):
    W, H = 1915, 1077
    rng = np.random.default_rng(100)
    G = rng.integers(0, 12, mo.grid_shape(W, H)).astype(np.uint8)
    x0, y0 = rng.integers(-50, W, 100), rng.integers(-50, H, 100)
    boxes = [(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in zip(x0, y0, rng.integers(0, 900, 100), rng.integers(0, 700, 100))]
    passes = [int(v) for v in rng.random(100) < 0.8]
    got = check_stamp(dev_eng, G, boxes, W, H, 6, passes)
    assert (got >= G).all() and (got == 6).sum() > (G == 6).sum() and (got[G > 6] == G[G > 6]).all()
    check_stamp(dev_eng, G, boxes, W, H, 255)
