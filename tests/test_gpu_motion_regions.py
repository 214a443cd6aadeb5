"""The region kernel on the GPU (csrc/k_motion.hip: wz_k_motion_regions, through wz_stage_motion_regions) against
tests/motion_oracle.py: rectangles, their changed cells and the component count, equal in every integer.  The grids are built as
ref = 0 and now = thr * npix + 1 where a change is wanted, thr * npix -- the largest sum that is none -- where it is not."""
import numpy as np
import pytest

import motion_oracle as mo
from conftest import make_engine
from watsor_amd.runtime import FMT_NV12, FMT_RGB24, FMT_YUYV422

pytestmark = pytest.mark.gpu

THR = 9


@pytest.fixture(scope="module")
def dev_eng(model_dir_default):
    e = make_engine(model_dir_default, dev=True, max_batch=8, max_width=640, max_height=480)
    yield e
    e.close()


def grid(gh, gw, cells=()):
    C = np.zeros((gh, gw), bool)
    for y, x in cells:
        C[y, x] = True
    return C


def check(eng, C, W=None, H=None, fmt=FMT_RGB24, thr=THR, **kw):
    """the kernel on the grids of C against the oracle on the same grids; W x H defaults to whole cells"""
    gh, gw = C.shape
    W, H = W or 16 * gw, H or 16 * gh
    assert mo.grid_shape(W, H) == (gh, gw)
    p = dict(mo.DEFAULTS, **kw)
    now, ref = mo.grids_for(C, W, H, thr)
    want = mo.regions(now, ref, W, H, fmt, thr, **p)
    assert want == mo.regions_of(C, W, H, fmt, **p)              # (the grids say what C says)
    got = eng.stage_motion_regions(now, ref, W, H, thr, fmt=fmt, **p)
    assert got == want, (C.shape, W, H, fmt, p)
    return got


def test_empty_full_and_no_reference(dev_eng):
    assert check(dev_eng, grid(23, 40)) == ([], [], 0)
    rects, cells, comps = check(dev_eng, np.ones((23, 40), bool), W=640, H=360)
    assert rects == [(0, 0, 640, 360)] and cells == [920] and comps == 1
    now, _ = mo.grids_for(np.ones((23, 40), bool), 640, 360, THR)
    assert dev_eng.stage_motion_regions(now, None, 640, 360, 0, **mo.DEFAULTS) == ([], [], 0)      # ref = null: nothing has changed


def test_threshold_edge_is_the_oracles(dev_eng):
    """thr * npix is no change and one more is, on full cells and on the partial last column, row and corner (640 x 360: 22.5 cell rows)"""
    C = grid(23, 40, [(0, 0), (22, 39), (22, 5), (7, 39)])
    rects, cells, comps = check(dev_eng, C, W=632, H=360, dilate=0, max_regions=16, min_side=16, pad=0)
    assert comps == 4 and cells == [1, 1, 1, 1]
    assert rects == [(0, 0, 16, 16), (616, 112, 16, 16), (80, 344, 16, 16), (616, 344, 16, 16)]      # (a partial cell is grown to min_side too)


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_corners_diagonal_and_gap(dev_eng, dilate):
    kw = dict(dilate=dilate, max_regions=16, min_side=16, pad=0)
    assert check(dev_eng, grid(23, 40, [(0, 0), (0, 39), (22, 0), (22, 39)]), W=640, H=360, **kw)[2] == 4
    assert check(dev_eng, grid(9, 9, [(1, 1), (2, 2), (3, 3), (4, 2)]), **kw)[2] == 1            # contact at corners only
    assert check(dev_eng, grid(9, 12, [(4, 1), (4, 3), (4, 6), (4, 10)]), **kw)[2] == (4, 2, 1)[dilate]      # gaps of 1, 2 and 3 cells: two dilated cells that touch are one component
    assert check(dev_eng, grid(12, 9, [(1, 4), (3, 4), (6, 4), (10, 4)]), **kw)[2] == (4, 2, 1)[dilate]


@pytest.mark.parametrize("gh,gw", [(23, 40), (68, 120)])
def test_serpentine_is_one_component(dev_eng, gh, gw):
    """what a labelling that stops after a fixed number of sweeps gets wrong: a one-cell-wide path through the whole grid"""
    C = mo.serpentine(gh, gw)
    rects, cells, comps = check(dev_eng, C, dilate=0, max_regions=16, min_side=16, pad=0)
    assert comps == 1 and cells == [int(C.sum())] and rects == [(0, 0, 16 * gw, 16 * gh)]
    check(dev_eng, C[:, ::-1], dilate=0, max_regions=16, min_side=16, pad=0)
    check(dev_eng, C[::-1].copy(), dilate=0, max_regions=16, min_side=16, pad=0)


def test_comb(dev_eng):
    for C in (mo.comb(23, 40), mo.comb(23, 40)[::-1].copy(), mo.comb(40, 23).T.copy()):
        assert check(dev_eng, C, dilate=0, max_regions=16, min_side=16, pad=0)[2] == 1


@pytest.mark.parametrize("gw", [1, 63, 64, 65, 120])
def test_grid_widths(dev_eng, gw):
    gh = 5 if gw > 1 else 70
    C = np.random.default_rng(gw).random((gh, gw)) < 0.12
    for dilate in (0, 1):
        check(dev_eng, C, dilate=dilate, max_regions=16, min_side=48, pad=3)
    check(dev_eng, C, W=16 * gw - 5, H=16 * gh - 11, dilate=1, max_regions=5, min_side=40, pad=8)


def test_the_largest_grid(dev_eng):
    """240 x 135 cells (3840 x 2160): near WZ_MOTION_MAX_CELLS, past what a launch gets of LDS without asking; 2 % noise and three blobs"""
    C = np.random.default_rng(2160).random((135, 240)) < 0.02
    C[20:31, 30:52] = True
    C[100:104, 200:240] = True
    C[60:90, 120:125] = True
    rects, cells, comps = check(dev_eng, C, dilate=1, max_regions=16, min_side=300, pad=8, min_cells=1)
    assert comps > 64 and len(rects) == 16 and cells[0] >= 11 * 22
    check(dev_eng, C, dilate=0, max_regions=3, min_side=300, pad=8, min_cells=4)
    with pytest.raises(ValueError, match="cells"):
        dev_eng.stage_motion_regions(np.zeros((136, 241), np.uint16), None, 3856, 2176, 1, **mo.DEFAULTS)


def test_ties_and_more_components_than_candidates(dev_eng):
    cells = [(y, x) for y in range(0, 20, 2) for x in range(0, 14, 2)]          # 70 isolated cells
    C = grid(68, 120, cells)
    rects, n, comps = check(dev_eng, C, dilate=0, max_regions=16, min_side=16, pad=0)
    assert comps == 70 and n == [1] * 16 and rects[:3] == [(0, 0, 16, 16), (32, 0, 16, 16), (64, 0, 16, 16)]      # ties: by id
    # the heaviest component's rectangle covers the 70: 63 of them are dropped one by one, and there the 64 candidates end -- the three far
    # cells, ranked 72nd to 74th, never get their turn although only one region was accepted
    C[5, 20:24] = True
    for y, x in ((60, 100), (62, 110), (64, 118)):
        C[y, x] = True
    rects, n, comps = check(dev_eng, C, dilate=0, max_regions=16, min_side=1000, pad=0)
    assert comps == 74 and n == [4] and rects == [(0, 0, 1000, 1000)]
    rects, n, comps = check(dev_eng, C, dilate=0, max_regions=16, min_side=1000, pad=0, min_cells=2)
    assert comps == 1 and n == [4]


def test_more_components_than_are_ranked_in_lds(dev_eng):
    """8160 isolated cells on the largest grid, a few of them joined: past the 2048 components the kernel ranks by counting, on to its
    repeated selection over the keys in device memory; and a grid one cell wide, where half the cells can be components"""
    C = np.zeros((135, 240), bool)
    C[0::2, 0::2] = True
    C[100, 51] = C[100, 53] = C[60, 201] = C[2, 1] = True          # joins of three, five and three cells
    rects, cells, comps = check(dev_eng, C, dilate=0, max_regions=16, min_side=16, pad=0)
    assert comps == 8160 - 4 and cells[:4] == [5, 3, 3, 1]
    assert check(dev_eng, C, dilate=0, max_regions=16, min_side=16, pad=0, min_cells=2)[2] == 3
    line = np.zeros((4600, 1), bool)
    line[0::2] = True
    line[3001] = True
    rects, cells, comps = check(dev_eng, line, dilate=0, max_regions=4, min_side=16, pad=0)
    assert comps == 2299 and cells == [3, 1, 1, 1]


@pytest.mark.parametrize("max_regions", [1, 16])
@pytest.mark.parametrize("min_cells", [1, 4])
def test_max_regions_and_min_cells(dev_eng, max_regions, min_cells):
    C = np.random.default_rng(77).random((23, 40)) < 0.05
    C[3:6, 4:7] = True
    C[15:17, 30:33] = True
    rects, cells, comps = check(dev_eng, C, W=640, H=360, dilate=1, max_regions=max_regions, min_cells=min_cells, min_side=64, pad=8)
    assert 1 <= len(rects) <= max_regions and all(n >= min_cells for n in cells)


@pytest.mark.parametrize("fmt", [FMT_RGB24, FMT_NV12, FMT_YUYV422])
def test_rectangles_the_format_can_cut(dev_eng, fmt):
    C = grid(23, 40, [(3, 3), (10, 20), (22, 39), (0, 17), (15, 0)])
    rects, _, comps = check(dev_eng, C, W=640, H=360, fmt=fmt, dilate=0, max_regions=16, min_side=33, pad=7)
    assert comps == 5 and len(rects) == 5
    ex, ey = mo.even_axes(fmt)
    for x0, y0, w, h in rects:
        assert x0 >= 0 and y0 >= 0 and x0 + w <= 640 and y0 + h <= 360
        assert not (ex and (x0 | w) & 1) and not (ey and (y0 | h) & 1)
    assert any((x0 | w) & 1 for x0, _, w, _ in rects) == (not ex)


def test_refused_settings(dev_eng):
    now = np.zeros((23, 40), np.uint16)
    for bad in (dict(threshold=256), dict(min_cells=0), dict(dilate=3), dict(max_regions=0), dict(max_regions=17), dict(min_side=15),
                dict(pad=65), dict(pad=-1)):
        kw = dict(mo.DEFAULTS, threshold=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            dev_eng.stage_motion_regions(now, now, 640, 360, **kw)
