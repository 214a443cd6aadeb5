"""The region kernel's masked instantiations on the GPU, alone (csrc/k_motion.hip: wz_k_motion_regions<false, true> and <true, true> through
wz_stage_motion_ignore) against tests/ignore_oracle.py: regions, their n, the component count, the changed cells the
mask removed and -- with a hold -- active, held and every byte of the ages, equal.  Grids are built as in test_gpu_motion_regions.py:
ref = 0 and now = thr * npix + 1 where a change is wanted, thr * npix where it is not.  The shapes are a wave's and a bit-map word's edges:
a mask word holds the 64 cells of one wave's step."""
import numpy as np
import pytest

import ignore_oracle as io
import motion_oracle as mo
from conftest import make_engine
from watsor_amd.runtime import FMT_NV12, FMT_RGB24

pytestmark = pytest.mark.gpu

THR = 9
KW = dict(dilate=1, max_regions=16, min_side=48, pad=3)
TIGHT = dict(dilate=0, min_side=16, pad=0)                      # every cell its own rectangle
SHAPES = [(1, 1), (5, 63), (3, 64), (9, 65), (68, 120)]         # (gh, gw), as the region and hold tests use them


@pytest.fixture(scope="module")
def dev_eng(model_dir_default):
    e = make_engine(model_dir_default, dev=True, max_batch=8, max_width=640, max_height=480)
    yield e
    e.close()


def bits(gh, gw, cells=()):
    C = np.zeros((gh, gw), bool)
    for i in cells:
        C.ravel()[i] = True                                     # (linear cell indices: what the mask words are indexed by)
    return C


def check(eng, C, M, W=None, H=None, fmt=FMT_RGB24, ref=True, **kw):
    """the kernel without a hold on the grids of C and the cell mask M (None: no mask pointer) against the oracle"""
    gh, gw = C.shape
    W, H = W or 16 * gw, H or 16 * gh
    assert mo.grid_shape(W, H) == (gh, gw)
    p = dict(mo.DEFAULTS, **dict(KW, **kw))
    now, zero = mo.grids_for(C, W, H, THR)
    zero = zero if ref else None
    want = io.regions(now, zero, M, W, H, fmt, THR, **p)
    got = eng.stage_motion_ignore(now, zero, None if M is None else M.astype(np.uint8), W, H, THR, fmt=fmt, **p)
    assert got == want, (C.shape, W, H, p)
    return got


def check_hold(eng, C, M, G, hold=2, W=None, H=None, fmt=FMT_RGB24, ref=True, **kw):
    """... and with a hold: the ages G (None: no age grid)"""
    gh, gw = C.shape
    W, H = W or 16 * gw, H or 16 * gh
    p = dict(mo.DEFAULTS, **dict(KW, **kw))
    now, zero = mo.grids_for(C, W, H, THR)
    zero = zero if ref else None
    want = io.hold_step(now, zero, G, M, W, H, fmt, THR, hold, **p)
    got = eng.stage_motion_ignore(now, zero, None if M is None else M.astype(np.uint8), W, H, THR, hold=hold, age=G, fmt=fmt, **p)
    assert got[:5] == want[:5] and got[6] == want[6], (C.shape, W, H, hold, p)
    np.testing.assert_array_equal(got[5], want[5])
    return got


@pytest.mark.parametrize("gh,gw", SHAPES)
def test_seeded_changes_under_a_seeded_mask(dev_eng, gh, gw):
    rng = np.random.default_rng(100 * gh + gw)
    C, M = rng.random((gh, gw)) < 0.15, rng.random((gh, gw)) < 0.3
    for W, H in ((16 * gw, 16 * gh), (16 * gw - 5, 16 * gh - 11)):      # whole cells; a partial last column and row
        got = check(dev_eng, C, M, W=W, H=H)
        assert got[3] == int((C & M).sum())
        check(dev_eng, C, M, W=W, H=H, fmt=FMT_NV12 if W % 2 == 0 and H % 2 == 0 else FMT_RGB24, max_regions=3, min_cells=2, **TIGHT)
        check_hold(dev_eng, C, M, None, W=W, H=H)


def test_more_components_than_candidates_under_a_mask(dev_eng):
    rng = np.random.default_rng(6812)
    C, M = rng.random((68, 120)) < 0.04, rng.random((68, 120)) < 0.5
    got = check(dev_eng, C, M, W=1915, H=1077, dilate=0, max_regions=16, min_side=300, pad=8)
    assert got[2] > 64 and got[3] > 64


@pytest.mark.parametrize("gh,gw", SHAPES[1:])
def test_mask_bits_at_the_edges_of_a_mask_word(dev_eng, gh, gw):
    """M exactly at cells 63, 64 and the last; C there and beside them: a bit one place off, in the neighbouring word or lane, shows"""
    last = gh * gw - 1
    at = [63, 64, last]
    beside = sorted({i for m in at for i in (m - 1, m + 1) if 0 <= i <= last} - set(at))
    M = bits(gh, gw, at)
    got = check(dev_eng, bits(gh, gw, at + beside), M, **TIGHT)
    assert got[3] == 3
    for one in at:                                              # each of the three alone, and then only its neighbours
        assert check(dev_eng, bits(gh, gw, [one]), M, **TIGHT) == ([], [], 0, 1)
    got = check(dev_eng, bits(gh, gw, beside), M, **TIGHT)
    assert got[3] == 0 and sum(got[1]) == len(beside)
    got = check(dev_eng, bits(gh, gw, at), bits(gh, gw, beside), **TIGHT)      # the complement: the mask beside, the change at
    assert got[3] == 0 and sum(got[1]) == 3


@pytest.mark.parametrize("gh,gw", SHAPES)
def test_every_changed_cell_ignored_is_a_still_picture(dev_eng, gh, gw):
    C = np.random.default_rng(gw).random((gh, gw)) < 0.2
    C.ravel()[-1] = True
    assert check(dev_eng, C, C.copy()) == ([], [], 0, int(C.sum()))
    assert check(dev_eng, C, np.ones((gh, gw), bool)) == ([], [], 0, int(C.sum()))
    assert check(dev_eng, np.ones((gh, gw), bool), np.ones((gh, gw), bool), W=16 * gw - 5, H=16 * gh - 11) == ([], [], 0, gh * gw)
    got = check_hold(dev_eng, C, C.copy(), None, hold=9)        # ... with a hold too: no active cell, no age
    assert got[:5] == ([], [], 0, 0, 0) and not got[5].any() and got[6] == int(C.sum())


@pytest.mark.parametrize("gh,gw", SHAPES)
def test_no_mask_pointer_is_the_plain_kernel(dev_eng, gh, gw):
    """a camera without a mask inside a launch that has one: wz_k_motion_regions<.., true> with WzMotionCam::ignore null"""
    C = np.random.default_rng(gh).random((gh, gw)) < 0.1
    W, H = 16 * gw, 16 * gh
    now, ref = mo.grids_for(C, W, H, THR)
    p = dict(mo.DEFAULTS, **KW)
    got = check(dev_eng, C, None)
    assert got[:3] == dev_eng.stage_motion_regions(now, ref, W, H, THR, **p) and got[3] == 0
    assert check(dev_eng, C, np.zeros((gh, gw), bool)) == got   # ... and so is a mask that ignores nothing
    G = np.where(np.random.default_rng(gw).random((gh, gw)) < 0.1, 3, 0).astype(np.uint8)
    held = check_hold(dev_eng, C, None, G)
    plain = dev_eng.stage_motion_hold(now, ref, G, W, H, THR, 2, **p)
    assert held[:5] == plain[:5] and (held[5] == plain[5]).all() and held[6] == 0


def test_a_changed_ignored_cell_gets_no_hold_and_an_aged_one_stays_active(dev_eng):
    gh, gw = 9, 65
    changed_ignored, aged_ignored, both, free = 63, 64, 130, 200
    C = bits(gh, gw, [changed_ignored, both, free])
    M = bits(gh, gw, [changed_ignored, aged_ignored, both])
    G = np.zeros((gh, gw), np.uint8)
    G.ravel()[aged_ignored], G.ravel()[both] = 3, 1
    got = check_hold(dev_eng, C, M, G, hold=7, **TIGHT)
    out = got[5].ravel()
    assert out[changed_ignored] == 0                            # age 0, not hold
    assert out[aged_ignored] == 2 and out[both] == 0            # an ignored cell with G > 0 decays ...
    assert out[free] == 7
    assert got[3:5] == (3, 2) and got[6] == 2                   # ... and is active: `free` changed, the two aged cells are held
    assert sorted(got[0]) == sorted([(16 * (i % gw), 16 * (i // gw), 16, 16) for i in (aged_ignored, both, free)])


@pytest.mark.parametrize("gh,gw", SHAPES)
def test_active_and_held_counts_under_seeded_ages(dev_eng, gh, gw):
    rng = np.random.default_rng(7 * gh + gw)
    C, M = rng.random((gh, gw)) < 0.1, rng.random((gh, gw)) < 0.4
    G = np.where(rng.random((gh, gw)) < 0.1, rng.integers(1, 256, (gh, gw)), 0).astype(np.uint8)
    got = check_hold(dev_eng, C, M, G, hold=5, W=16 * gw - 5, H=16 * gh - 11)
    A = (C & ~M) | (G > 0)
    assert got[3] == int(A.sum()) and got[4] == int((A & ~(C & ~M)).sum()) and got[6] == int((C & M).sum())


@pytest.mark.parametrize("gh,gw", SHAPES)
def test_with_a_hold_no_reference_and_a_mask_the_ages_alone_make_regions(dev_eng, gh, gw):
    G = np.zeros((gh, gw), np.uint8)
    G[gh // 2, gw // 2], G[gh - 1, gw - 1] = 4, 1
    C = np.ones((gh, gw), bool)                                  # sums that WOULD be changes against a reference of zeros
    got = check_hold(dev_eng, C, np.ones((gh, gw), bool), G, ref=False, **TIGHT)
    assert got[6] == 0 and got[3] == got[4] == int((G > 0).sum()) and len(got[0]) == got[2] == int((G > 0).sum())
    assert check(dev_eng, C, np.ones((gh, gw), bool), ref=False) == ([], [], 0, 0)      # without a hold: no reference, nothing at all


def test_refused_arguments(dev_eng):
    now = np.zeros((23, 40), np.uint16)
    with pytest.raises(ValueError):
        dev_eng.stage_motion_ignore(now, now, np.zeros((23, 41), np.uint8), 640, 360, 5)
    with pytest.raises(ValueError):
        dev_eng.stage_motion_ignore(now, now, None, 640, 360, 5, hold=256)
    with pytest.raises(ValueError):
        dev_eng.stage_motion_ignore(now, now, None, 640, 360, 5, age=np.zeros((23, 40), np.uint8))
