"""The case list of the resize sweep (tests/resize_cases.py) covers what it is there to cover -- asserted on the CPU through the
restated plan (tests/resize_plan.py), every class naming the cases that satisfy it, so that an edit of the list that loses a class
fails here and not silently on the GPU -- and the list has the POWER to tell a wrong row-staged kernel from a right one: the numpy
emulation of its data path (tests/resize_emulation.py) equals oracle.preprocess bit for bit on the cases, and every planted fault
changes the output of at least one of them.  No GPU: DESIGN.md section 14e."""
import numpy as np
import pytest

import resize_cases as rc
import resize_emulation as em
import resize_plan as rp
from resize_plan import BGR24, GRAY8, I420, NV12, P010, RGB24, UYVY422, YUV420P10, YUYV422

RULES = (False, True)                                               # legacy, half-pixel
FAMILIES = {"4:2:0": (NV12, I420), "4:2:2": (YUYV422, UYVY422), "10-bit": (P010, YUV420P10)}
ROWS = [c for c in rc.CASES if c.R is not None]                     # the cases of engines that keep the row-staged kernel


def base(c):
    return c.fmt & rp.BASE_MASK


def having(pred, cases=ROWS, what=""):
    """ids of the cases that satisfy `pred`; at least one, or the class `what` is lost"""
    ids = [rc.case_id(c) for c in cases if pred(c)]
    assert ids, "no case of the list covers: " + what
    return ids


def test_the_list_claims_what_the_plan_says():
    """R, the last workgroup's rows and the staging trips written beside every case are the plan's, under both rules (the issue's
    starting sizes among them: every R it lists is the R of the restated kernel); nothing overruns its budget; 10-bit cases pass
    the host's LDS rule, so the row-staged kernel does run them."""
    for c in ROWS:
        for hp in RULES:
            p = rc.case_plan(c, hp)
            assert (p.R, p.workgroups[-1].nrows, rp.trips(p)) == rc.listed(c, hp), (rc.case_id(c), hp)
            assert rp.lds_used(p) <= p.budget and rp.need(p.R, c.w, c.h, c.fmt) <= p.budget, rc.case_id(c)
            assert rp.rows_fit(c.w, c.fmt, p.budget), rc.case_id(c)
        mw, mh, _ = rc.ENGINES[c.engine]
        assert c.w <= mw and c.h <= mh and 3 * c.w * c.h <= 3 * mw * mh, rc.case_id(c)
    assert rc.budget("std") == 40 * 1024 and rc.budget("wide") == 54272


@pytest.mark.parametrize("R", range(1, 9))
def test_every_row_count_on_rgb24(R):
    having(lambda c: base(c) == RGB24 and c.R == R, what="RGB24 at R = %d" % R)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("R", range(2, 8))
def test_budget_limited_row_counts_on_every_format_family(family, R):
    """R = 2 .. 7: the LDS budget, not WZ_PRE_ROWS_MAX, ends the loop -- need(R + 1) is what did not fit"""
    ids = having(lambda c: base(c) in FAMILIES[family] and c.R == R, what="%s at R = %d" % (family, R))
    for c in ROWS:
        if rc.case_id(c) in ids:
            assert rp.need(R, c.w, c.h, c.fmt) <= rc.budget(c.engine) < rp.need(R + 1, c.w, c.h, c.fmt)


def test_divisors_and_tails():
    for R in range(2, 7):
        assert rp.SIZE % R == 0
        having(lambda c: c.R == R and c.last == R, what="300 %% R == 0 at R = %d" % R)
    having(lambda c: c.R == 7 and c.last == 6 and len(rc.case_plan(c).workgroups) == 43, what="the R = 7 tail: a last workgroup of 6 rows")
    having(lambda c: c.R == 8 and c.last == 4, what="the R = 8 tail")
    for family, fmts in FAMILIES.items():
        having(lambda c: base(c) in fmts and c.R == 7 and c.last == 6, what="the R = 7 tail on " + family)


@pytest.mark.parametrize("trips", (1, 2, 3))
def test_staging_trips(trips):
    for hp in RULES:
        having(lambda c: rc.listed(c, hp)[2] == trips, what="%d staging trips" % trips)
    if trips == 3:                                                  # only above the 40 KiB floor
        assert all(rc.budget(c.engine) > rp.LDS_FLOOR for c in ROWS if 3 in (rc.listed(c, False)[2], rc.listed(c, True)[2]))
        having(lambda c: c.trips == 3 and base(c) in (NV12, I420), what="three trips with chroma runs")


def test_the_scale_two_switch():
    """599 stages a span (R > 1); at 600 the scale is exactly 2.0f and at 601 above it: two adjacent rows, R = 1"""
    assert rp.scale(600) == np.float32(2.0) and rp.scale(599) < np.float32(2.0) < rp.scale(601)
    for width, what in ((lambda c: c.w <= 16, "narrow"), (lambda c: c.w >= 1600, "wide")):
        having(lambda c: base(c) == RGB24 and width(c) and c.h == 599 and c.R > 1, what=what + " x 599")
        having(lambda c: base(c) == RGB24 and width(c) and c.h == 600 and c.R == 1, what=what + " x 600")
        having(lambda c: base(c) == RGB24 and width(c) and c.h == 601 and c.R == 1, what=what + " x 601")
    for c in ROWS:
        if c.h >= 600:
            assert c.R == 1, rc.case_id(c)
    having(lambda c: base(c) in (NV12, I420) and c.h == 598 and c.R > 1 and c.w <= 16, what="4:2:0 below the switch")
    having(lambda c: base(c) in (NV12, I420) and c.h == 600 and c.R == 1 and c.w <= 16, what="4:2:0 at the switch")


def _batch_plans(hp):
    return [(f, rp.plan(f.w, f.h, f.fmt, rc.budget("std"), hp, f.residue)) for b in rc.BATCHES for f in b]


def test_run_alignment():
    """sh0 takes all 16 residues over the list; sh1 and sh2 take all 16 over the planar cases.  (A staged frame starts on a 16-byte
    boundary, where NV12's and the 10-bit formats' chroma rows -- an even number of bytes -- only reach even residues: the odd ones
    come from I420 with an odd chroma row, and from the batches' frames at odd device addresses.)"""
    for hp in RULES:
        plans = [(c.fmt, rc.case_plan(c, hp)) for c in ROWS] + [(f.fmt, p) for f, p in _batch_plans(hp)]
        planar = [(fmt, p) for fmt, p in plans if p.layout.planar]
        assert set().union(*(rp.residues(p, 0) for _, p in plans)) == set(range(16))
        assert set().union(*(rp.residues(p, 1) for _, p in planar)) == set(range(16))
        assert set().union(*(rp.residues(p, 2) for _, p in planar)) == set(range(16))
        assert all(not rp.residues(p, 2) for _, p in planar if not p.layout.two_planes)
        # in ONE frame, so that a kernel that is right for a single residue cannot pass: RGB24's run 0, I420's chroma runs
        having(lambda c: base(c) == RGB24 and rp.residues(rc.case_plan(c, hp), 0) == set(range(16)), what="one RGB24 frame with 16 sh0")
        having(lambda c: base(c) == I420 and rp.residues(rc.case_plan(c, hp), 1) == rp.residues(rc.case_plan(c, hp), 2) == set(range(16)),
               what="one I420 frame with 16 sh1 and sh2")
        # the batches bring run 0 above the 9 residues that staged frames had reached, and odd chroma residues to every planar format
        batch = _batch_plans(hp)
        for fmts in ((NV12,), (P010, YUV420P10)):
            assert any(r & 1 for f, p in batch if f.fmt & rp.BASE_MASK in fmts for r in rp.residues(p, 1)), fmts


def test_small_and_lopsided_frames():
    sides = (1, 2, 3, 299)
    for fmt in (RGB24, BGR24, GRAY8):                                # any side
        for s in (1, 3):
            having(lambda c: base(c) == fmt and c.w == s, what="%s %d wide" % (rp.NAMES[fmt], s))
            having(lambda c: base(c) == fmt and c.h == s, what="%s %d high" % (rp.NAMES[fmt], s))
    for s in sides:
        having(lambda c: base(c) == RGB24 and c.w == s, what="RGB24 %d wide" % s)
        having(lambda c: base(c) == RGB24 and c.h == s, what="RGB24 %d high" % s)
    for fmt in (NV12, I420, P010, YUV420P10):                        # even sides
        having(lambda c: base(c) == fmt and (c.w, c.h) == (2, 2), what="%s 2 x 2" % rp.NAMES[fmt])
    for fmts in FAMILIES.values():
        having(lambda c: base(c) in fmts and c.w == 2 and c.h >= 1200, what="2 x 1200 on %s" % (fmts,))
    for s in (1, 3, 299):                                            # 4:2:2: even width, any height
        having(lambda c: base(c) in (YUYV422, UYVY422) and c.h == s, what="4:2:2 %d high" % s)
    having(lambda c: base(c) in (YUYV422, UYVY422) and c.w == 2, what="4:2:2 one macropixel wide")
    having(lambda c: c.w >= 2560 and c.h <= 2, what="2560 x 2")
    having(lambda c: c.w <= 2 and c.h >= 1200, what="2 x 1200")
    having(lambda c: (c.w, c.h) == (300, 300), what="identity")


def test_half_pixel_coordinates():
    """A first source coordinate below zero on each axis (fl = -1, lo clamped, the weight from the unclamped floor) -- only the
    half-pixel rule on an up-scale has one --, taps exactly on a sample and taps between two, on each axis, on more formats than RGB24"""
    assert rc.first_coordinate(150, True) < 0 <= rc.first_coordinate(150, False)
    for fmts in ((RGB24,),) + tuple(FAMILIES.values()):
        having(lambda c: base(c) in fmts and rc.first_coordinate(c.h, True) < 0 and np.floor(rc.first_coordinate(c.h, True)) == -1,
               what="negative first row on %s" % (fmts,))
        having(lambda c: base(c) in fmts and rc.first_coordinate(c.w, True) < 0, what="negative first column on %s" % (fmts,))
        having(lambda c: base(c) in fmts and 1 < c.h < 300 and 1 < c.w < 300, what="an up-scale on both axes with weights on %s" % (fmts,))
    for hp in RULES:
        for axis in ("w", "h"):
            having(lambda c: min(rc.integer_taps(getattr(c, axis), hp)) > 0 and c.w > 3 and c.h > 3,
                   what="taps on and between samples along %s, half_pixel=%s" % (axis, hp))
            having(lambda c: rc.integer_taps(getattr(c, axis), hp)[0] == rp.SIZE and getattr(c, axis) > 300,
                   what="every tap on a sample on a down-scale along %s, half_pixel=%s" % (axis, hp))
            having(lambda c: rc.integer_taps(getattr(c, axis), hp)[0] == (0 if hp else 1) and getattr(c, axis) > 3,   # (legacy: output 0 is sample 0)
                   what="no tap but the origin on a sample along %s, half_pixel=%s" % (axis, hp))


def test_per_pixel_kernel_tails():
    """the byte-wise tail behind the 12-byte load at every residue of the frame's byte count mod 4, and the 4-byte load of a 4:2:2
    frame's last macropixel -- taken by output pixels of the case, not just present in the frame"""
    for hp in RULES:
        for r in range(4):
            having(lambda c: base(c) in (RGB24, BGR24) and (3 * c.w * c.h) % 4 == r and c.w * c.h > 16
                   and rc.pixel_kernel_tail_taps(c.w, c.h, hp) > 0, rc.CASES, "RGB24 tail at %d bytes mod 4, half_pixel=%s" % (r, hp))
        having(lambda c: base(c) in (RGB24, BGR24) and c.w * c.h > 16 and rc.pixel_kernel_tail_taps(c.w, c.h, hp) == 0, rc.CASES,
               "an RGB24 frame whose tail no tap reaches")
        for fmt in (YUYV422, UYVY422):
            having(lambda c: base(c) == fmt and c.w > 2 and rc.pixel_kernel_last_macropixel_taps(c.w, c.h, hp) > 0, rc.CASES,
                   "%s last macropixel" % rp.NAMES[fmt])


def test_the_60_kib_limit():
    keeps, loses = rc.LIMIT_KEEPS, rc.LIMIT_LOSES
    assert loses == keeps + 1
    assert rp.wz_preprocess_rows_lds(keeps) <= rp.LDS_LIMIT < rp.wz_preprocess_rows_lds(loses)
    assert rp.engine_keeps_rows_kernel(keeps) and not rp.engine_keeps_rows_kernel(loses)
    assert all(rp.engine_keeps_rows_kernel(rc.ENGINES[e][0]) for e in ("std", "wide"))
    for engine, width in (("limit_keeps", keeps), ("limit_loses", loses)):
        assert rc.ENGINES[engine][0] == width
        having(lambda c: c.engine == engine and c.w == width, rc.CASES, "a frame as wide as the engine takes on " + engine)
        having(lambda c: c.engine == engine and c.w < 1000, rc.CASES, "a narrow frame on " + engine)
    assert all((c.R is None) == (c.engine == "limit_loses") for c in rc.CASES)
    # the widest frame of the engine that keeps the kernel stages more than any other engine's launch holds: three trips
    having(lambda c: c.engine == "limit_keeps" and c.trips == 3 and rp.lds_used(rc.case_plan(c)) > rc.budget("wide"), what="LDS above every other budget")


def test_mixed_batches():
    mw, mh, mb = rc.ENGINES["std"]
    assert set(f.residue for b in rc.BATCHES for f in b) == set(range(16))
    rgb_mod4 = {f.residue % 4 for b in rc.BATCHES for f in b if f.fmt == RGB24}
    assert {1, 2, 3} <= rgb_mod4
    for b in rc.BATCHES:
        assert len(b) == 8 == mb and len({f.R for f in b}) >= 6 and {1, 2, 3, 5, 7, 8} <= {f.R for f in b}
        assert len({f.fmt & rp.BASE_MASK for f in b}) >= 4
        assert len({f.residue for f in b}) == 8
        for f in b:
            assert f.w <= mw and f.h <= mh
            for hp in RULES:
                assert rp.plan(f.w, f.h, f.fmt, rc.budget("std"), hp, f.residue).R == f.R, f
    assert {f.fmt & rp.BASE_MASK for b in rc.BATCHES for f in b} == {RGB24, BGR24, GRAY8, NV12, I420, YUYV422, UYVY422, P010, YUV420P10}


# ---- power ----------------------------------------------------------------------------------------------------------------------------
# The emulation's cases: a subset of the list that keeps this file to a few seconds -- every R, every format, the tails, the switch,
# three trips, the tiny frames; the cases left out repeat these classes at more bytes.  WITNESSES: the cases the faults are planted on.
EMULATED_IDS = """rgb24-2560x480-std rgb24-1920x540-std rgb24-1000x500-std rgb24-1919x301-std bgr24-1280x480-std nv12-2408x350-std i420-200-2406x300-std
    yuyv422-2560x216-std uyvy422-2560x250-std gray-2560x598-std p010-2560x150-std yuv420p10-100-2560x100-std p010-200-2560x76-std
    yuv420p10-2560x50-std p010-2560x44-std yuv420p10-3392x60-wide rgb24-6000x4-wide rgb24-6816x3-limit_keeps nv12-6816x4-limit_keeps
    rgb24-16x599-std rgb24-16x600-std rgb24-16x601-std nv12-16x598-std nv12-16x600-std rgb24-1x1-std rgb24-2x3-std rgb24-299x299-std
    rgb24-301x298-std rgb24-322x242-std rgb24-150x100-std rgb24-2x1200-std nv12-2x2-std nv12-298x300-std i420-322x242-std
    yuyv422-2x1-std uyvy422-322x242-std p010-2x2-std p010-322x242-std yuv420p10-200-322x242-std bgr24-299x3-std gray-3x299-std""".split()
WITNESS_IDS = """rgb24-1920x540-std rgb24-1000x500-std nv12-2408x350-std i420-200-2406x300-std p010-2560x44-std yuv420p10-100-2560x100-std
    yuyv422-2560x216-std nv12-16x598-std i420-322x242-std p010-322x242-std rgb24-322x242-std""".split()
BY_ID = {rc.case_id(c): c for c in ROWS}
EMULATED = [BY_ID[i] for i in EMULATED_IDS]                         # (a KeyError: the list lost a case the power check stands on)
assert set(WITNESS_IDS) <= set(EMULATED_IDS)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def emulated():
    """{case id: (case, frame, expected legacy, expected half-pixel)}"""
    out = {}
    for c in EMULATED:
        f, rgb = rc.random_frame(c.fmt, c.w, c.h)
        out[rc.case_id(c)] = (c, f, em.expected(rgb, False), em.expected(rgb, True))
    return out


def test_the_emulated_subset_keeps_every_row_count_and_family():
    for R in range(1, 9):
        having(lambda c: c.R == R, EMULATED, "R = %d in the emulated subset" % R)
    for fmt in rp.NAMES:
        having(lambda c: base(c) == fmt, EMULATED, rp.NAMES[fmt] + " in the emulated subset")
    having(lambda c: c.trips == 3, EMULATED, "three trips in the emulated subset")


def test_emulation_without_a_fault_is_the_oracle_bit_for_bit(emulated):
    """... so the plan's spans hold every tap the oracle takes, on every emulated case under both rules, at the staged address and (the
    witnesses) at an odd one"""
    for name, (c, f, legacy, half) in emulated.items():
        for hp, want in ((False, legacy), (True, half)):
            for address in (0, 5) if name in WITNESS_IDS and not hp else (0,):
                got = em.rows_kernel(f, c.w, c.h, c.fmt, rc.budget(c.engine), hp, address)
                assert np.array_equal(_bits(got), _bits(want)), (name, hp, address)


@pytest.mark.parametrize("fault", em.FAULTS)
def test_every_planted_fault_changes_some_cases_output(emulated, fault):
    caught = []
    for name in WITNESS_IDS:
        c, f, legacy, _ = emulated[name]
        got = em.rows_kernel(f, c.w, c.h, c.fmt, rc.budget(c.engine), False, 0, faults={fault})
        if not np.array_equal(_bits(got), _bits(legacy)):
            caught.append(name)
    assert caught, "no case of the list would notice the fault " + fault
    print(fault, "changes", len(caught), "of", len(WITNESS_IDS), "witnesses:", ", ".join(caught))
    if fault in ("cy1_short", "sh1_ignored"):                       # chroma faults: on both chroma layouts, 8 and 10 bit
        for fmts in ((NV12, P010), (I420, YUV420P10)):
            assert any(emulated[n][0].fmt & rp.BASE_MASK in fmts for n in caught), (fault, fmts)
    if fault == "need_short":                                       # seen only where the budget ends the loop
        assert all(2 <= emulated[n][0].R <= 7 for n in caught)
