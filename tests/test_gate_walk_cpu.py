"""What the activity kernel's long-row cases prove, shown without a GPU: tests/gate_walk.py restates how wz_k_tile_activity walks a row
(csrc/k_gate.hip) and can be told to make one of six mistakes.

  a. without a mistake it gives tests/gate_oracle.py's bytes on every case, old and new;
  b. the five mistakes that live in trips beyond a row's first 64 words are INVISIBLE on the old cases (tests/gate_cases.py: OLD) --
     which is the statement that the suite could not see them -- while the sixth, every row on row 0's head, was always caught;
  c. every mistake changes the bytes of at least one new case (NEW), the two carry mistakes on an RGB and on a BGR case;
  d. the new table reaches the paths DESIGN.md section 16 lists: these are conditions the table is built to meet, not measurements.

tests/test_gpu_gate_long_rows.py runs the same table through the kernel."""
import numpy as np
import pytest

import gate_cases as gc
import gate_oracle as go
import gate_walk as gw
from watsor_amd.runtime import FMT_BGR24, FMT_RGB24, FMT_YUV420P10


@pytest.fixture(scope="module")
def want():
    """the oracle's cell sums of every case, worked out once"""
    out = {}
    for case in gc.OLD + gc.NEW:
        frame, fmt = gc.oracle_view(case)
        out[case.name] = go.cell_sums(frame, case.w, case.h, fmt, case.rect)
    return out


@pytest.fixture(scope="module")
def walked():
    """(cell sums, census) of every case without a defect"""
    return {case.name: gw.walk(*gc.walk_args(case)) for case in gc.OLD + gc.NEW}


@pytest.fixture(scope="module")
def differs(want):
    """defect -> the names of the cases whose bytes it changes.  The carry defects touch three-byte pixels only: the other modes never
    read carry63, so they are walked on the RGB / BGR cases alone."""
    out = {}
    for defect in gw.DEFECTS:
        cases = [c for c in gc.OLD + gc.NEW if not defect.startswith("carry") or c.fmt in gc.THREE_BYTE]
        out[defect] = {c.name for c in cases if gw.walk(*gc.walk_args(c), defect=defect)[0].tobytes() != want[c.name].tobytes()}
    return out


def census_of(walked, cases):
    total = gw.new_census()
    for case in cases:
        gw.merge_census(total, walked[case.name][1])
    return total


# ---- a ------------------------------------------------------------------------------------------------------------------------------------
def test_names_are_unique_and_rectangles_lie_in_their_frames():
    names = [c.name for c in gc.OLD + gc.NEW]
    assert len(set(names)) == len(names)
    for c in gc.OLD + gc.NEW:
        x0, y0, tw, th = c.rect
        assert 0 <= x0 and 0 <= y0 and tw >= 1 and th >= 1 and x0 + tw <= c.w and y0 + th <= c.h, c.name
        if c.fmt in gc.EIGHT or c.fmt in gc.ONE_BYTE[1:]:
            assert (x0 | y0 | tw | th) & 1 == 0, c.name           # 4:2:0
        if c.fmt in gc.TWO_BYTE:
            assert (x0 | tw) & 1 == 0, c.name


@pytest.mark.parametrize("table", ["old", "new"])
def test_the_walk_is_the_oracle(want, walked, table):
    for case in gc.OLD if table == "old" else gc.NEW:
        got = walked[case.name][0]
        assert got.dtype == np.uint16 and got.shape == want[case.name].shape and got.tobytes() == want[case.name].tobytes(), case.name


# ---- b ------------------------------------------------------------------------------------------------------------------------------------
def test_no_old_row_is_longer_than_one_trip(walked):
    trips = census_of(walked, gc.OLD)["trips"]
    assert trips and max(t for t, _ in trips) == 1 and max(n for _, n in trips) < gw.LANES      # (not even a full first trip)


@pytest.mark.parametrize("defect", gw.BEYOND_FIRST_TRIP)
def test_the_old_cases_cannot_see_a_defect_beyond_the_first_trip(differs, defect):
    old = {c.name for c in gc.OLD}
    assert differs[defect] & old == set()


def test_the_old_cases_do_see_a_wrong_head(differs):
    """The one seeded defect that is not about long rows: 34-, 37-, 68- and 111-byte pitches give the rows of a rectangle different
    heads, and the old cases have always failed an engine that took row 0's for all of them."""
    assert differs["head_of_row0"] & {c.name for c in gc.OLD}


# ---- c ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", gw.DEFECTS)
def test_the_new_cases_see_every_defect(differs, defect):
    seen = [c for c in gc.NEW if c.name in differs[defect]]
    assert seen, defect
    if defect.startswith("carry"):
        assert any(c.fmt == FMT_RGB24 for c in seen) and any(c.fmt == FMT_BGR24 for c in seen)
    if defect in gw.BEYOND_FIRST_TRIP and not defect.startswith("carry"):
        for group in (gc.THREE_BYTE, gc.TWO_BYTE, gc.ONE_BYTE):                                # every byte-select path has its witness
            assert any(c.fmt in group for c in seen), (defect, group)


# ---- d ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", gc.THREE_BYTE, ids=["rgb", "bgr"])
def test_census_of_the_three_byte_cases(walked, fmt):
    cases = [c for c in gc.NEW if c.fmt == fmt]
    cen = census_of(walked, cases)
    trips = cen["trips"]
    assert (1, 64) in trips                       # one trip, and a full one
    assert (2, 1) in trips                        # a single word in the second trip
    assert (2, 64) in trips                       # two full trips
    assert any(t >= 3 for t, _ in trips)
    assert cen["e_at_trip"] == {0, 1, 2}          # the pixel at a trip boundary: whole, its last byte over, its last two bytes over
    assert cen["boundary_mod3"] == {0, 1, 2}      # byte 1024 s - head of the row, modulo 3
    assert cen["heads"] == set(range(16))
    assert any(len(walked[c.name][1]["heads"]) == 1 and max(t for t, _ in walked[c.name][1]["trips"]) >= 3 for c in cases)   # one head in every row
    assert any(walked[c.name][1]["heads"] == set(range(16)) for c in cases)                                                   # all sixteen in one case
    assert cen["two_cells"] and cen["last_cell_cut"] and cen["zero_sum_skipped"] and cen["ragged_first"] and cen["ragged_last"]


@pytest.mark.parametrize("fmt", gc.TWO_BYTE, ids=[gc.NAMES[f] for f in gc.TWO_BYTE])
def test_census_of_the_two_byte_cases(walked, fmt):
    cen = census_of(walked, [c for c in gc.NEW if c.fmt == fmt])
    assert min(t for t, _ in cen["trips"]) >= 2
    assert cen["multi_trip_head_parity"] == {0, 1}
    assert cen["low10_split_at_trip"] == (fmt == FMT_YUV420P10)
    assert cen["two_cells"] and cen["ragged_first"] and cen["ragged_last"]


@pytest.mark.parametrize("fmt", gc.ONE_BYTE, ids=[gc.NAMES[f] for f in gc.ONE_BYTE])
def test_census_of_the_one_byte_cases(walked, fmt):
    cen = census_of(walked, [c for c in gc.NEW if c.fmt == fmt])
    assert min(t for t, _ in cen["trips"]) >= 2
    assert cen["two_cells"] and cen["ragged_first"] and cen["ragged_last"]


def test_skews_and_fills_of_the_new_table(want):
    assert {c.skew for c in gc.NEW} == {0, 1, 2, 11}
    assert {c.fill for c in gc.NEW} == {"random", "ones", "zeros"}
    ones = [c for c in gc.NEW if c.fill == "ones"]
    assert {c.fmt for c in ones} >= set(gc.THREE_BYTE) and all(int(want[c.name].max()) == 255 * 256 for c in ones)      # 65280 fits the uint16
    assert all(not want[c.name].any() for c in gc.NEW if c.fill == "zeros")
    assert max(c.w * c.h for c in gc.NEW) <= 1090 * 34 and max(c.w for c in gc.NEW) <= 1090
