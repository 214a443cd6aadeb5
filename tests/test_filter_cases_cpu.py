"""The filter edge cases and their numpy reference, proved without a GPU (tests/filter_cases.py):
`lattice_verdict` equals the literal oracle wherever both apply, the builders are deterministic and their counts are pinned, the
answers that hold by construction hold, and a reference with each seeded defect fails at least one case set."""
import numpy as np
import pytest

import filter_cases as fc
from oracle import zones as oz


def both(cfg, alpha, rows):
    """(literal, lattice) verdicts of the same rows."""
    return fc.literal_verdict(fc.literal_filters(cfg, alpha), rows), fc.lattice_verdict(fc.Camera.from_config(cfg, alpha), rows)


def assert_same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_sweep_counts_are_pinned():
    boxes = fc.sweep_boxes()
    assert len(boxes) == len(set(boxes)) == fc.SWEEP_BOXES == 43460
    assert -(-len(boxes) // fc.CALL_ROWS) == 435
    fill = oz.zone_fill(fc.sweep_alpha())
    assert tuple(int(f.sum()) for f in fill) == fc.SWEEP_ZONE_POINTS == (9, 43, 3)
    assert fill[1][5, 6] == 1 and fc.sweep_alpha()[5, 6] == 0                       # the hole belongs to its zone
    assert fill[0][0, 0] and fill[2][0, 12] and fill[1][10, 12]                     # zones in three frame corners
    want_pass, want_zones, hits = fc.sweep_expected()
    assert hits == fc.SWEEP_ZONE_HITS == (11358, 30731, 7759)
    for h in hits:
        assert 0.1 * len(boxes) < h < 0.9 * len(boxes)
    assert 0 < int(want_pass.sum()) < len(boxes)


def test_lattice_rule_equals_the_literal_oracle_on_the_sweep():
    want_pass, want_zones, _ = fc.sweep_expected()
    got = fc.lattice_verdict(fc.Camera.from_config(fc.sweep_config(), fc.sweep_alpha()), fc.sweep_rows())
    assert_same(got, (want_pass, want_zones))
    # every (box, zone) pair, not only the zones a row's label allows: the clamped box holds a lattice point of the polygon
    fill = oz.zone_fill(fc.sweep_alpha())
    for z, n in enumerate(fc.SWEEP_ZONE_HITS):
        hit = 0
        for x0, y0, x1, y1 in fc.sweep_boxes():
            xa, xb, ya, yb = max(min(x0, x1), 0), min(max(x0, x1), fc.SWEEP_W - 1), max(min(y0, y1), 0), min(max(y0, y1), fc.SWEEP_H - 1)
            hit += int(xa <= xb and ya <= yb and fill[z, ya:yb + 1, xa:xb + 1].any())
        assert hit == n


def test_lattice_rule_equals_the_literal_oracle_on_cap_threshold_and_wild_rows():
    rows, want_zones = fc.cap_rows()
    lit, lat = both(fc.cap_config(), fc.cap_alpha(), rows)
    assert_same(lit, lat)
    np.testing.assert_array_equal(lit[1], want_zones)                                # ... and both give the zones built in
    np.testing.assert_array_equal(lit[0], want_zones.any(1))
    for alpha in (None, fc.edge_alpha()):
        for cfg, (rows, groups) in ((fc.threshold_config(), fc.threshold_rows()), (fc.wild_config(), fc.wild_rows())):
            lit, lat = both(cfg, alpha, rows)
            assert_same(lit, lat)
            for name, idx in groups.items():
                if alpha is None and name.startswith("mask"):
                    continue
                assert 0 < int(lit[0][idx].sum()) < len(idx), name
            if alpha is None:
                assert not lit[1].any()
            else:
                assert not lit[1][lit[0] == 0].any() and lit[1][lit[0] == 1, 0].all()   # zones only on rows that reached the mask


def test_threshold_rows_known_answers():
    rows, groups = fc.threshold_rows()
    got, _ = fc.literal_verdict(fc.literal_filters(fc.threshold_config()), rows)
    want = {"confidence 50": [0, 1, 1], "confidence 30": [0, 1, 1], "confidence 0": [1, 1, 0, 1, 0, 0],
            "confidence 50, not finite": [0, 1, 0, 0, 0], "area 100": [1, 0, 1, 0, 1], "area 0": [1, 1, 0, 0],
            "both extents negative": [1, 0, 0], "one extent negative": [1, 0, 1, 0], "area 10000": [1, 0, 0, 0, 0, 1, 1],
            "labels": [0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0]}
    for name, w in want.items():
        assert got[groups[name]].tolist() == w, name
    t = float(np.float32(0.3))
    assert t > 30 / 100 > float(np.nextafter(np.float32(0.3), np.float32(0)))          # float32(0.3) lies ABOVE the double 30 / 100


def test_wild_rows_known_answers():
    rows, groups = fc.wild_rows()
    got, _ = fc.literal_verdict(fc.literal_filters(fc.wild_config()), rows)
    i = groups["area 100"][0]                                                         # (INT32_MIN, 0, INT32_MAX, 0): 2^32 x 1 pixels
    assert tuple(int(rows[i][k]) for k in ("x_min", "y_min", "x_max", "y_max")) == (fc.I32_MIN, 0, fc.I32_MAX, 0)
    assert got[i] == 1 and got[groups["area 10000"][0]] == 1
    assert fc.lattice_verdict(fc.Camera.from_config(fc.wild_config()), rows, "extent32")[0][i] == 0


def test_builders_are_deterministic():
    for build in (fc.sweep_rows, lambda: fc.cap_rows()[0], lambda: fc.threshold_rows()[0], lambda: fc.wild_rows()[0],
                  lambda: fc.plane_stride_case()[1]):
        assert build().tobytes() == build().tobytes()
    for W, H in fc.TABLE_SHAPES:
        for build in (fc.single_pixel_case, fc.seeded_plane_case):
            a, b = build(W, H), build(W, H)
            assert a[0].fill.tobytes() == b[0].fill.tobytes() and a[1].tobytes() == b[1].tobytes()
    assert fc.threshold_rows()[0]["zones"].any() == fc.threshold_rows()[0]["_pad"].any() == False   # noqa: E712


@pytest.mark.parametrize("wh", fc.TABLE_SHAPES)
def test_table_cases_hold_by_construction(wh):
    W, H = wh
    cam, rows, hit = fc.single_pixel_case(W, H)
    assert cam.fill.reshape(len(cam.fill), -1).sum(1).tolist() == [1] * len(cam.fill)
    got_pass, got_zones = fc.lattice_verdict(cam, rows)
    np.testing.assert_array_equal(got_pass, hit)
    np.testing.assert_array_equal(got_zones[:, 0], np.where(hit, rows["label"], 0))  # label k is allowed zone k alone
    assert not got_zones[:, 1:].any() and hit.any() and (W * H == 1 or not hit.all())
    cam, rows = fc.seeded_plane_case(W, H)
    got_pass, _ = fc.lattice_verdict(cam, rows)
    brute = [bool(cam.fill[0, r["y_min"]:r["y_max"] + 1, r["x_min"]:r["x_max"] + 1].any()) for r in rows]
    np.testing.assert_array_equal(got_pass, brute)
    if W * H > 771:
        thin = (rows["x_min"] == rows["x_max"]) | (rows["y_min"] == rows["y_max"])
        assert len(rows) == 2000 and thin.sum() >= 500 and 200 < got_pass.sum() < 1800
    else:
        assert len(rows) == W * H and got_pass.sum() == cam.fill.sum()
    for value in (2, 255):
        other, same_rows = fc.seeded_plane_case(W, H, value)
        assert same_rows.tobytes() == rows.tobytes() and set(np.unique(other.fill)) <= {0, value}
        np.testing.assert_array_equal(fc.lattice_verdict(other, rows)[0], got_pass)


def test_plane_stride_and_large_corner_cases():
    cam, rows, zones = fc.plane_stride_case()
    got = fc.lattice_verdict(cam, rows)
    np.testing.assert_array_equal(got[1], zones)
    np.testing.assert_array_equal(got[0], zones.any(1))
    W, H = 64, 48                                                                       # the large case's builder on a small frame
    cam, rows = fc.corners_case(W, H)
    got_pass, _ = fc.lattice_verdict(cam, rows)
    brute = []
    for r in rows:
        xa, xb, ya, yb = max(r["x_min"], 0), min(r["x_max"], W - 1), max(r["y_min"], 0), min(r["y_max"], H - 1)
        brute.append(bool(xa <= xb and ya <= yb and cam.fill[0, ya:yb + 1, xa:xb + 1].any()))
    np.testing.assert_array_equal(got_pass, brute)
    assert 0 < got_pass.sum() < len(rows) and len(rows) <= fc.CALL_ROWS
    assert (fc.LARGE_SHAPE[0] + 1) * (fc.LARGE_SHAPE[1] + 1) * 4 > 33e6                 # one 33 MB table


def case_sets():
    """name -> (camera, rows): everything the GPU module runs against a reference."""
    sets = {"sweep": (fc.Camera.from_config(fc.sweep_config(), fc.sweep_alpha()), fc.sweep_rows()),
            "cap": (fc.Camera.from_config(fc.cap_config(), fc.cap_alpha()), fc.cap_rows()[0]),
            "thresholds": (fc.Camera.from_config(fc.threshold_config(), fc.edge_alpha()), fc.threshold_rows()[0]),
            "wild": (fc.Camera.from_config(fc.wild_config()), fc.wild_rows()[0]),
            "wild, masked": (fc.Camera.from_config(fc.wild_config(), fc.edge_alpha()), fc.wild_rows()[0]),
            "planes": fc.plane_stride_case()[:2]}
    for W, H in fc.TABLE_SHAPES:
        sets["pixels %dx%d" % (W, H)] = fc.single_pixel_case(W, H)[:2]
        sets["seeded %dx%d" % (W, H)] = fc.seeded_plane_case(W, H)
    return sets


@pytest.fixture(scope="module")
def expected():
    return {name: (cam, rows, fc.lattice_verdict(cam, rows)) for name, (cam, rows) in case_sets().items()}


# where each seeded defect must show at the least (it may show elsewhere too)
SEEN_BY = {"lookup": ("sweep", "pixels 1x1", "pixels 257x3", "pixels 3x257", "seeded 513x258"),
           "row0": ("sweep", "pixels 2x1", "pixels 256x3", "seeded 257x3"),
           "noclamp": ("sweep", "wild, masked"),
           "cap9": ("cap", "planes"),
           "gt": ("thresholds",),
           "extent32": ("wild", "wild, masked")}


@pytest.mark.parametrize("defect", fc.DEFECTS)
def test_each_seeded_defect_is_caught(expected, defect):
    caught = []
    for name, (cam, rows, want) in expected.items():
        got = fc.lattice_verdict(cam, rows, defect)
        if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
            caught.append(name)
    for name in SEEN_BY[defect]:
        assert name in caught, (defect, name, caught)
