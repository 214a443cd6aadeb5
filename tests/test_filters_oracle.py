"""Filter oracle + host-side zone extraction, pinned by the reference's known-answer tests
(watsor/test/test_filter.py:14-74), by fixtures generated from the reference's own classes
(tests/golden/make_filter_golden.py) and by the zone statistics of the reference's porch.png."""
import json
import os

import numpy as np
import pytest
from PIL import Image, ImageDraw

from oracle import filters as of
from oracle import zones as oz
from watsor_amd.runtime import zones_from_alpha
from watsor_amd.share import BoundingBox, Detection

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def det(label, confidence, box=(0, 0, 0, 0)):
    return Detection(label=label, confidence=confidence, bounding_box=BoundingBox(*box))


# ---- known-answer tests restated from watsor/test/test_filter.py -----------------------------------
def test_confidence_kat():                      # test_filter.py:14-22
    f = of.ConfidenceFilter({'detect': [{'person': {'confidence': 50}}]})
    assert f(det(1, 0.70)) and not f(det(1, 0.40)) and not f(det(2, 0.70))


def test_area_kat():                            # test_filter.py:24-36
    f = of.AreaFilter({'width': 100, 'height': 100, 'detect': [{'person': {'area': 50}}]})
    assert f(det(1, 0.7, (0, 0, 100, 50)))
    assert not f(det(1, 0.7, (0, 0, 50, 50)))
    assert not f(det(2, 0.7, (0, 0, 100, 50)))


def kat_alpha():
    """test_filter.py:51-55: 100x100 RGBA, alpha = rectangle (50,0)-(100,100) filled with 255."""
    with Image.new("L", (100, 100)) as alpha:
        ImageDraw.Draw(alpha).rectangle((50, 0, alpha.width, alpha.height), fill=255)
        return np.array(alpha)


def test_mask_kat(tmp_path):                    # test_filter.py:38-74
    with pytest.raises(AssertionError, match="Error reading mask file"):
        of.MaskFilter({'width': 1, 'height': 1, 'mask': 'notafile.png', 'detect': []})
    p = str(tmp_path / "m.png")
    Image.new('RGB', (10, 10)).save(p)
    with pytest.raises(AssertionError, match="Mask image .+ is not of 32 bit color"):
        of.MaskFilter({'width': 10, 'height': 10, 'mask': p, 'detect': []})
    img = Image.new('RGBA', (100, 100))
    img.putalpha(Image.fromarray(kat_alpha()))
    img.save(p)
    with pytest.raises(AssertionError, match="The size of mask image .+ doesn't match"):
        of.MaskFilter({'width': 50, 'height': 50, 'mask': p, 'detect': []})
    f = of.MaskFilter({'width': 100, 'height': 100, 'mask': p, 'detect': []})
    assert not f(det(1, 0.7, (20, 20, 40, 80)))
    d = det(1, 0.7, (20, 20, 80, 80))
    assert f(d) and d.zones[0] == 1


def test_product_mask_reader_raises_like_the_reference(tmp_path):
    from watsor_amd.filter.hip_filter import read_mask_alpha
    with pytest.raises(AssertionError, match="Error reading mask file"):
        read_mask_alpha('notafile.png', 1, 1)
    p = str(tmp_path / "m.png")
    Image.new('RGB', (10, 10)).save(p)
    with pytest.raises(AssertionError, match="Mask image .+ is not of 32 bit color"):
        read_mask_alpha(p, 10, 10)
    Image.new('RGBA', (100, 100)).save(p)
    with pytest.raises(AssertionError, match="The size of mask image .+ doesn't match"):
        read_mask_alpha(p, 50, 50)


# ---- fixtures generated from the reference's own ConfidenceFilter / AreaFilter ------------------------
def test_confidence_area_match_reference_fixture():
    g = json.load(open(os.path.join(GOLDEN, "filters.json")))
    cf, af = of.ConfidenceFilter(g["config"]), of.AreaFilter(g["config"])
    assert len(g["rows"]) == 400
    for r in g["rows"]:
        d = det(r["label"], r["confidence"], r["box"])
        assert cf(d) == r["conf_pass"] and af(d) == r["area_pass"], r
    assert 30 < sum(r["conf_pass"] for r in g["rows"]) < 370


def test_coco_table_and_filters_against_reference():
    """The reference's COCO table and its ConfidenceFilter / AreaFilter verdicts on 300 seeded detections, as recorded from its
    sources (tests/golden/make_reference_golden.py)."""
    from watsor_amd.coco import COCO_CLASSES
    ref = json.load(open(os.path.join(GOLDEN, "reference_layout.json")))
    assert ref["coco_classes"] == list(COCO_CLASSES)
    cfg = json.load(open(os.path.join(GOLDEN, "filters.json")))["config"]
    b, d = of.ConfidenceFilter(cfg), of.AreaFilter(cfg)
    rng = np.random.default_rng(5)
    assert len(ref["filter_cases"]) == 300
    for r in ref["filter_cases"]:
        x0, y0 = int(rng.integers(0, 600)), int(rng.integers(0, 440))      # the recorded cases are these seeded detections
        label, score = int(rng.choice([0, 1, 3, 8, 5])), float(np.float32(rng.random()))
        assert (r["label"], r["confidence"], r["box"]) == (label, score, [x0, y0, int(rng.integers(x0, 640)), int(rng.integers(y0, 480))])
        dd = det(r["label"], r["confidence"], r["box"])
        assert r["conf_pass"] == b(dd) and r["area_pass"] == d(dd), r


# ---- zones: host extraction (C++, raster) vs oracle (Python, polygons) -------------------------------
def porch_opaque():
    z = np.load(os.path.join(GOLDEN, "porch_zones.npz"))
    h, w = z["shape"]
    return np.unpackbits(z["opaque"])[:h * w].reshape(h, w).astype(bool), z["zone_pixels"]


def test_porch_zones_match_survey_statistics():
    opaque, pixels = porch_opaque()
    alpha = np.where(opaque, 255, 204).astype(np.uint8)
    fill, cent = zones_from_alpha(alpha)
    assert fill.shape == (2, 480, 640)
    assert fill.reshape(2, -1).sum(1).tolist() == pixels.tolist()          # 42 853 and 58 038 px
    assert abs(cent[0][0] - 132) <= 1 and abs(cent[0][1] - 377) <= 1      # centroids ~(132,377), ~(424,370)
    assert abs(cent[1][0] - 424) <= 1 and abs(cent[1][1] - 370) <= 1
    polys = oz.zone_polygons(alpha)
    assert len(polys) == 2
    for z, poly in enumerate(polys):
        m00, m10, m01 = oz.contour_moments(poly)
        assert (int(m10 / m00), int(m01 / m00)) == tuple(cent[z])


def random_blobs(rng, h, w, n):
    alpha = rng.integers(0, 255, (h, w)).astype(np.uint8)                  # anything but 255
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n):
        cy, cx = rng.integers(8, h - 8), rng.integers(8, w - 8)
        ry, rx = rng.integers(4, h // 4), rng.integers(4, w // 4)
        if rng.random() < 0.5:
            m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        else:
            m = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx)
        alpha[m] = 255
        if rng.random() < 0.5:                                             # punch a hole, maybe with an island
            hm = ((yy - cy) / max(ry // 2, 1)) ** 2 + ((xx - cx) / max(rx // 2, 1)) ** 2 <= 1
            alpha[hm] = 254
            if rng.random() < 0.5:
                alpha[cy, cx] = 255
    return alpha


@pytest.mark.parametrize("seed", range(6))
def test_zone_fill_equals_lattice_points_of_contour_polygons(seed):
    rng = np.random.default_rng(seed)
    alpha = random_blobs(rng, 60, 80, 3)
    fill, cent = zones_from_alpha(alpha)
    ofill = oz.zone_fill(alpha)                       # polygon interior by exact point-in-polygon
    assert fill.shape == ofill.shape
    np.testing.assert_array_equal(fill, ofill)
    for z, poly in enumerate(oz.zone_polygons(alpha)):
        m00, m10, m01 = oz.contour_moments(poly)
        assert (int(m10 / m00), int(m01 / m00)) == tuple(cent[z])


@pytest.mark.parametrize("seed", range(4))
def test_lattice_rule_equals_polygon_intersection(seed):
    """box polygon intersects zone polygon  <=>  a filled-zone pixel lies in the closed box."""
    rng = np.random.default_rng(100 + seed)
    alpha = random_blobs(rng, 48, 64, 3)
    fill, _ = zones_from_alpha(alpha)
    polys = oz.zone_polygons(alpha)
    for _ in range(400):
        x0, y0 = int(rng.integers(0, 64)), int(rng.integers(0, 48))
        x1, y1 = int(rng.integers(x0, 64)), int(rng.integers(y0, 48))
        if rng.random() < 0.15:
            x1 = x0                                   # degenerate boxes follow the lattice rule too
        for z, poly in enumerate(polys):
            assert oz.box_intersects_polygon(x0, y0, x1, y1, poly) == bool(fill[z, y0:y1 + 1, x0:x1 + 1].any())


def test_thin_zone_raises_zero_division_like_the_reference():
    alpha = np.zeros((20, 20), np.uint8)
    alpha[5, 3:12] = 255                               # 1-px line: contour polygon has zero area
    with pytest.raises(ZeroDivisionError):
        zones_from_alpha(alpha)
    with pytest.raises(ZeroDivisionError):
        oz.zone_polygons(alpha)


# ---- zones at the frame's edges, the zone limit and the order of equal keys ----------------------------------------------------
def assert_zones_match_oracle(alpha):
    """Fill, order and centroids of `zones_from_alpha` against the oracle's polygons; returns the product's (fill, centroids)."""
    fill, cent = zones_from_alpha(alpha)
    ofill = oz.zone_fill(alpha)
    assert fill.shape == ofill.shape
    np.testing.assert_array_equal(fill, ofill)
    for z, poly in enumerate(oz.zone_polygons(alpha)):
        m00, m10, m01 = oz.contour_moments(poly)
        assert (int(m10 / m00), int(m01 / m00)) == tuple(cent[z])
    return fill, cent


def blank(h, w):
    return np.full((h, w), 100, np.uint8)


def test_zones_in_all_four_frame_corners():
    alpha = blank(16, 20)
    alpha[:3, :3] = alpha[:3, -4:] = alpha[-2:, :3] = alpha[-3:, -3:] = 255
    fill, _ = assert_zones_match_oracle(alpha)
    assert fill.shape[0] == 4 and fill[0][0, 0] and fill[:, 0, 19].any() and fill[:, 15, 0].any() and fill[3][15, 19]
    assert sorted(int(f.sum()) for f in fill) == [6, 9, 9, 12]


def test_all_opaque_frame_and_two_by_two():
    for h, w in ((5, 7), (2, 2), (2, 9), (9, 2)):
        fill, cent = assert_zones_match_oracle(np.full((h, w), 255, np.uint8))
        assert fill.shape[0] == 1 and fill.all()
    assert tuple(cent[0]) == (0, 4)                                      # int(0.5), int(4.0)


def test_ring_along_the_border_with_an_island_is_one_zone():
    alpha = blank(10, 12)
    alpha[0, :] = alpha[-1, :] = alpha[:, 0] = alpha[:, -1] = 255
    alpha[4:6, 5:8] = 255                                                # nested in the ring's hole: RETR_EXTERNAL does not report it
    fill, _ = assert_zones_match_oracle(alpha)
    assert fill.shape[0] == 1 and fill.all()


def test_u_open_to_the_top_edge_is_not_filled():
    alpha = blank(9, 11)
    alpha[0:7, 2] = alpha[0:7, 8] = 255
    alpha[6, 2:9] = 255
    fill, _ = assert_zones_match_oracle(alpha)
    assert fill.shape[0] == 1 and int(fill.sum()) == 7 + 7 + 5 and not fill[0][3, 5]
    alpha[0, 2:9] = 255                                                  # closed: now the inside belongs to the zone
    fill, _ = assert_zones_match_oracle(alpha)
    assert fill.shape[0] == 1 and int(fill.sum()) == 7 * 7


def test_equal_keys_the_later_found_zone_first():
    alpha = blank(16, 16)
    alpha[2:5, 10:13] = 255                                              # centroid (11, 3), found first
    alpha[10:13, 2:5] = 255                                              # centroid (3, 11): the same key
    fill, cent = assert_zones_match_oracle(alpha)
    assert [tuple(c) for c in cent] == [(3, 11), (11, 3)] and fill[0][11, 3] and fill[1][3, 11]


def test_forty_zones_and_forty_one_refused():
    import filter_cases as fc
    fill, cent = assert_zones_match_oracle(fc.cap_alpha(40))
    assert fill.shape[0] == 40 and [tuple(c) for c in cent] == [(4 * k + 1, 4) for k in range(40)]
    assert len(oz.zone_polygons(fc.cap_alpha(41))) == 41
    with pytest.raises(ValueError):
        zones_from_alpha(fc.cap_alpha(41))


def test_ellipses_with_centres_on_the_border():
    h, w = 40, 56
    yy, xx = np.mgrid[0:h, 0:w]
    compared = touching = 0
    for seed in range(8):
        rng = np.random.default_rng(300 + seed)
        alpha = blank(h, w)
        for _ in range(4):
            cy, cx = int(rng.choice([0, h - 1, rng.integers(0, h)])), int(rng.choice([0, w - 1, rng.integers(0, w)]))
            ry, rx = int(rng.integers(2, h // 4)), int(rng.integers(2, w // 4))
            alpha[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = 255
        try:
            oz.zone_polygons(alpha)
        except ZeroDivisionError:                                        # a sliver of an ellipse: the reference raises, so must the product
            with pytest.raises(ZeroDivisionError):
                zones_from_alpha(alpha)
            continue
        fill, _ = assert_zones_match_oracle(alpha)
        compared += 1
        touching += int(fill[:, 0, :].any() or fill[:, -1, :].any() or fill[:, :, 0].any() or fill[:, :, -1].any())
    assert compared >= 6 and touching >= 6


def test_checkerboard_is_one_eight_connected_zone():
    yy, xx = np.mgrid[0:8, 0:10]
    alpha = np.where((yy + xx) % 2 == 0, 255, 100).astype(np.uint8)
    fill, _ = assert_zones_match_oracle(alpha)
    assert fill.shape[0] == 1
    inner = fill[0][1:-1, 1:-1]
    assert inner.all() and fill[0][alpha == 255].all() and not fill[0][0, 1] and not fill[0][1, 0]


def test_one_pixel_frame_and_diagonal_line_raise_zero_division():
    line = blank(12, 12)
    line[np.arange(2, 9), np.arange(2, 9)] = 255
    for alpha in (np.full((1, 1), 255, np.uint8), line):
        with pytest.raises(ZeroDivisionError):
            zones_from_alpha(alpha)
        with pytest.raises(ZeroDivisionError):
            oz.zone_polygons(alpha)
