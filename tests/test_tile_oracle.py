"""Tiled detection without a GPU: known answers of the merge restated in tests/tile_oracle.py (tests/test_gpu_tiled.py runs the same
cases through the kernel), `tile_grid`, the plugin's `tiles` option and the binding of the new entry points."""
import os
import re

import numpy as np
import pytest

import tile_oracle as to
from watsor_amd import _lib
from watsor_amd.runtime import ROW_DTYPE, tile_grid

ORIGIN = (0, 0, 320, 240)


def rows_of(dets):
    """ROW_DTYPE[100]: the given (label, confidence, (x_min, y_min, x_max, y_max)) first, the engine's padding rows behind them."""
    rows = np.zeros(100, ROW_DTYPE)
    rows[:] = to.padding_row()
    for i, (label, conf, box) in enumerate(dets):
        rows[i]["label"], rows[i]["confidence"] = label, conf
        rows[i]["x_min"], rows[i]["y_min"], rows[i]["x_max"], rows[i]["y_max"] = box
    return rows


def found(rows):
    """[(label, confidence, box)] of the rows in front of the padding"""
    return [(int(r["label"]), float(r["confidence"]), (int(r["x_min"]), int(r["y_min"]), int(r["x_max"]), int(r["y_max"])))
            for r in rows if r["confidence"] != 0 or r["label"] != 1]


def distinct_rows(n_tiles, per_tile):
    """n_tiles * per_tile candidates that overlap nowhere (10 x 10 boxes on a 12-pixel lattice), every confidence different"""
    tiles, rows, k = [], [], 0
    for t in range(n_tiles):
        dets = []
        for _ in range(per_tile):
            x, y = 12 * (k % 26), 12 * (k // 26)
            dets.append((1 + k % 3, 0.1 + 0.005 * ((k * 37) % 151), (x, y, x + 10, y + 10)))
            k += 1
        tiles.append(ORIGIN)
        rows.append(rows_of(dets))
    return tiles, np.stack(rows)


# name -> (tiles, tile rows, iou, ios, expected (label, confidence, box) list or None).  Shared with tests/test_gpu_tiled.py.
def known_cases():
    box = (10, 20, 110, 220)
    c = {}
    c["same_box_higher_confidence_wins"] = ([(0, 0, 200, 240), (100, 0, 220, 240)],
                                            np.stack([rows_of([(3, 0.6, (110, 20, 210, 220))]), rows_of([(3, 0.8, box)])]), 0.6, 1.0,
                                            [(3, 0.8, (110, 20, 210, 220))])
    c["equal_confidence_lower_tile_stays"] = ([(0, 0, 200, 240), (100, 0, 220, 240)],
                                              np.stack([rows_of([(3, 0.5, (112, 20, 210, 220))]), rows_of([(3, 0.5, box)])]), 0.6, 1.0,
                                              [(3, 0.5, (112, 20, 210, 220))])
    c["different_labels_both_stay"] = ([ORIGIN, ORIGIN], np.stack([rows_of([(3, 0.6, box)]), rows_of([(4, 0.8, box)])]), 0.6, 1.0,
                                       [(4, 0.8, box), (3, 0.6, box)])
    half, whole = (10, 20, 60, 220), (10, 20, 110, 220)
    c["half_box_goes_with_ios"] = ([ORIGIN, ORIGIN], np.stack([rows_of([(1, 0.7, half)]), rows_of([(1, 0.9, whole)])]), 0.6, 0.5,
                                   [(1, 0.9, whole)])
    c["half_box_stays_without_ios"] = ([ORIGIN, ORIGIN], np.stack([rows_of([(1, 0.7, half)]), rows_of([(1, 0.9, whole)])]), 0.6, 1.0,
                                       [(1, 0.9, whole), (1, 0.7, half)])
    flat = [(2, 0.9, (50, 50, 50, 90)), (2, 0.8, (50, 50, 50, 90)), (2, 0.7, (40, 40, 100, 100)), (2, 0.6, (60, 70, 90, 70))]
    c["zero_area_boxes"] = ([ORIGIN], rows_of(flat)[None], 0.0, 0.0, flat)
    tiles, rows = distinct_rows(2, 75)
    c["150_candidates_keep_100"] = (tiles, rows, 0.6, 0.5, None)
    c["no_candidate"] = ([ORIGIN, (5, 5, 100, 100)], np.stack([rows_of([]), rows_of([])]), 0.6, 0.5, [])
    tiles, rows = distinct_rows(1, 40)
    c["identity"] = (tiles, rows, 1.0, 1.0, None)
    return c


KNOWN = known_cases()


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_merge_known_answers(name):
    tiles, rows, iou, ios, want = KNOWN[name]
    out = to.merge_tiles(tiles, rows, iou, ios)
    assert out.shape == (100,) and not out["zones"].any() and not out["_pad"].any()
    if want is not None:
        assert found(out) == want
        assert out[len(want):].tobytes() == rows_of([])[len(want):].tobytes()


def test_merge_keeps_100_of_150_in_confidence_order():
    tiles, rows, iou, ios, _ = KNOWN["150_candidates_keep_100"]
    out = to.merge_tiles(tiles, rows, iou, ios)
    conf = np.sort(rows["confidence"].reshape(-1))[::-1]
    assert (rows["confidence"] > 0).sum() == 150 and len(set(conf[:150])) == 150
    np.testing.assert_array_equal(out["confidence"], conf[:100])
    assert (np.diff(out["confidence"]) < 0).all()


def test_merge_identity_returns_the_rows():
    tiles, rows, iou, ios, _ = KNOWN["identity"]
    order = np.argsort(-rows[0]["confidence"], kind="stable")
    assert to.merge_tiles(tiles, rows, iou, ios).tobytes() == rows[0][order].tobytes()
    # ... and a threshold of 1 is off even for identical boxes
    twice = np.stack([rows_of([(1, 0.5, (1, 1, 9, 9))]), rows_of([(1, 0.5, (1, 1, 9, 9))])])
    assert len(found(to.merge_tiles([ORIGIN, ORIGIN], twice, 1.0, 1.0))) == 2
    assert len(found(to.merge_tiles([ORIGIN, ORIGIN], twice, 0.99, 1.0))) == 1


def test_merge_skips_what_is_no_candidate_and_shifts_without_clamping():
    rows = rows_of([(1, float("nan"), (1, 1, 5, 5)), (0, 0.9, (1, 1, 5, 5)), (2, -0.5, (1, 1, 5, 5)), (2, 0.4, (-7, 300, 400, 310))])
    out = to.merge_tiles([(30, 40, 100, 100)], rows[None], 0.6, 0.5)
    assert found(out) == [(2, 0.4, (23, 340, 430, 350))]


@pytest.mark.parametrize("size,grid,overlap", [((1920, 1080), (3, 2), 0.2), ((320, 240), (2, 2), 0.25), ((37, 23), (4, 3), 0.0),
                                               ((101, 77), (5, 1), 0.5), ((640, 480), (1, 1), 0.3)])
@pytest.mark.parametrize("even", [False, True])
def test_tile_grid_covers_the_frame(size, grid, overlap, even):
    w, h = size
    if even:
        w, h = w & ~1, h & ~1
    rects = tile_grid(w, h, grid[0], grid[1], overlap, full_frame=False, even=even)
    seen = np.zeros((h, w), np.int32)
    for x0, y0, tw, th in rects:
        assert x0 >= 0 and y0 >= 0 and tw >= 1 and th >= 1 and x0 + tw <= w and y0 + th <= h
        if even:
            assert not (x0 | y0 | tw | th) & 1
        seen[y0:y0 + th, x0:x0 + tw] += 1
    assert len(rects) <= grid[0] * grid[1] and seen.min() >= 1
    if overlap == 0:
        assert seen.max() == 1                                          # disjoint
    elif len(rects) > 1:
        assert seen.max() > 1
    with_full = tile_grid(w, h, grid[0], grid[1], overlap, even=even)
    assert with_full[-1] == (0, 0, w, h) and with_full[:len(rects)] == rects[:len(with_full)]


def test_tile_grid_edge_cases():
    assert tile_grid(37, 23, 1, 1, full_frame=False) == [(0, 0, 37, 23)]
    assert tile_grid(37, 23, 1, 1) == [(0, 0, 37, 23)]                 # (the whole frame is not listed twice)
    assert len(tile_grid(1920, 1080, 3, 2, 0.2)) == 7
    assert tile_grid(4, 4, 2, 2) == [(0, 0, 2, 2), (2, 0, 2, 2), (0, 2, 2, 2), (2, 2, 2, 2), (0, 0, 4, 4)]
    for bad in [(0, 10, 1, 1), (10, 10, 0, 1), (10, 10, 1, 1, 1.0), (10, 10, 1, 1, -0.1)]:
        with pytest.raises(ValueError):
            tile_grid(*bad)


@pytest.mark.parametrize("bad", [
    {"grid": [2, 2], "rects": [[0, 0, 1, 1]]}, {}, {"grid": [2]}, {"grid": [0, 2]}, {"grid": [2, 2.5]}, {"grid": [2, 2], "overlap": 1.0},
    {"grid": [2, 2], "overlap": "a"}, {"grid": [2, 2], "full_frame": 1}, {"grid": [2, 2], "iou": -0.1}, {"grid": [2, 2], "ios": float("nan")},
    {"grid": [2, 2], "colour": 1}, {"rects": []}, {"rects": [[0, 0, 0, 5]]}, {"rects": [[-1, 0, 5, 5]]}, {"rects": [[0, 0, 5]]},
    {"rects": [[0, 0, 5, 5]], "overlap": 0.1}, {"grid": [9, 8]}, {"cam": {"grid": [2]}}, {"cam": 5}, "grid", 7])
def test_bad_tiles_options_raise(bad):
    from watsor_amd.detection.hip_gpu import tile_options
    with pytest.raises(ValueError):
        tile_options({"tiles": bad})


def test_tiles_options_parse(tmp_path):
    from watsor_amd.detection.hip_gpu import HipObjectDetector, tile_options
    assert tile_options({}) == (None, {})
    spec, per = tile_options({"tiles": {"grid": [3, 2], "overlap": 0.2, "ios": 0.6}})
    assert per == {} and spec["grid"] == (3, 2) and spec["full_frame"] is True and spec["count"] == 7 and spec["iou"] is None and spec["ios"] == 0.6
    spec, per = tile_options({"tiles": {"porch": {"rects": [[0, 0, 64, 48], [10, 10, 20, 20]]}, "yard": {"grid": [1, 1]}}})
    assert spec is None and per["porch"]["count"] == 2 and per["yard"]["count"] == 1
    # more tiles per frame than max_batch: refused when the detector is constructed, before any engine exists
    (tmp_path / "mi355x.bin").write_bytes(b"")
    with pytest.raises(ValueError, match="max_batch"):
        HipObjectDetector(str(tmp_path), 0, {"tiles": {"grid": [3, 3]}, "numa": False}, max_batch=8)


def test_binding_declares_the_new_functions_with_the_headers_arity():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "watsor_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, table in [("wz_detect_tiled", _lib.SIGNATURES), ("wz_submit_tiled_device", _lib.SIGNATURES), ("wz_nms_iou", _lib.SIGNATURES),
                        ("wz_stage_crop_tile", _lib.DEV_SIGNATURES), ("wz_stage_merge_tiles", _lib.DEV_SIGNATURES)]:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m, name
        assert len(table[name][1]) == len(m.group(1).split(",")), name
    assert re.search(r"#define\s+WZ_MAX_TILES\s+%d\b" % _lib.WZ_MAX_TILES, header)
    assert getattr(_lib.load(), "wz_detect_tiled") and getattr(_lib.load(dev=True), "wz_stage_merge_tiles")


def test_batched_worker_takes_the_synchronous_path_for_a_tiled_detector():
    """neither the frame table nor submit_host has a tiled form: a detector that says `tiled` is driven through detect_batch()"""
    import shm_standins as shm
    from test_worker_logic import TableDetector, Worker, drive, first_row, setup

    class Tiled(TableDetector):
        tiled = True

        def submit_host(self, lane, images, cameras=None):
            raise AssertionError("the asynchronous path detects untiled")

        def bind_frame_table(self, frame_buffers, ids):
            raise AssertionError("the frame table detects untiled")

    _, cams = setup()
    det, w = Tiled(), Worker()
    drive(w, det, cams, [[shm.Payload("cam%d" % c, i) for c in range(3)] for i in range(2)], hip_metric_interval=0)
    assert [e for e in det.log if e[0] == "sync"] == [("sync", 3), ("sync", 3)]
    assert all(first_row(cams["cam%d" % c].frames[i]) == (1 + 10 * c + i, c) for c in range(3) for i in range(2))
