"""The plugin option `motion` (watsor_amd/detection/hip_gpu.py: motion_options / check_motion_options; no GPU needed)."""
import pytest

from watsor_amd.detection.hip_gpu import check_motion_options, motion_options, tile_options

RECTS = [[0, 0, 64, 48], [32, 16, 64, 48]]
FULL = {"threshold": 12, "min_cells": 2, "dilate": 2, "max_regions": 16, "min_side": 16, "pad": 64, "whole_frame": False, "iou": 0.5, "ios": 0.6}


def test_defaults_and_every_key():
    spec, by_name = motion_options({"motion": {"threshold": 8}})
    assert not by_name
    assert spec == {"threshold": 8, "min_cells": 1, "dilate": 1, "max_regions": 3, "min_side": 300, "pad": 8, "whole_frame": True,
                    "iou": None, "ios": None, "count": 4}
    spec, _ = motion_options({"motion": FULL})
    assert spec == dict(FULL, count=16)
    for thr in (0, 255):
        assert motion_options({"motion": {"threshold": thr}})[0]["threshold"] == thr
    assert motion_options({"motion": {"threshold": 1, "dilate": 0, "pad": 0, "max_regions": 1}})[0]["count"] == 2
    assert motion_options({}) == (None, {}) and motion_options({"motion": None}) == (None, {})


def test_per_camera():
    spec, by_name = motion_options({"motion": {"porch": {"threshold": 4, "whole_frame": False}, "yard": {"threshold": 9, "max_regions": 5}}})
    assert spec is None and sorted(by_name) == ["porch", "yard"]
    assert by_name["porch"]["count"] == 3 and by_name["yard"]["count"] == 6 and by_name["yard"]["whole_frame"] is True


@pytest.mark.parametrize("bad", [
    8, "8", [8], True, {},                                                       # not a description / no threshold
    {"min_cells": 1},
    {"threshold": 8.0}, {"threshold": "8"}, {"threshold": True}, {"threshold": None}, {"threshold": -1}, {"threshold": 256},
    {"threshold": 8, "min_cells": 0}, {"threshold": 8, "min_cells": 1.5},
    {"threshold": 8, "dilate": -1}, {"threshold": 8, "dilate": 3}, {"threshold": 8, "dilate": "1"},
    {"threshold": 8, "max_regions": 0}, {"threshold": 8, "max_regions": 17}, {"threshold": 8, "max_regions": 2.0},
    {"threshold": 8, "min_side": 15}, {"threshold": 8, "min_side": None},
    {"threshold": 8, "pad": -1}, {"threshold": 8, "pad": 65},
    {"threshold": 8, "whole_frame": 1}, {"threshold": 8, "whole_frame": "yes"},
    {"threshold": 8, "iou": -0.1}, {"threshold": 8, "ios": "0.5"}, {"threshold": 8, "iou": float("nan")},
    {"threshold": 8, "max_age": 2}, {"threshold": 8, "grid": [2, 2]}, {"threshold": 8, "pixel_thr": 8},
])
def test_bad_settings_are_refused_and_the_message_names_the_option(bad):
    with pytest.raises(ValueError, match="^motion"):
        motion_options({"motion": bad})
    if isinstance(bad, dict):
        with pytest.raises(ValueError, match=r"^motion\['porch'\]"):
            motion_options({"motion": {"porch": bad}})


def test_motion_is_no_key_of_tiles():
    with pytest.raises(ValueError, match="unknown key"):
        tile_options({"tiles": {"rects": RECTS, "motion": {"threshold": 8}}})


def both(options, max_batch=8):
    m, t = motion_options(options), tile_options(options)
    check_motion_options(m[0], m[1], t[0], t[1], max_batch)


def test_motion_and_tiles_of_one_camera_are_refused():
    both({"motion": {"porch": {"threshold": 8}}, "tiles": {"yard": {"rects": RECTS}}})          # two cameras: fine
    both({"motion": {"threshold": 8}})
    with pytest.raises(ValueError, match=r"^motion\['porch'\].*tiles"):
        both({"motion": {"porch": {"threshold": 8}}, "tiles": {"porch": {"rects": RECTS}}})
    with pytest.raises(ValueError, match="^motion: .*tiles"):
        both({"motion": {"threshold": 8}, "tiles": {"porch": {"rects": RECTS}}})
    with pytest.raises(ValueError, match="^motion: .*tiles"):
        both({"motion": {"threshold": 8}, "tiles": {"rects": RECTS}})
    with pytest.raises(ValueError, match=r"^motion\['porch'\].*tiles"):
        both({"motion": {"porch": {"threshold": 8}}, "tiles": {"grid": [2, 1]}})


def test_configured_tiles_must_fit_max_batch():
    both({"motion": {"threshold": 8, "max_regions": 7}}, max_batch=8)
    with pytest.raises(ValueError, match="^motion: .*max_batch 8"):
        both({"motion": {"threshold": 8, "max_regions": 8}}, max_batch=8)
    both({"motion": {"threshold": 8, "max_regions": 8, "whole_frame": False}}, max_batch=8)
    with pytest.raises(ValueError, match=r"^motion\['yard'\].*max_batch 2"):
        both({"motion": {"porch": {"threshold": 8, "max_regions": 1}, "yard": {"threshold": 8, "max_regions": 2}}}, max_batch=2)


def test_batched_worker_takes_the_synchronous_path_for_a_motion_detector():
    """neither the frame table nor submit_host has a form for motion regions: a detector that says `motion` is driven through
    detect_batch(), with the frames' camera ids"""
    import shm_standins as shm
    from test_worker_logic import TableDetector, Worker, drive, first_row, setup

    class Moving(TableDetector):
        motion = True

        def submit_host(self, lane, images, cameras=None):
            raise AssertionError("the asynchronous path detects untiled")

        def bind_frame_table(self, frame_buffers, ids):
            raise AssertionError("the frame table detects untiled")

    _, cams = setup()
    det, w = Moving(), Worker()
    drive(w, det, cams, [[shm.Payload("cam%d" % c, i) for c in range(3)] for i in range(2)], hip_metric_interval=0)
    assert [e for e in det.log if e[0] == "sync"] == [("sync", 3), ("sync", 3)]
    assert all(first_row(cams["cam%d" % c].frames[i]) == (1 + 10 * c + i, c) for c in range(3) for i in range(2))
