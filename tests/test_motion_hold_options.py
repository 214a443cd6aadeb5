"""The plugin option `motion_hold` (watsor_amd/detection/hip_gpu.py: motion_hold_options; no GPU needed)."""
import copy

import pytest

from watsor_amd.detection.hip_gpu import motion_hold_options, motion_options

MOTION = {"motion": {"threshold": 8}}
PER_CAMERA = {"motion": {"porch": {"threshold": 4, "whole_frame": False}, "yard": {"threshold": 9}}}


def hold(options):
    return motion_hold_options(options, *motion_options(options))


def test_the_option_and_its_defaults():
    assert hold(MOTION) == (None, {}) and hold(dict(MOTION, motion_hold=None)) == (None, {}) and hold({}) == (None, {})
    assert hold(dict(MOTION, motion_hold={"hold": 2})) == ({"hold": 2, "object_hold": 0}, {})
    assert hold(dict(MOTION, motion_hold={"object_hold": 255})) == ({"hold": 0, "object_hold": 255}, {})
    assert hold(dict(MOTION, motion_hold={"hold": 255, "object_hold": 1})) == ({"hold": 255, "object_hold": 1}, {})
    assert hold(dict(PER_CAMERA, motion_hold={"hold": 3})) == ({"hold": 3, "object_hold": 0}, {})      # every camera that has motion settings


def test_per_camera():
    spec, by_name = hold(dict(PER_CAMERA, motion_hold={"porch": {"hold": 4}, "yard": {"object_hold": 30, "hold": 1}}))
    assert spec is None and by_name == {"porch": {"hold": 4, "object_hold": 0}, "yard": {"hold": 1, "object_hold": 30}}
    assert hold(dict(PER_CAMERA, motion_hold={"yard": {"hold": 4}}))[1] == {"yard": {"hold": 4, "object_hold": 0}}
    assert hold(dict(MOTION, motion_hold={"porch": {"hold": 4}}))[1] == {"porch": {"hold": 4, "object_hold": 0}}      # motion is set for every camera


@pytest.mark.parametrize("bad", [
    8, "8", [2, 3], True, {},                                                    # not a description
    {"hold": 2, "max_age": 1}, {"hold": 2, "threshold": 8}, {"object": 3},       # unknown keys
    {"hold": 2.0}, {"hold": "2"}, {"hold": True}, {"hold": None}, {"hold": -1}, {"hold": 256},
    {"object_hold": 1.5}, {"object_hold": "3"}, {"object_hold": False}, {"object_hold": -1}, {"object_hold": 256}, {"hold": 2, "object_hold": 256},
    {"hold": 0, "object_hold": 0}, {"hold": 0}, {"object_hold": 0},              # both 0
])
def test_bad_settings_are_refused_and_the_message_names_the_option(bad):
    with pytest.raises(ValueError, match="^motion_hold"):
        hold(dict(MOTION, motion_hold=bad))
    if isinstance(bad, dict) and bad:
        with pytest.raises(ValueError, match=r"^motion_hold\['porch'\]"):
            hold(dict(PER_CAMERA, motion_hold={"porch": bad}))


def test_a_hold_needs_motion_settings():
    with pytest.raises(ValueError, match="^motion_hold: .*no motion option"):
        hold({"motion_hold": {"hold": 2}})
    with pytest.raises(ValueError, match=r"^motion_hold\['porch'\].*no motion option"):
        hold({"motion_hold": {"porch": {"hold": 2}}})
    with pytest.raises(ValueError, match=r"^motion_hold\['garage'\].*no motion option"):
        hold(dict(PER_CAMERA, motion_hold={"porch": {"hold": 2}, "garage": {"hold": 2}}))


def test_motion_hold_is_no_key_of_motion_and_leaves_its_settings_alone():
    with pytest.raises(ValueError, match="^motion: unknown key"):
        motion_options({"motion": {"threshold": 8, "hold": 2}})
    for base in (MOTION, PER_CAMERA):
        with_hold = dict(copy.deepcopy(base), motion_hold={"hold": 2, "object_hold": 3})
        assert motion_options(with_hold) == motion_options(base)
        hold(with_hold)
        assert with_hold == dict(base, motion_hold={"hold": 2, "object_hold": 3})      # (the options are read, not rewritten)
