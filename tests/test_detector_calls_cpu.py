"""The detector plugin's engine calls (watsor_amd/detection/hip_gpu.py) against tests/golden/detector_calls.json: every scenario of
tests/detector_calls.py is replayed under the recording stand-in for `HipEngine` and must make the recorded calls with the recorded
arguments in the recorded order, return what was returned, note the same `bound_descriptions` and raise the same exceptions with the
same text.  No GPU needed."""
import json

import pytest

import detector_calls as dc


@pytest.fixture(scope="module")
def golden():
    with open(dc.PATH) as f:
        return json.load(f)["scenarios"]


def test_the_golden_holds_the_scenarios(golden):
    assert sorted(golden) == sorted(dc.SCENARIOS)


@pytest.mark.parametrize("name", list(dc.SCENARIOS))
def test_the_plugin_makes_the_recorded_calls(name, golden, monkeypatch):
    from watsor_amd.detection import hip_gpu
    monkeypatch.setattr(hip_gpu, "HipEngine", dc.RecordingEngine)
    steps = dc.record(name, hip_gpu)
    assert [s["step"] for s in steps] == [s["step"] for s in golden[name]]
    for got, want in zip(steps, golden[name]):
        assert got == want, "%s, step %r" % (name, got["step"])
    if name == "A mixed":
        # what the docstring of the motion set-up states in words: the table's bind configures each camera once, and the synchronous
        # batch behind it -- the worker's retry of a refused piece -- finds every layout current and sets no camera again
        by_step = {s["step"]: [c[0] for c in s["calls"]] for s in steps}
        assert [n for n in by_step["bind_tiled_frame_table"] if n.startswith("set_camera_")] == \
            ["set_camera_tiles", "set_camera_ignore", "set_camera_motion", "set_camera_motion_hold", "set_camera_ignore"]
        assert by_step["detect_batch after the bind"] == ["detect_motion", "detect_batch", "detect_gated", "detect_tiled"]
        assert not [n for n in by_step["detect_batch after the bind"] if n.startswith("set_camera_")]
    if name == "E plain":
        by_step = {s["step"]: s["calls"] for s in steps}
        assert [c[0] for c in by_step["detect"]] == ["detect_batch"] and by_step["detect"][0][1][4] is None      # formats=None
        assert [c[0] for c in by_step["bind_frame_table"]] == ["bind_frames"]
