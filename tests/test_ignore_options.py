"""The plugin option `ignore` (watsor_amd/detection/hip_gpu.py: ignore_options, check_ignore_cameras, ignore_plane; no GPU needed): its
three forms -- pixel rectangles, an (H, W) uint8 array, a mask file -- and every refusal text."""
import numpy as np
import pytest

from watsor_amd.detection.hip_gpu import check_ignore_cameras, ignore_options, ignore_plane, motion_options, tile_options

MOTION = {"motion": {"threshold": 8}}
PER_CAMERA = {"motion": {"porch": {"threshold": 4}}, "tiles": {"yard": {"grid": [2, 2], "gate": {"threshold": 6}}, "street": {"grid": [2, 2]}}}
CLOCK = [[16, 8, 48, 16]]


def ignore(options):
    return ignore_options(options, *motion_options(options), *tile_options(options))


def plane(options, name, w, h):
    return ignore_plane(ignore(options)[name], "ignore[%r]" % name, w, h)


def test_no_option_is_no_mask():
    assert ignore({}) == {} and ignore(MOTION) == {} and ignore(dict(MOTION, ignore=None)) == {}


def test_rectangles():
    opts = dict(MOTION, ignore={"porch": CLOCK, "yard": [[0, 0, 1, 1], (318, 238, 2, 2)]})
    assert ignore(opts) == {"porch": ("rects", [(16, 8, 48, 16)]), "yard": ("rects", [(0, 0, 1, 1), (318, 238, 2, 2)])}
    p = plane(opts, "porch", 320, 240)
    assert p.dtype == np.uint8 and p.shape == (240, 320) and p.sum() == 48 * 16 and p[8:24, 16:64].all()
    p = plane(opts, "yard", 320, 240)
    assert p.sum() == 5 and p[0, 0] and p[238:, 318:].all()      # the frame's last pixel is inside


def test_an_array():
    mask = np.zeros((240, 320), np.uint8)
    mask[100:120, 7:9] = 255
    opts = dict(PER_CAMERA, ignore={"yard": mask, "porch": mask[:, ::-1]})      # (a view is made contiguous)
    kind, kept = ignore(opts)["yard"]
    assert kind == "mask" and np.array_equal(kept, mask)
    assert np.array_equal(plane(opts, "yard", 320, 240), mask)
    got = plane(opts, "porch", 320, 240)
    assert got.flags["C_CONTIGUOUS"] and np.array_equal(got, mask[:, ::-1])


def test_a_mask_file_ignores_where_alpha_is_above_zero(tmp_path):
    from PIL import Image
    rgba = np.zeros((48, 64, 4), np.uint8)
    rgba[..., :3] = 90
    rgba[4:9, 10:20, 3] = 255
    rgba[30, 40, 3] = 1                             # (any alpha above zero)
    name = str(tmp_path / "porch.png")
    Image.fromarray(rgba, "RGBA").save(name)
    opts = dict(MOTION, ignore={"porch": name, "yard": tmp_path / "porch.png"})
    assert ignore(opts) == {"porch": ("file", name), "yard": ("file", name)}
    for cam in ("porch", "yard"):
        p = plane(opts, cam, 64, 48)
        assert p.dtype == np.uint8 and set(np.unique(p)) == {0, 1} and np.array_equal(p != 0, rgba[..., 3] > 0)
    with pytest.raises(ValueError, match=r"^ignore\['porch'\]: the mask is 64x48 \(width x height\) but the camera's frames are 320x240"):
        plane(opts, "porch", 320, 240)
    Image.fromarray(rgba[..., :3].copy(), "RGB").save(name)
    with pytest.raises(ValueError, match=r"^ignore\['porch'\]: Mask image .* is not of 32 bit color"):
        plane(opts, "porch", 64, 48)
    with pytest.raises(ValueError, match=r"^ignore\['porch'\]: Error reading mask file"):
        plane(dict(MOTION, ignore={"porch": str(tmp_path / "missing.png")}), "porch", 64, 48)


@pytest.mark.parametrize("bad", [8, "porch.png", CLOCK, True, {}, np.zeros((4, 4), np.uint8)])
def test_the_option_is_per_camera_name_only(bad):
    with pytest.raises(ValueError, match="^ignore: expected \\{camera name: "):
        ignore(dict(MOTION, ignore=bad))


@pytest.mark.parametrize("bad", [8, 1.5, True, [], (), {"rects": CLOCK}, None])
def test_what_is_none_of_the_three_forms_is_refused(bad):
    with pytest.raises(ValueError, match=r"^ignore\['porch'\]: expected a list of \[x, y, w, h\] pixel rectangles, an \(H, W\) uint8 array or the name of a mask file"):
        ignore(dict(MOTION, ignore={"porch": bad}))


@pytest.mark.parametrize("bad", [[16, 8, 48, 16], [[16, 8, 48]], [[16, 8, 48, 16, 1]], [[16, 8, 48, 16.0]], [[16, 8, 48, "16"]], [[True, 8, 48, 16]],
                                 [[-1, 8, 48, 16]], [[16, -1, 48, 16]], [[16, 8, 0, 16]], [[16, 8, 48, 0]], [[16, 8, 48, 16], [1, 2, 3]]])
def test_a_bad_rectangle_is_refused(bad):
    with pytest.raises(ValueError, match=r"^ignore\['porch'\]: rectangle .*expected \[x, y, w, h\]: whole numbers, x and y >= 0, w and h >= 1"):
        ignore(dict(MOTION, ignore={"porch": bad}))


@pytest.mark.parametrize("rect", [[273, 0, 48, 16], [0, 225, 48, 16], [320, 0, 1, 1], [0, 240, 1, 1], [0, 0, 321, 240]])
def test_a_rectangle_outside_the_frame_is_refused_when_the_frame_is_known(rect):
    opts = dict(MOTION, ignore={"porch": [CLOCK[0], rect]})
    with pytest.raises(ValueError, match=r"^ignore\['porch'\]: rectangle \[%d, %d, %d, %d\] does not lie inside the camera's 320x240 frame" % tuple(rect)):
        plane(opts, "porch", 320, 240)


@pytest.mark.parametrize("bad", [np.zeros((240, 320, 1), np.uint8), np.zeros(320, np.uint8), np.zeros((240, 320), np.int32),
                                 np.zeros((240, 320), bool), np.zeros((0, 320), np.uint8)])
def test_an_array_that_is_no_plane_is_refused(bad):
    with pytest.raises(ValueError, match=r"^ignore\['porch'\]: an array of shape .* expected \(H, W\) uint8"):
        ignore(dict(MOTION, ignore={"porch": bad}))


@pytest.mark.parametrize("shape", [(320, 240), (240, 319), (241, 320), (120, 160)])
def test_an_array_of_another_size_than_the_frames_is_refused(shape):
    opts = dict(MOTION, ignore={"porch": np.zeros(shape, np.uint8)})
    with pytest.raises(ValueError, match=r"^ignore\['porch'\]: the mask is %dx%d \(width x height\) but the camera's frames are 320x240" % shape[::-1]):
        plane(opts, "porch", 320, 240)


def test_a_camera_with_neither_motion_nor_a_gate_is_refused():
    text = r"^ignore\[%r\]: the camera has neither a motion option nor tiles with a gate"
    with pytest.raises(ValueError, match=text % "porch"):
        ignore({"ignore": {"porch": CLOCK}})
    with pytest.raises(ValueError, match=text % "street"):                      # tiles, but no gate: nothing looks for change
        ignore(dict(PER_CAMERA, ignore={"street": CLOCK}))
    with pytest.raises(ValueError, match=text % "garage"):
        ignore(dict(PER_CAMERA, ignore={"porch": CLOCK, "garage": CLOCK}))
    with pytest.raises(ValueError, match=text % "porch"):
        ignore({"tiles": {"grid": [2, 2]}, "ignore": {"porch": CLOCK}})
    assert set(ignore(dict(PER_CAMERA, ignore={"porch": CLOCK, "yard": CLOCK}))) == {"porch", "yard"}
    assert set(ignore({"tiles": {"grid": [2, 2], "gate": {"threshold": 3}}, "ignore": {"anything": CLOCK}})) == {"anything"}      # a gate for every camera


def test_an_unknown_camera_is_refused_once_the_cameras_are_known():
    by_name = ignore(dict(MOTION, ignore={"porch": CLOCK, "yard": CLOCK}))
    check_ignore_cameras(by_name, ["porch", "yard", "street"])
    check_ignore_cameras({}, [])
    with pytest.raises(ValueError, match=r"^ignore\['yard'\]: unknown camera, this detector's cameras are 'porch', 'street'"):
        check_ignore_cameras(by_name, ["porch", "street"])
    with pytest.raises(ValueError, match=r"^ignore\['porch'\]: unknown camera, this detector's cameras are none"):
        check_ignore_cameras(by_name, [])


def test_ignore_leaves_the_other_options_alone():
    opts = dict(PER_CAMERA, ignore={"porch": CLOCK})
    assert motion_options(opts) == motion_options(PER_CAMERA) and tile_options(opts) == tile_options(PER_CAMERA)
