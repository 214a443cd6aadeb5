"""The per-camera filters at zone, threshold and table edges: `wz_apply_filter`, `wz_k_filter_rows`,
`wz_k_sat_rows`, `wz_k_sat_cols` against known answers.  Every comparison is exact: pass bytes, zones[10] and every other byte of the
72-byte rows.  The cases and the numpy reference live in tests/filter_cases.py and are proved on the CPU
(tests/test_filter_cases_cpu.py).  A mask that goes through `HipCameraFilter` is held to the literal polygon oracle, raw fill planes
that go through `HipEngine.set_camera_filter` to `filter_cases.lattice_verdict`."""
import numpy as np
import pytest

import filter_cases as fc
from conftest import make_engine
from watsor_amd.filter.hip_filter import HipCameraFilter
from watsor_amd.runtime import ROW_DTYPE, zones_from_alpha
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(model_dir):
    e = make_engine(model_dir, max_batch=4)
    yield e
    e.close()


def run(eng, cam, rows):
    """`filter_rows` over all rows, 100 per call: (pass[n], rows as they came back)."""
    out_pass, out_rows = np.zeros(len(rows), np.uint8), np.zeros(len(rows), ROW_DTYPE)
    for start, chunk in fc.calls(rows):
        n = min(fc.CALL_ROWS, len(rows) - start)
        got = eng.filter_rows(cam, chunk)
        assert not got[n:].any() and chunk[n:].tobytes() == bytes(72 * (fc.CALL_ROWS - n))   # the padding: label 0, untouched
        out_pass[start:start + n], out_rows[start:start + n] = got[:n], chunk[:n]
    return out_pass, out_rows


def check(eng, cam, rows, want, what=""):
    """Pass bytes, zones and every other byte of the rows against (pass, zones) of a reference."""
    want_pass, want_zones = want
    got_pass, got_rows = run(eng, cam, rows)
    np.testing.assert_array_equal(got_pass, want_pass, err_msg=what)
    np.testing.assert_array_equal(got_rows["zones"], want_zones, err_msg=what)
    expect = rows.copy()
    expect["zones"] = want_zones
    assert got_rows.tobytes() == expect.tobytes(), what
    return got_pass, got_rows


def set_raw(eng, cam_id, cam):
    eng.set_camera_filter(cam_id, *cam.engine_args())


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def test_exhaustive_sweep_on_a_tiny_mask(eng):
    rows = fc.sweep_rows()
    want_pass, want_zones, hits = fc.sweep_expected()
    assert len(rows) == 43460 and len(list(fc.calls(rows))) == 435
    for h in hits:                                                    # every zone hit by > 10 % and missed by > 10 % of the boxes
        assert 0.1 * len(rows) < h < 0.9 * len(rows)
    flt = HipCameraFilter(eng, 3, fc.sweep_config(), alpha=fc.sweep_alpha())
    try:
        assert flt.num_zones == 3
        check(eng, 3, rows, (want_pass, want_zones))
    finally:
        flt.close()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", fc.TABLE_SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_tables_single_pixels(eng, wh):
    cam, rows, hit = fc.single_pixel_case(*wh)
    want = fc.lattice_verdict(cam, rows)
    np.testing.assert_array_equal(want[0], hit)
    set_raw(eng, 9, cam)
    try:
        check(eng, 9, rows, want)
    finally:
        eng.clear_camera_filter(9)


@pytest.mark.parametrize("wh", fc.TABLE_SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_tables_seeded_plane_and_fill_bytes(eng, wh):
    cam, rows = fc.seeded_plane_case(*wh)
    want = fc.lattice_verdict(cam, rows)
    assert wh[0] * wh[1] < 64 or 0 < want[0].sum() < len(rows)
    try:
        for value in (1, 2, 255):
            other, _ = fc.seeded_plane_case(*wh, value)
            assert other.fill.max() in (0, value)
            set_raw(eng, 9, other)
            check(eng, 9, rows, want, "fill byte %d" % value)
    finally:
        eng.clear_camera_filter(9)


def test_tables_largest_frame(eng):
    cam, rows = fc.corners_case(*fc.LARGE_SHAPE)
    want = fc.lattice_verdict(cam, rows)
    assert 0 < want[0].sum() < len(rows)
    set_raw(eng, 9, cam)
    try:
        check(eng, 9, rows, want)
    finally:
        eng.clear_camera_filter(9)


def test_tables_plane_stride_of_forty_zones(eng):
    cam, rows, zones = fc.plane_stride_case()
    want = fc.lattice_verdict(cam, rows)
    np.testing.assert_array_equal(want[1], zones)
    set_raw(eng, 9, cam)
    try:
        check(eng, 9, rows, want)
    finally:
        eng.clear_camera_filter(9)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_zone_cap_and_allow_lists(eng):
    alpha, cfg = fc.cap_alpha(), fc.cap_config()
    assert zones_from_alpha(alpha)[0].shape[0] == 40
    with pytest.raises(ValueError):
        zones_from_alpha(fc.cap_alpha(41))
    rows, zones = fc.cap_rows()
    want = fc.literal_verdict(fc.literal_filters(cfg, alpha), rows)
    np.testing.assert_array_equal(want[1], zones)
    flt = HipCameraFilter(eng, 3, cfg, alpha=alpha)
    try:
        assert flt.num_zones == 40
        check(eng, 3, rows, want)
    finally:
        flt.close()


# ---- 4, 5, 6 -------------------------------------------------------------------------------------------------------------------
EDGE_CASES = {"thresholds": (fc.threshold_config, fc.threshold_rows), "wild": (fc.wild_config, fc.wild_rows)}


@pytest.mark.parametrize("masked", [False, True], ids=["no mask", "mask"])
@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_thresholds_labels_and_wild_coordinates(eng, case, masked):
    cfg, (rows, groups) = EDGE_CASES[case][0](), EDGE_CASES[case][1]()
    alpha = fc.edge_alpha() if masked else None
    want = fc.literal_verdict(fc.literal_filters(cfg, alpha), rows)            # the oracle on Python integers
    for name, idx in groups.items():
        if masked or not name.startswith("mask"):
            assert 0 < int(want[0][idx].sum()) < len(idx), name
    flt = HipCameraFilter(eng, 3, cfg, alpha=alpha)
    try:
        assert flt.num_zones == (2 if masked else 0)
        check(eng, 3, rows, want)
    finally:
        flt.close()


@pytest.mark.parametrize("masked", [False, True], ids=["no mask", "mask"])
@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_drop_mode(eng, case, masked):
    cfg, (rows, _) = EDGE_CASES[case][0](), EDGE_CASES[case][1]()
    alpha = fc.edge_alpha() if masked else None
    want = fc.literal_verdict(fc.literal_filters(cfg, alpha), rows)
    keep_cam = HipCameraFilter(eng, 6, cfg, alpha=alpha)
    drop_cam = HipCameraFilter(eng, 7, cfg, alpha=alpha, drop=True)
    try:
        p_keep, r_keep = check(eng, 6, rows, want)
        p_drop, r_drop = run(eng, 7, rows)
        np.testing.assert_array_equal(p_drop, p_keep)
        keep = p_keep.astype(bool)
        assert keep.any() and not keep.all()
        assert r_drop[keep].tobytes() == r_keep[keep].tobytes()
        assert r_drop[~keep].tobytes() == bytes(72 * int((~keep).sum()))
    finally:
        keep_cam.close()
        drop_cam.close()


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_replacing_a_cameras_filter(eng):
    """Camera 3 goes through five states; cameras 2 and 4 keep their own filters throughout."""
    cap_rows, _ = fc.cap_rows()
    thr_rows, _ = fc.threshold_rows()
    neighbours = [(2, cap_rows, fc.literal_verdict(fc.literal_filters(fc.cap_config(), fc.cap_alpha()), cap_rows)),
                  (4, thr_rows, fc.literal_verdict(fc.literal_filters(fc.threshold_config(), fc.edge_alpha()), thr_rows))]
    wide, probes, _ = fc.single_pixel_case(257, 3)
    fixed = np.concatenate([fc.sweep_rows()[::870], probes[:50]])               # 50 boxes of the sweep, 50 probes of the wide frame
    assert len(fixed) == fc.CALL_ROWS
    flts = [HipCameraFilter(eng, 2, fc.cap_config(), alpha=fc.cap_alpha()),
            HipCameraFilter(eng, 4, fc.threshold_config(), alpha=fc.edge_alpha())]
    seen = []

    def step(what, want):
        seen.append(check(eng, 3, fixed, want, what)[0])
        for cam, rows, verdict in neighbours:
            check(eng, cam, rows, verdict, "camera %d after: %s" % (cam, what))

    try:
        flts.append(HipCameraFilter(eng, 3, fc.sweep_config(), alpha=fc.sweep_alpha()))
        step("13 x 11, three zones", fc.literal_verdict(fc.literal_filters(fc.sweep_config(), fc.sweep_alpha()), fixed))
        set_raw(eng, 3, wide)
        step("257 x 3, other zones", fc.lattice_verdict(wide, fixed))
        bare = fc.Camera.plain(257, 3)
        set_raw(eng, 3, bare)
        step("no mask", fc.lattice_verdict(bare, fixed))
        empty = fc.Camera.plain(257, 3, fill=np.zeros((0, 3, 257), np.uint8))
        set_raw(eng, 3, empty)
        step("a mask without zones", fc.lattice_verdict(empty, fixed))
        assert not seen[-1].any()
        eng.clear_camera_filter(3)
        step("cleared", ((fixed["label"] > 0).astype(np.uint8), np.zeros((len(fixed), fc.ROW_ZONES), np.int32)))
        for a, b in zip(seen, seen[1:]):                                        # every step changed what the rows get
            assert not np.array_equal(a, b)
        assert 0 < seen[0].sum() < len(fixed) and 0 < seen[1].sum() < len(fixed) and seen[2].all() and seen[4].all()
    finally:
        for f in flts:
            f.close()


def test_highest_camera_id(eng):
    cfg, alpha = fc.threshold_config(), fc.edge_alpha()
    rows, _ = fc.threshold_rows()
    flt = HipCameraFilter(eng, 255, cfg, alpha=alpha)
    try:
        check(eng, 255, rows, fc.literal_verdict(fc.literal_filters(cfg, alpha), rows))
    finally:
        flt.close()
    cam = fc.Camera.from_config(cfg)
    with pytest.raises(ValueError):
        set_raw(eng, 256, cam)
    with pytest.raises(ValueError):
        eng.filter_rows(256, np.zeros(fc.CALL_ROWS, ROW_DTYPE))
    with pytest.raises(ValueError):
        set_raw(eng, -1, cam)


def test_setting_a_filter_while_batches_are_in_flight(eng):
    W, H, cam_id = 640, 480, 11
    fill_a = np.zeros((1, H, W), np.uint8)
    fill_a[0, :, :64] = 1
    fill_b = np.zeros((2, H, W), np.uint8)
    fill_b[0, :, 576:] = 1
    fill_b[1, :48, :] = 1
    A = fc.Camera.plain(W, H, fill_a)
    B = fc.Camera.plain(W, H, fill_b, area=0.25 * W * H)
    frames = [synthetic_frame(W, H, 900), synthetic_frame(W, H, 901)]
    ptrs = [eng.upload(f) for f in frames]

    def submit(lane):
        eng.submit_device(lane, [ptrs[lane]] * 2, [W, W], [H, H], cams=[cam_id, -1])

    def collect(lane, cam):
        rows = [np.zeros(fc.CALL_ROWS, ROW_DTYPE) for _ in range(2)]
        passes = [np.full(fc.CALL_ROWS, 9, np.uint8) for _ in range(2)]
        eng.collect(lane, rows, passes)
        filtered, plain = rows
        assert (plain["label"] > 0).sum() >= 10 and not plain["zones"].any()
        np.testing.assert_array_equal(passes[1], (plain["label"] > 0).astype(np.uint8))
        want = fc.lattice_verdict(cam, plain)
        np.testing.assert_array_equal(passes[0], want[0])
        np.testing.assert_array_equal(filtered["zones"], want[1])
        expect = plain.copy()
        expect["zones"] = want[1]
        assert filtered.tobytes() == expect.tobytes()
        return plain

    try:
        set_raw(eng, cam_id, A)
        submit(0)
        submit(1)
        set_raw(eng, cam_id, B)                     # neither lane collected: their batches were submitted under A
        plain = [collect(0, A), collect(1, A)]
        for p in plain:
            a, b = fc.lattice_verdict(A, p), fc.lattice_verdict(B, p)
            assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
        submit(0)
        again = collect(0, B)
        assert again.tobytes() == plain[0].tobytes()
    finally:
        eng.sync()
        eng.clear_camera_filter(cam_id)
        for p in ptrs:
            eng.free(p)
