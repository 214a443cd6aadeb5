"""The NMS edge cases (nms_cases.py) are what they claim to be, by the oracle's own float32 `iou()` (no GPU)."""
from collections import Counter

import numpy as np
import pytest

import nms_cases as N
from oracle import postprocess as post

F32 = np.float32


@pytest.mark.parametrize("thr", [0.6, 0.5, 0.45])
def test_threshold_pair_populations(thr):
    """The +/- 3000-ulp scan over six anchors and three tx values: at least 8 pairs strictly below and 8 strictly above the float32
    threshold within 3 ulps of it, for 0.5 and 0.45 at least 3 exactly on it -- checked pair by pair with the scalar iou()."""
    found = N.scan_pairs(thr)
    t32 = F32(thr)
    dec0 = N.decode(N.blank()[0])
    for it in found[::7]:
        be = N.blank()[0]
        be[it["j"]] = it["enc"]
        assert (be[:, 2:] == 0).all()
        boxes = post.clip_to_unit_window(N.decode(be))
        np.testing.assert_array_equal(boxes[it["i"]], post.clip_to_unit_window(dec0)[it["i"]])      # i is the anchor as it stands
        q = post.iou(boxes[it["i"]], boxes[it["j"]])
        assert q == it["q"] and abs(int(N.ulps(q, t32))) <= N.NEAR_ULPS
        assert it["rel"] == (1 if q > t32 else -1 if q < t32 else 0)
    n = Counter(it["rel"] for it in found)
    print(thr, dict(n))
    assert n[-1] >= 8 and n[1] >= 8
    if thr in (0.5, 0.45):
        assert n[0] >= 3


@pytest.mark.parametrize("thr,border,clip", [(0.6, False, True), (0.5, False, True), (0.45, False, True), (0.6, True, False)])
def test_selected_pairs_and_their_frames(thr, border, clip):
    sel = N.select_pairs(thr, border=border, clip=clip)
    kinds = Counter(it["kind"] for it in sel)
    assert kinds["below"] >= 8 and kinds["above"] >= 8 and (thr == 0.6 or kinds["equal"] >= 3)
    t32 = F32(thr)
    lo, hi = F32(t32 * F32(0.999)), F32(t32 * F32(1.001))
    for it in sel:
        if it["kind"][:2] in ("lo", "hi"):
            edge = lo if it["kind"][:2] == "lo" else hi
            assert abs(int(N.ulps(it["q"], edge))) <= 4
            assert it["rel"] == (-1 if edge < t32 else 1)
    assert all(kinds[k] >= 1 for k in ("lo-1", "lo+1", "hi-1", "hi+1")), kinds
    frames = N.frames_of_pairs(sel)
    assert sum(len(placed) for _, _, placed in frames) == len(sel)
    if border:
        assert min(N.decode(be)[[p["i"] for p in placed]][:, 0].min() for be, _, placed in frames) < 0      # boxes reach above the image
    for twins in (False, True):
        for be, lg, placed in N.frames_of_pairs(sel, twins=twins):
            assert (be[:, 2:] == 0).all()
            cand = np.argwhere(lg[:, 1:] > N.OFF)
            assert len(cand) == 2 * len(placed)
            live = np.sort(lg[lg > N.OFF])
            assert np.diff(live).min() >= 0.05                       # no two candidates an ulp of expf could reorder
            kw = dict(iou_thr=thr, clip_after_nms=not clip)
            b, s, c, nd = post.postprocess(be, lg, N.anchors_cs(), **kw)
            assert nd == 2 * len(placed) - sum(p["suppressed"] for p in placed)
            for p in placed:
                assert (c[:nd] == p["ci"]).sum() + (0 if p["ci"] == p["cj"] else (c[:nd] == p["cj"]).sum()) == (1 if p["suppressed"] else 2)
            if twins:
                assert not any(p["suppressed"] for p in placed)


@pytest.mark.parametrize("kind", ["long", "single_bin", "bands", "interleaved"])
@pytest.mark.parametrize("outside", [False, True])
def test_ladders_are_chains(kind, outside):
    thr = post.IOU_THRESHOLD
    be, lg, info = N.ladder_frame(kind, outside=outside)
    assert (be[:, 2:] == 0).all()
    for col, ids in info["chains"]:
        lo, hi = N.chain_properties(be, ids, thr, clip=False)
        assert lo > thr + 0.03 and hi < thr - 0.1                     # neighbours suppress, nobody else does: margins no rounding reaches
        s = post.sigmoid(lg[ids, col])
        assert (np.diff(s) < 0).all()                                 # strictly descending along the chain
        if kind == "single_bin":
            assert len(set((s.view(np.uint32) >> 20).tolist())) == 1
        if kind == "bands":
            assert len(set((s.view(np.uint32) >> 20).tolist())) >= 60
    if kind == "long":
        assert len(info["chains"][0][1]) > 256 - len(info["cluster"][1]) + 60 and len(info["cluster"][1]) + len(info["chains"][0][1]) > 256
    if outside:
        assert N.decode(be)[info["chains"][0][1]].min() < -0.1
        return
    # greedy NMS keeps every other member (the oracle says so: the first rows of a chain's class are its members 0, 2, 4, ...)
    b, s, c, nd = post.postprocess(be, lg, N.anchors_cs())
    assert nd == min(100, sum((len(ids) + 1) // 2 for _, ids in info["chains"]) + (1 if kind == "long" else 0))
    boxes = post.clip_to_unit_window(N.decode(be))
    for col, ids in info["chains"]:
        rows = b[:nd][c[:nd] == col]
        assert len(rows) >= 40
        np.testing.assert_array_equal(rows, boxes[ids[::2]][:len(rows)])
    if kind == "long":
        assert (c[:nd] == info["cluster"][0]).sum() == 1              # the cluster's one survivor: 64 rows kept where the chunk ends
