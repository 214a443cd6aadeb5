"""Known answers at the edges of the NMS walk, on the MI355X (nms_cases.py).

Through `stage_postprocess` first: the pair test, the chunk resolution and the band logic are the same wz_nms_band code on the production
path.  Then every case is REPLAYED through the production tail (`_replay`): `stage_post_production` feeds the same head outputs to the
grouped head reduce as its partial sums, so the boxes are decoded there, the first band is listed in the bit map against the slot's hint
and read by the elist / take() code, and the NMS kernel writes the rows -- checked as test_gpu_post_production.py checks a batch (bit for
bit against the stage path, then the oracle, then the rows), with the hint primed where a case is about a chunk or band border.
Exact geometry (th = tw = 0): the boxes are compared BIT FOR BIT with the oracle's, N and the classes exactly, the scores at
1e-6 (expf).  On top of the oracle's rows every pair is asserted by itself: which of its two boxes were kept.

  threshold pairs   engines built with iou_threshold 0.6, 0.5 and 0.45: IoU within 3 ulps of the float32 threshold on either side
                    and exactly on it (the exact double-precision branch of wz_pair_suppresses: mid, tie_up), IoU within 4 ulps of
                    thr * (1 -/+ 1e-3) (the edges of the hoisted clear-case tests), the same geometry in different classes
  ladders           chains that keep every other member: across the 256-candidate chunk border, inside one score bin, across the
                    walk's band borders (the hint primed so that the first band ends inside the chain), two classes interleaved
  clip-after twins  pairs and a ladder with negative coordinates on a clip_after_nms engine (the SIGNED pair test), against
                    multiclass_nms_clip_after"""
import os

import numpy as np
import pytest

import conftest
import nms_cases as N
import parity_utils as pu
from oracle import detect as odet
from watsor_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(tmp_path_factory, synth_weights):
    """key -> development-library engine: an IoU threshold, or "clip_after" (threshold 0.6); the weights do not reach these tests."""
    cache = {}

    def get(key):
        if key not in cache:
            kw = dict(options=dict(clip_after_nms=True)) if key == "clip_after" else dict(post=dict(iou_threshold=key))
            d = tmp_path_factory.mktemp("nms_edges_%s" % str(key).replace(".", "_"))
            engine.save_engine(engine.build_engine(synth_weights, **kw), os.path.join(str(d), "mi355x.bin"))
            cache[key] = conftest.make_engine(str(d), max_batch=8, max_width=300, max_height=300, dev=True)
            assert key == "clip_after" or abs(cache[key].nms_iou - key) < 1e-6
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


def _check(e, be, lg, **okw):
    """stage_postprocess on [n] frames against the literal oracle: N, classes exact, boxes bit for bit, scores within 1e-6."""
    out = []
    for k in range(0, len(be), 8):
        B, S, C, Nn = e.stage_postprocess(be[k:k + 8], lg[k:k + 8])
        rB, rS, rC, rN = pu.oracle_postprocess(be[k:k + 8], lg[k:k + 8], **okw)
        np.testing.assert_array_equal(Nn, rN)
        np.testing.assert_array_equal(C, rC)
        np.testing.assert_array_equal(B.view(np.uint32), rB.view(np.uint32))
        np.testing.assert_allclose(S, rS, rtol=0, atol=1e-6)
        out += [(B[i], S[i], C[i], int(Nn[i])) for i in range(len(Nn))]
    return out


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _replay(e, be, lg, prime=None, **okw):
    """The same head outputs through the production tail (head reduce: decode + candidate bit map; wz_k_nms: listed first band, rows),
    checked as a production batch is: the values arrive bit for bit, det_* and rows equal the stage path's bit for bit, det_* equal the
    oracle's (boxes bit for bit: exact geometry), rows equal rows_as_array.  prime: the hint bin of frame slot 0 on entry.  Returns the
    diagnostics of the last batch."""
    P = None
    for k in range(0, len(be), 8):
        b, l = np.ascontiguousarray(be[k:k + 8]), np.ascontiguousarray(lg[k:k + 8])
        n = len(b)
        if prime is not None:
            _set_hint(e, prime)
        rows = e.stage_post_production(b, l, 300, 300)
        P = e.stage_post_lane(0, n)
        assert P["cands_listed"] and P["decode_fused"]
        if prime is not None:
            assert P["hint_in"][0] == prime
        np.testing.assert_array_equal(_u32(P["box_enc"]), _u32(b))
        np.testing.assert_array_equal(_u32(P["logits"]), _u32(l))
        assert (P["listed"] >= P["first_cnt"]).all() and (P["first_cnt"] > 0).all()      # the first band came out of the bit map
        B, S, C, Nn = e.stage_postprocess(b, l)
        np.testing.assert_array_equal(P["num"], Nn)
        np.testing.assert_array_equal(P["classes"], C)
        np.testing.assert_array_equal(_u32(P["scores"]), _u32(S))
        np.testing.assert_array_equal(_u32(P["boxes"]), _u32(B))
        rB, rS, rC, rN = pu.oracle_postprocess(b, l, **okw)
        np.testing.assert_array_equal(P["num"], rN)
        np.testing.assert_array_equal(P["classes"], rC)
        np.testing.assert_array_equal(_u32(P["boxes"]), _u32(rB))
        np.testing.assert_allclose(P["scores"], rS, rtol=0, atol=1e-6)
        for i in range(n):
            assert rows[i].tobytes() == e.stage_rows(300, 300, B[i], S[i], C[i]).tobytes()
            ref = odet.rows_as_array((300, 300, 3), P["boxes"][i], P["classes"][i], P["scores"][i])
            np.testing.assert_array_equal(rows[i]["label"], ref["label"])
            np.testing.assert_array_equal(rows[i]["confidence"], ref["confidence"])
            np.testing.assert_array_equal(np.stack([rows[i]["x_min"], rows[i]["y_min"], rows[i]["x_max"], rows[i]["y_max"]], 1), ref["box"])
    return P


def _check_pairs(e, thr, border, clip):
    sel = N.select_pairs(thr, border=border, clip=clip)
    okw = dict(iou_thr=thr, clip_after_nms=True) if not clip else dict(iou_thr=thr)
    for twins in (False, True):
        frames = N.frames_of_pairs(sel, twins=twins)
        got = _check(e, np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), **okw)
        _replay(e, np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), **okw)
        for (be, lg, placed), (B, S, C, n) in zip(frames, got):
            dec = np.clip(N.decode(be), np.float32(0), np.float32(1))      # a row is the clipped box in either kind of engine
            for p in placed:
                rows_i = B[:n][C[:n] == p["ci"]]
                kept_j = any(np.array_equal(r.view(np.uint32), dec[p["j"]].view(np.uint32)) for r in B[:n][C[:n] == p["cj"]])
                assert any(np.array_equal(r.view(np.uint32), dec[p["i"]].view(np.uint32)) for r in rows_i), p
                assert kept_j == (not p["suppressed"]), "thr %s %s pair %r: IoU %r, j %s" % (thr, "twins" if twins else "same class", p["kind"],
                                                                                            p["q"], "kept" if kept_j else "suppressed")
    return sel


@pytest.mark.parametrize("thr", [0.6, 0.5, 0.45])
def test_threshold_pairs(engines, thr):
    sel = _check_pairs(engines(thr), thr, border=False, clip=True)
    print("\nthr %s: %d pairs (%s)" % (thr, len(sel), ", ".join(sorted({p["kind"] for p in sel}))))


def _set_hint(e, target):
    """Move the hint of lane 0's frame slot 0 to bin `target` with calls of their own: no candidate lowers it two bins a call, 1 000
    saturated scores raise it one bin a call (k_post.hip: WZ_CAND_TARGET = 192, four times that to raise)."""
    be, quiet = N.blank()
    dense = quiet.copy()
    dense[:1000, 1] = 20.0
    cur = None
    for _ in range(1100):
        if cur == target:
            return
        e.stage_postprocess(be[None], (dense if cur is not None and cur < target else quiet)[None])
        P = e.stage_post_lane(0, 1)
        lo, cnt = int(P["first_lo"][0]), int(P["first_cnt"][0])
        cur = max(lo - 2, 1) if cnt < 192 else min(lo + 1, 1023) if cnt > 768 else lo
    raise AssertionError("the hint did not reach bin %d (at %r)" % (target, cur))


def _bin(score):
    return int(np.float32(score).view(np.uint32) >> 20)


def _every_other(got, be, info, clip=True):
    B, S, C, n = got
    dec = N.decode(be)
    if clip:
        dec = np.clip(dec, np.float32(0), np.float32(1))
    for col, ids in info["chains"]:
        rows = B[:n][C[:n] == col]
        assert len(rows) >= 40
        np.testing.assert_array_equal(rows.view(np.uint32), dec[ids[::2]][:len(rows)].view(np.uint32))


@pytest.mark.parametrize("kind", ["long", "single_bin", "interleaved"])
def test_ladders(engines, kind):
    e = engines(0.6)
    be, lg, info = N.ladder_frame(kind)
    if kind == "long":        # a first band that reaches well below member 126 of the ladder (score 0.0038), so that ONE band holds more than a chunk
        Q = _replay(e, be[None], lg[None], prime=_bin(0.0005))
        assert Q["first_cnt"][0] >= 256 + 2 and Q["listed"][0] >= Q["first_cnt"][0]         # ... read from the bit map, the chunk border inside it
        _set_hint(e, _bin(0.0005))
    else:
        _replay(e, be[None], lg[None])
    got = _check(e, be[None], lg[None])[0]
    assert got[3] == min(100, sum((len(ids) + 1) // 2 for _, ids in info["chains"]) + (1 if kind == "long" else 0))
    _every_other(got, be, info)
    P = e.stage_post_lane(0, 1)
    print("\n%s: first band %d candidates from bin %d, %d walked" % (kind, P["first_cnt"][0], P["first_lo"][0], P["processed"][0]))
    if kind == "long":
        assert P["first_cnt"][0] >= 256 + 2                        # sorted positions 255 .. 257, members 125 .. 127 of the chain, lie in ONE band: it crosses the chunk border
        assert got[3] == 100 and (got[2][:100] == info["cluster"][0]).sum() == 1


def test_ladder_across_band_borders(engines):
    """The hint primed so that the first band ends inside the ladder, near its top, in its middle and near its end: the members
    kept in one band must go on suppressing in the bands below."""
    e = engines(0.6)
    be, lg, info = N.ladder_frame("bands")
    shown = []
    for target_score in (0.9, 0.1, 0.01):
        Q = _replay(e, be[None], lg[None], prime=_bin(target_score))
        assert 0 < Q["first_cnt"][0] < Q["processed"][0]             # the listed first band ended inside the chain, too
        _set_hint(e, _bin(target_score))
        got = _check(e, be[None], lg[None])[0]
        _every_other(got, be, info)
        P = e.stage_post_lane(0, 1)
        first, walked = int(P["first_cnt"][0]), int(P["processed"][0])
        shown.append((target_score, int(P["hint_in"][0]), first, walked))
        assert 0 < first < walked, shown                            # the first band ended inside the chain
    print("\nbands: (score primed to, hint on entry, first band, walked) %s" % shown)


def test_clip_after_twins(engines):
    e = engines("clip_after")
    sel = _check_pairs(e, 0.6, border=True, clip=False)
    assert len(sel) >= 20
    for kind in ("bands", "long"):
        be, lg, info = N.ladder_frame(kind, outside=True)
        _replay(e, be[None], lg[None], clip_after_nms=True)
        B, S, C, n = _check(e, be[None], lg[None], clip_after_nms=True)[0]
        col, ids = info["chains"][0]
        dec = N.decode(be)
        assert dec[ids].min() < -0.1
        # every other member is selected; those left without area after clipping are no rows, the others are the clipped boxes
        want = np.clip(dec[ids[::2]], np.float32(0), np.float32(1))
        want = want[(want[:, 2] - want[:, 0]) * (want[:, 3] - want[:, 1]) > 0]
        rows = B[:n][C[:n] == col]
        assert len(rows) >= 30
        np.testing.assert_array_equal(rows.view(np.uint32), want[:len(rows)].view(np.uint32))
