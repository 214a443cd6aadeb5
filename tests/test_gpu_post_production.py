"""The post-processing a real batch runs, on the MI355X, on heads that look trained.

Every other post-processing test goes through `stage_postprocess`: wz_k_decode, then wz_k_nms scanning the logits for its first band,
then the det_* arrays.  A batch that comes in through `submit_host` runs none of that front end: the boxes are decoded inside the grouped
head reduce, the first band is read from the bit map that reduce fills by comparing finished logits with the slot's `hint_logit` (left
there by the slot's previous NMS), the two-pass list / `take()` code turns the map into the band, and the NMS kernel writes the rows.

The check, per frame of a production batch (`_verify`): take (be, lg), the GPU's OWN head outputs, read back from the lane by
`stage_post_lane` (no kernel launched), and require
  * the production det_* arrays and rows == what the stage path gives on (be, lg) on the same engine, BIT FOR BIT (same expf, two front ends);
  * the det_* arrays == `parity_utils.oracle_postprocess(be, lg)` at test_gpu_parity._check_post's bars (N and classes exact, scores
    1e-6, boxes 2e-6) -- on at most a dozen frames per test, the literal per-class oracle is what takes the time;
  * the rows == `oracle.detect.rows_as_array` of the production det_* arrays.
`expf` against numpy at the last ulp stays unpinned, hence the two steps.

Weights: trained_like_heads.py (noise = busy scene, constant frame = the quiet / dead-column scene whose rows end inside a bin of
9 585 equal scores).  Programs and their flags (decode_fused, cands_listed), asserted on every frame:

  mobilenet_v2_default     `-p 16` default            True, True    asserted, regimes asserted
  mobilenet_v2_robust      `-p 16` robust             True, True    asserted, regimes asserted
  mobilenet_v2_clip_after  default + clip_after_nms   True, True    asserted
  mobilenet_v2_cap3        default + max_per_class=3  True, True    asserted
  mobilenet_v1_fused       `-p 16`                    True, True    as read back on the MI355X (all six heads go through the grouped reduce
  inception_v2_p16         `-p 16`                    True, True    there as well), so asserted too: the listed path, not the fallback

Regimes (`REGIMES`), read from the diagnostic words of wz_k_nms -- first-band count, candidates walked, entries found in the bit map,
the first band's lower bin as walked, the hint on entry -- and asserted by the module's last test for the programs marked above:
  short     the first band came up short: more candidates walked than the first band held
  sufficed  the first band came from the list as hinted and held all 100 rows
  raised    the first band overflowed WZ_CAND_CAP and its lower edge was raised
  fallback  more than 2 * WZ_CAND_CAP listed entries: `take()` straight from the bit-map loop
  serial    the kernel's own word: wz_nms_band_serial walked a bin (and, as a cross-check of that word, a row's score then lies in a bin
            that holds more than WZ_CAND_CAP scores, and more than WZ_CAND_CAP candidates were walked)
"""
import os
import time

import numpy as np
import pytest

import conftest
import parity_utils as pu
import trained_like_heads as H
from oracle import detect as odet
from oracle.postprocess import sigmoid
from watsor_amd import arch, engine, inception, mobilenet_v1
from watsor_amd.runtime import ROW_DTYPE
from watsor_amd.synth import synthetic_inception_v2, synthetic_mobilenet_v1, synthetic_weights

pytestmark = pytest.mark.gpu

SEED, HEAD_SEED = 1234, 5
WZ_CAND_CAP = H.WZ_CAND_CAP
REGIMES = ("short", "sufficed", "raised", "fallback", "serial")

# program -> (seeded weights, the one-op-per-layer program the generator walks, build_engine arguments, the oracle twin's arguments,
#             flags asserted, regimes asserted)
PROGRAMS = {
    "mobilenet_v2_default":    (synthetic_weights, lambda: arch.build(fuse=False), dict(), dict(), True, True),
    "mobilenet_v2_robust":     (synthetic_weights, lambda: arch.build(fuse=False), dict(robust=True), dict(), True, True),
    "mobilenet_v2_clip_after": (synthetic_weights, lambda: arch.build(fuse=False), dict(options=dict(clip_after_nms=True)),
                                dict(clip_after_nms=True), True, False),
    "mobilenet_v2_cap3":       (synthetic_weights, lambda: arch.build(fuse=False), dict(post=dict(max_per_class=3)),
                                dict(max_per_class=3), True, False),
    "mobilenet_v1_fused":      (synthetic_mobilenet_v1, lambda: mobilenet_v1.build(fuse=False), dict(), dict(), True, False),
    "inception_v2_p16":        (synthetic_inception_v2, lambda: inception.build(), dict(), dict(), True, False),
}
MAIN = ("mobilenet_v2_default", "mobilenet_v2_robust")

_seen = {name: set() for name in PROGRAMS}       # program -> regimes its tests have shown so far
_flags = {}                                      # program -> (decode_fused, cands_listed) as read back
_values = {name: {} for name in PROGRAMS}        # program -> regime -> the diagnostic words of the first frame that showed it


@pytest.fixture(scope="module")
def engines(tmp_path_factory):
    """name -> a development-library engine (max_batch 8) of that program on the trained-like heads, built on first use."""
    cache, weights = {}, {}

    def get(name):
        if name not in cache:
            make_weights, make_prog, kw = PROGRAMS[name][:3]
            if make_weights not in weights:
                weights[make_weights] = H.trained_heads(make_weights(SEED), make_prog(), HEAD_SEED)
            d = tmp_path_factory.mktemp(name)
            engine.save_engine(engine.build_engine(weights[make_weights], **kw), os.path.join(str(d), "mi355x.bin"))
            cache[name] = conftest.make_engine(str(d), max_batch=8, max_width=300, max_height=300, dev=True)
        return cache[name]
    yield get
    for e in cache.values():
        e.close()


_frames = {}


def scene(kind, seed, small=False):
    """A frame of trained_like_heads.frame_kinds: 300 x 300, or 64 x 48 (the frame size does not reach the post-processing)."""
    key = (seed, small)
    if key not in _frames:
        _frames[key] = H.frame_kinds(seed, *((64, 48) if small else (300, 300)))
    return _frames[key][kind]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _regimes(P, i, lg):
    """The regimes frame i of a production batch shows, from its diagnostic words (and, for `serial`, its scores)."""
    out = set()
    first_cnt, processed, listed = int(P["first_cnt"][i]), int(P["processed"][i]), int(P["listed"][i])
    first_lo, hint_in, num = int(P["first_lo"][i]), int(P["hint_in"][i]), int(P["num"][i])
    if not P["cands_listed"]:
        assert listed == 0
        return out
    if processed > first_cnt:
        out.add("short")
    if listed > 0 and first_lo == hint_in and processed == first_cnt and num == 100:
        out.add("sufficed")
    if first_lo > hint_in:
        assert listed > WZ_CAND_CAP          # (the list holds at least the band that overflowed)
        out.add("raised")
    if listed > 2 * WZ_CAND_CAP:
        out.add("fallback")
    hist = np.bincount(H.score_bins(sigmoid(lg[:, 1:])).ravel(), minlength=H.WZ_HIST_BINS)
    row_bins = H.score_bins(P["scores"][i][:num])
    if P["serial"][i]:
        assert processed > WZ_CAND_CAP
        assert hist.max() > WZ_CAND_CAP - 64, "the serial walk ran, but no bin is crowded"
        out.add("serial")
    else:
        assert not [b for b in np.unique(row_bins) if hist[b] > WZ_CAND_CAP + 2000]      # a row out of a bin only the serial walk takes
    return out


def _verify(e, name, slot, frames, rows, P, oracle_on):
    """The module docstring's check on every frame of the batch `frames` that lane `slot` ran (its rows in `rows`, its device state in
    P, read before anything else ran on lane 0); the oracle on the frames listed in `oracle_on`."""
    okw, assert_flags = PROGRAMS[name][3], PROGRAMS[name][4]
    n = len(frames)
    _flags.setdefault(name, (P["decode_fused"], P["cands_listed"]))
    assert _flags[name] == (P["decode_fused"], P["cands_listed"]), "the path changed between batches of one program"
    if assert_flags:
        assert P["cands_listed"] and P["decode_fused"], "%s fell back to the scanned first band / the decode kernel" % name
    be, lg = P["box_enc"], P["logits"]
    assert np.isfinite(be).all() and np.isfinite(lg).all()
    B, S, C, N = e.stage_postprocess(be, lg)                      # the stage path on the same head outputs, same engine
    np.testing.assert_array_equal(P["num"], N)
    np.testing.assert_array_equal(P["classes"], C)
    np.testing.assert_array_equal(_bits(P["scores"]), _bits(S))
    np.testing.assert_array_equal(_bits(P["boxes"]), _bits(B))
    for i, f in enumerate(frames):
        h, w = f.shape[:2]
        got = np.asarray(rows[i])
        assert got.tobytes() == e.stage_rows(w, h, B[i], S[i], C[i]).tobytes(), "%s lane %d frame %d: rows differ from the stage path's" % (name, slot, i)
        ref = odet.rows_as_array(f.shape, P["boxes"][i], P["classes"][i], P["scores"][i])
        np.testing.assert_array_equal(got["label"], ref["label"])
        np.testing.assert_array_equal(got["confidence"], ref["confidence"])
        np.testing.assert_array_equal(np.stack([got["x_min"], got["y_min"], got["x_max"], got["y_max"]], 1), ref["box"])
        assert not got["zones"].any() and not got["_pad"].any()
        r = _regimes(P, i, lg[i])
        for k in r - _seen[name]:
            _values[name][k] = {q: int(P[q][i]) for q in ("hint_in", "first_lo", "first_cnt", "first_kept", "processed", "listed", "num")}
        _seen[name] |= r
    idx = list(oracle_on)
    if idx:
        rB, rS, rC, rN = pu.oracle_postprocess(be[idx], lg[idx], **okw)
        np.testing.assert_array_equal(P["num"][idx], rN)
        np.testing.assert_array_equal(P["classes"][idx], rC)
        np.testing.assert_allclose(P["scores"][idx], rS, rtol=0, atol=1e-6)
        np.testing.assert_allclose(P["boxes"][idx], rB, rtol=0, atol=2e-6)
    return P


def _batch(e, name, slot, frames, oracle_on=()):
    """One production batch on lane `slot`, collected and verified."""
    e.submit_host(slot, frames)
    rows = [np.zeros(100, ROW_DTYPE) for _ in frames]
    e.collect(slot, rows)
    return _verify(e, name, slot, frames, rows, e.stage_post_lane(slot, len(frames)), oracle_on)


def _next_hint(first_lo, first_cnt):
    """Where wz_k_nms leaves the hint (k_post.hip: WZ_CAND_TARGET = 192)."""
    if first_cnt < 192:
        return max(first_lo - 2, 1)
    if first_cnt > 4 * 192:
        return min(first_lo + 1, H.WZ_HIST_BINS - 1)
    return first_lo


def _prime(e, n, target):
    """Move the hint of lane 0's frame slots 0 .. n - 1 to `target` with stage_postprocess calls, which share post.hint / post.hint_logit
    with lane 0's production path.  Per slot: no candidate at all lowers it two bins a call, 1 000 saturated scores raise it one bin a
    call, 400 of them hold it where it is."""
    A, Cn = e.num_anchors, e.num_classes
    be = np.zeros((n, A, 4), np.float32)
    lg = np.full((n, A, Cn), -30.0, np.float32)
    cur = [None] * n
    for _ in range(1100):
        if all(c == target for c in cur):
            return
        for f in range(n):
            lg[f, :, 1] = -30.0
            if cur[f] is not None and cur[f] <= target:
                lg[f, :1000 if cur[f] < target else 400, 1] = 20.0
        e.stage_postprocess(be, lg)
        P = e.stage_post_lane(0, n)
        cur = [_next_hint(int(a), int(b)) for a, b in zip(P["first_lo"], P["first_cnt"])]
    raise AssertionError("the hints did not reach bin %d (at %r)" % (target, cur))


BATCH_NAMES = list(PROGRAMS)


@pytest.mark.parametrize("name", MAIN)
def test_batch_sizes_on_one_lane(engines, name):
    """Batches of 8, 1, 3 and 8 on lane 0, a different scene in every slot: slots 1 .. 7 carry the hints -- and would carry any bit left
    in the map -- of the first batch into the last."""
    t0 = time.time()
    e = engines(name)
    kinds = ("noise", "constant", "synthetic")
    first = [scene(kinds[i % 3], i, small=i in (2, 5)) for i in range(8)]
    last = [scene(kinds[(i + 1) % 3], 10 + i, small=i == 4) for i in range(8)]
    _batch(e, name, 0, first, oracle_on=(0, 1, 7))
    _batch(e, name, 0, [scene("constant", 21)], oracle_on=(0,))
    _batch(e, name, 0, [scene("noise", 22), scene("synthetic", 23, small=True), scene("constant", 24)], oracle_on=(0, 1, 2))
    P = _batch(e, name, 0, last, oracle_on=(0, 3, 6, 7))
    print("\n%s: batches 8, 1, 3, 8 in %.1f s; last batch hint_in %s first_cnt %s listed %s" %
          (name, time.time() - t0, P["hint_in"].tolist(), P["first_cnt"].tolist(), P["listed"].tolist()))


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_scene_cuts_through_one_slot(engines, name):
    """Busy, constant, busy, dead-column, constant and busy scenes through frame slot 0 of lane 0 (the constant frames ARE the
    dead-column scene: their rows end inside the crowded bin), every frame against the oracle -- for the two build options against
    their oracle twins."""
    t0 = time.time()
    e = engines(name)
    seen = []
    cuts = (("noise", 30), ("constant", 30), ("noise", 31), ("constant", 31), ("constant", 32), ("noise", 32))
    if name == "mobilenet_v2_cap3":          # (three rows a class: every frame walks the whole crowded bin one candidate at a time, ~0.7 s a run)
        cuts = cuts[:2]
    for kind, seed in cuts:
        P = _batch(e, name, 0, [scene(kind, seed)], oracle_on=(0,))
        seen.append((kind, int(P["hint_in"][0]), int(P["first_lo"][0]), int(P["first_cnt"][0]), int(P["processed"][0]), int(P["listed"][0])))
    print("\n%s: flags (decode_fused, cands_listed) = %s; (scene, hint_in, first_lo, first_cnt, processed, listed): %s; %.1f s" %
          (name, _flags[name], seen, time.time() - t0))
    if name == "mobilenet_v2_cap3":
        assert np.bincount(P["classes"][0][:P["num"][0]]).max() == 3


@pytest.mark.parametrize("name", MAIN)
def test_primed_hints(engines, name):
    """The ends of the hint's range, reached by priming lane 0: bin 1 (the whole frame is listed: 172 k entries, all but the first
    8 192 through `take()` in the bit-map loop, and the band is raised again and again), the bin of 1.0 (a first band of ties that the
    anchor index orders), the bin above every score (an empty first band), and the bin just above the dead columns' (a busy frame's
    first band suffices)."""
    e = engines(name)
    frames = [scene("noise", 40), scene("constant", 40), scene("synthetic", 40)]
    one = int(H.score_bins(np.float32([1.0]))[0])
    for target, oracle_on in ((1, (0, 1)), (one, (1, 2)), (one + 1, (0,)), (H.dead_bin() + 1, (0, 2))):
        _prime(e, len(frames), target)
        P = _batch(e, name, 0, frames, oracle_on=oracle_on)
        assert (P["hint_in"] == target).all()
        if target == 1:
            assert (P["listed"] > 100000).all() and (P["first_lo"] > target).all()
        if target == one + 1:
            assert (P["first_cnt"] == 0).all() and (P["processed"] > 0).all()
    assert "sufficed" in _seen[name]


@pytest.mark.parametrize("name", MAIN)
def test_all_lanes_with_their_own_histories(engines, name):
    """The same scenes through every lane the engine has, lane k after k batches of other scenes that lane 0 never saw (its hints and
    its bit map are its own): every lane's rows equal lane 0's byte for byte, and every lane passes the check."""
    e = engines(name)
    lanes = e.num_slots
    assert lanes >= 2
    frames = [scene("noise", 50), scene("constant", 50), scene("synthetic", 50, small=True), scene("constant", 51)]
    for k in range(1, lanes):
        for j in range(k):
            other = [scene(("constant", "noise")[(j + k) % 2], 60 + j)] * (1 + (j + k) % 3)
            e.submit_host(k, other)
            e.collect(k, [np.zeros(100, ROW_DTYPE) for _ in other])
    for k in range(lanes):
        e.submit_host(k, frames)
    rows = {}
    for k in range(lanes):
        rows[k] = [np.zeros(100, ROW_DTYPE) for _ in frames]
        e.collect(k, rows[k])
    state = {k: e.stage_post_lane(k, len(frames)) for k in range(lanes)}       # before the stage path overwrites lane 0's
    hints = {k: state[k]["hint_in"].tolist() for k in range(lanes)}
    assert len({tuple(h) for h in hints.values()}) > 1, hints                   # (the histories did differ)
    for k in range(lanes):
        for a, b in zip(rows[0], rows[k]):
            assert a.tobytes() == b.tobytes()
        _verify(e, name, k, frames, rows[k], state[k], oracle_on=(0, 1, 2, 3) if k == 0 else ())
    print("\n%s: %d lanes, hints on entry %s" % (name, lanes, hints))


@pytest.mark.parametrize("name", MAIN)
def test_every_regime_was_reached(name):
    """Regimes are conditions, not hopes: the tests above (this module run as a whole) showed every one of them on this program."""
    print("\n%s: %s" % (name, _values[name]))
    missing = [r for r in REGIMES if r not in _seen[name]]
    assert not missing, "%s never showed: %s (run the whole module: the regimes are collected over its tests)" % (name, missing)
