"""Known answers at the edges of the NMS walk (test infrastructure; tests/test_nms_cases_cpu.py asserts that the cases are what they
claim, tests/test_gpu_nms_edges.py runs them on the MI355X).

Exact geometry.  Every encoding here has th = tw = 0: exp(0) == 1 in any implementation, the rest of the decode is one division, one
product and two sums per coordinate, each rounded once -- the decoded boxes are BIT-identical on the GPU and in oracle/postprocess.py,
and so is every IoU.  A box is its anchor's shape, moved by (ty, tx).  Logits of candidates whose order matters lie at least LOGIT_STEP
apart (the single-bin ladder: FINE_STEP), far more than an ulp of expf can move them.

Threshold pairs: anchor i as it stands (encoding 0) and its neighbour j one grid row further down, same shape, moved back up so that
IoU(i, j) lands on the engine's threshold: the encoding of j steps through neighbouring float32 values, and the pairs kept are those
whose oracle `iou()` -- TF's float32 quotient -- lies within 3 ulps of float32(thr): strictly below, exactly equal (not suppressed:
the comparison is `>`) and strictly above.  Margin pairs lie within a few ulps of thr * (1 -/+ 1e-3), the edges between the NMS
kernel's clear-case tests and its exact double-precision test.  i scores higher than j; every pair has a class of its own.

Ladders: chains of same-class boxes in strictly descending score, each overlapping its successor above the threshold and every other
member of the chain at or below it: greedy NMS keeps members 0, 2, 4, ...; a resolver that lets a suppressed member suppress keeps
fewer, one that forgets a kept member across a chunk or band border keeps more."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import postprocess as post

F32 = np.float32
NUM_COLS = 91
OFF = F32(-30.0)             # a logit that is no candidate: sigmoid(-30) = 9e-14 < the graph's 1e-8 score threshold
LOGIT_STEP = 0.06
FINE_STEP = 0.002            # score steps of 5e-4 around 0.5: four orders of magnitude above an ulp of expf
SCAN_ULPS = 3000
NEAR_ULPS = 3
G0, APL0 = 19, 3             # the first feature map: 19 x 19 locations, 3 anchors each; anchor 0 of a location is the 0.1 x 0.1 square
_ANCHORS = None


def anchors_cs() -> np.ndarray:
    global _ANCHORS
    if _ANCHORS is None:
        _ANCHORS = post.anchors_center_size(post.generate_anchors())
    return _ANCHORS


def blank() -> Tuple[np.ndarray, np.ndarray]:
    """(box encodings [1917, 4] all zero, logits [1917, 91] all OFF)."""
    A = anchors_cs().shape[0]
    return np.zeros((A, 4), F32), np.full((A, NUM_COLS), OFF, F32)


def decode(be: np.ndarray) -> np.ndarray:
    return post.decode_boxes(np.asarray(be, F32), anchors_cs())


def ulps(q, ref) -> np.ndarray:
    """Signed distance of positive float32 values q from ref in units in the last place."""
    return np.asarray(q, F32).view(np.int32).astype(np.int64) - int(np.asarray(ref, F32).view(np.int32))


# (anchor index i, its same-shape neighbour one grid row down): three shapes of the first map, three of the second, away from the border
def _pair_anchors(border: bool) -> List[Tuple[int, int]]:
    out = []
    for y, x, a in ((9, 9, 0), (9, 13, 1), (4, 9, 2)) if not border else ((0, 9, 1), (0, 3, 2), (0, 14, 1)):
        i = (y * G0 + x) * APL0 + a
        out.append((i, i + G0 * APL0))
    off1, g1, apl1 = G0 * G0 * APL0, 10, 6
    for y, x, a in ((4, 4, 0), (3, 6, 3), (5, 3, 5)) if not border else ((0, 4, 0), (0, 6, 1), (0, 2, 5)):
        i = off1 + (y * g1 + x) * apl1 + a
        out.append((i, i + g1 * apl1))
    return out


TX = (0.0, 0.05, 0.11)


def scan_pairs(thr: float, target: Optional[float] = None, near: int = NEAR_ULPS, border: bool = False, clip: bool = True) -> List[dict]:
    """Every (anchor pair, tx, encoding of j) of the +/- SCAN_ULPS scan whose IoU lies within `near` ulps of float32(target) (default:
    the threshold itself), as dict(i, j, enc [4], q float32, d ulps from float32(target), rel = -1 / 0 / +1 against float32(thr)).
    border: anchors of the first grid row, whose boxes reach above the image; clip: the IoU of the boxes clipped to the image (what an
    engine that clips before the NMS compares), else of the boxes as decoded (clip_after_nms)."""
    an = anchors_cs()
    t32 = F32(thr)
    tgt = F32(t32 if target is None else target)
    t = float(tgt)
    out = []
    for i, j in _pair_anchors(border):
        yci, xci, h, w = (float(v) for v in an[i])
        assert np.abs(an[j][1:] - an[i][1:]).max() < 1e-6      # (the same shape and column up to the rounding of the anchor table)
        box_i = decode(np.zeros((an.shape[0], 4), F32))[i]
        if clip:
            box_i = post.clip_to_unit_window(box_i[None])[0]
        for tx in TX:
            dx = tx * w
            dy = h - 2.0 * h * w * t / ((1.0 + t) * (w - dx))              # IoU of two h x w boxes offset by (dy, dx) == t
            e0 = F32(10.0 * (yci + dy - float(an[j][0])) / h)
            e1 = F32(10.0 * tx)
            base = int(np.asarray(e0).view(np.int32))
            codes = np.zeros((2 * SCAN_ULPS + 1, 4), F32)
            codes[:, 0] = (base + np.arange(-SCAN_ULPS, SCAN_ULPS + 1)).astype(np.int32).view(F32)
            codes[:, 1] = e1
            boxes = post.decode_boxes(codes, np.repeat(an[j][None], len(codes), 0))
            if clip:
                boxes = post.clip_to_unit_window(boxes)
            q = post.iou_many(box_i, boxes)
            d = ulps(q, tgt)
            for k in np.nonzero(np.abs(d) <= near)[0]:
                out.append(dict(i=i, j=j, enc=codes[k].copy(), q=F32(q[k]), d=int(d[k]),
                                rel=int(np.sign(int(ulps(q[k], t32))))))
    return out


def select_pairs(thr: float, border: bool = False, clip: bool = True, each: int = 10, equal: int = 6, margin: int = 2) -> List[dict]:
    """The pairs of one threshold's frame: up to `each` strictly below and `each` strictly above the threshold (spread over the
    anchors and tx values: round-robin over the scan's order), up to `equal` exactly on it, and per margin edge thr * (1 -/+ 1e-3) up
    to `margin` pairs on either side of it.  Deterministic."""
    found = scan_pairs(thr, border=border, clip=clip)

    def spread(items, n):
        groups: Dict[tuple, list] = {}
        for it in items:
            groups.setdefault((it["i"], float(it["enc"][1])), []).append(it)
        for g in groups.values():
            g.sort(key=lambda it: abs(it["d"]))
        out = []
        while len(out) < n and any(groups.values()):
            for g in groups.values():
                if g and len(out) < n:
                    out.append(g.pop(0))
        return out

    sel = []
    for rel, n, kind in ((-1, each, "below"), (0, equal, "equal"), (1, each, "above")):
        for it in spread([f for f in found if f["rel"] == rel], n):
            sel.append(dict(it, kind=kind))
    t32 = F32(thr)
    for factor, name in ((F32(0.999), "lo"), (F32(1.001), "hi")):
        edge = F32(t32 * factor)
        near = scan_pairs(thr, target=float(edge), near=4, border=border, clip=clip)
        for side in (-1, 1):
            for it in spread([f for f in near if (f["d"] > 0) - (f["d"] < 0) == side or (side == 1 and f["d"] == 0)], margin):
                sel.append(dict(it, kind="%s%+d" % (name, side)))
    return sel


def pairs_frame(pairs: List[dict], twins: bool = False) -> Tuple[np.ndarray, np.ndarray, List[dict]]:
    """(be, lg, placed) of one frame holding every pair in a class of its own: pair p's anchor i in column 1 + p at logit
    4 - 2 p LOGIT_STEP, its moved neighbour j one LOGIT_STEP lower -- in the same column, or (twins=True) in column 46 + p: the same
    geometry in different classes, never suppressed.  placed: the pairs with their columns and whether j must be suppressed."""
    assert len(pairs) <= 45
    be, lg = blank()
    placed = []
    for p, it in enumerate(pairs):
        ci = 1 + p
        cj = 46 + p if twins else ci
        assert not be[it["j"]].any() and lg[it["i"], ci] == OFF and lg[it["j"], cj] == OFF
        be[it["j"]] = it["enc"]
        lg[it["i"], ci] = F32(4.0 - 2 * p * LOGIT_STEP)
        lg[it["j"], cj] = F32(4.0 - (2 * p + 1) * LOGIT_STEP)
        placed.append(dict(it, ci=ci, cj=cj, suppressed=(not twins) and it["rel"] > 0))
    return be, lg, placed


def frames_of_pairs(pairs: List[dict], twins: bool = False) -> List[Tuple[np.ndarray, np.ndarray, List[dict]]]:
    """The selected pairs dealt out over as few frames as hold them: a frame takes each anchor pair (i, j) once, because j has one
    encoding per frame."""
    frames: List[List[dict]] = []
    for it in pairs:
        for fr in frames:
            if all(o["j"] != it["j"] for o in fr):
                fr.append(it)
                break
        else:
            frames.append([it])
    return [pairs_frame(fr, twins) for fr in frames]


# ------------------------------------------------------------------------------------------------------------------------------
# ladders
# ------------------------------------------------------------------------------------------------------------------------------
SQUARES = [(y * G0 + x) * APL0 for y in range(G0) for x in range(G0)]     # the 361 anchors of the first map's 0.1 x 0.1 shape


def ladder_step(thr: float) -> float:
    """The offset d between neighbours of a ladder of h x h boxes: IoU(d) = (h - d) / (h + d) > thr >= IoU(2 d), in the middle of the
    interval that allows (thr 0.6, h 0.1: d in [0.0125, 0.025) -> 0.0219; IoU(d) = 0.64, IoU(2 d) = 0.39)."""
    h = float(anchors_cs()[0][2])
    hi = h * (1.0 - thr) / (1.0 + thr)
    return 0.75 * hi + 0.25 * (hi / 2.0)


def snake(n: int, d: float, y0: float = 0.1, x0: float = 0.08, run: int = 36) -> np.ndarray:
    """Centres [n, 2] (y, x) of a chain with neighbours d apart: `run` steps to the right, 8 steps down (past the reach of the row
    above: 8 d > h), `run` steps to the left, ..."""
    out, y, x, sx = [], y0, x0, 1.0
    k = 0
    while len(out) < n:
        out.append((y, x))
        k += 1
        phase = k % (run + 8)
        if phase == 0:
            sx = -sx
        if 0 < phase <= run:
            x += sx * d
        else:
            y += d
    return np.asarray(out, np.float64)


def place(be: np.ndarray, anchor_ids, centres) -> None:
    """Encodings (th = tw = 0) that move the given anchors' boxes to the given centres."""
    an = anchors_cs()
    for a, (cy, cx) in zip(anchor_ids, centres):
        assert not be[a].any()
        be[a, 0] = F32(10.0 * (cy - float(an[a][0])) / float(an[a][2]))
        be[a, 1] = F32(10.0 * (cx - float(an[a][1])) / float(an[a][3]))


def ladder_frame(kind: str, thr: float = post.IOU_THRESHOLD, outside: bool = False) -> Tuple[np.ndarray, np.ndarray, dict]:
    """(be, lg, info) of one ladder frame; info: chains = [(class column, [anchor ids in score order])], expect_kept = per chain the
    members greedy NMS keeps before the 100-row cut is applied (every other one), plus what the kind adds.
      long         (a ladder alone stops at 100 kept rows, i.e. at member 200 and sorted position 200, so a cluster pushes the chain over
                   position 256:) a cluster of 130 boxes of ANOTHER class on one spot at the top of the order (one survivor), then a ladder of 200: its
                   members 126 .. 127 straddle sorted position 256, the border between the walk's chunks, with 64 rows kept by then
      single_bin   100 members FINE_STEP apart in logit, all scores inside the bin [0.5, 0.5625)
      bands        150 members 0.08 apart in logit: scores from 0.98 down to 3e-4, across 90 score bins
      interleaved  two classes' ladders of 90 on the SAME boxes, their scores interleaved
    outside: the chain starts above and left of the image (negative coordinates; a clip-after engine walks the boxes as decoded)."""
    be, lg = blank()
    d = ladder_step(thr)
    y0, x0 = (-0.12, -0.05) if outside else (0.1, 0.08)
    info: dict = dict(kind=kind, d=d, chains=[])
    if kind == "long":
        n = 200
        cluster = [a + 1 for a in SQUARES[:130]]                  # the 0.2-scale wide anchors of the same locations
        place(be, cluster, [(0.5, 0.5)] * len(cluster))
        for k, a in enumerate(cluster):
            lg[a, 7] = F32(9.9 - k * LOGIT_STEP)
        info["cluster"] = (7, cluster)
        cols, top, step = [3], 2.0, LOGIT_STEP
    elif kind == "single_bin":
        n, cols, top, step = 100, [3], 0.22, FINE_STEP
    elif kind == "bands":
        n, cols, top, step = 150, [3], 4.0, 0.08
    elif kind == "interleaved":
        n, cols, top, step = 90, [3, 60], 4.0, 0.1
    else:
        raise ValueError(kind)
    ids = SQUARES[:n]
    place(be, ids, snake(n, d, y0, x0))
    for c, col in enumerate(cols):
        for k, a in enumerate(ids):
            lg[a, col] = F32(top - k * step - c * step / 2)
        info["chains"].append((col, list(ids)))
    return be, lg, info


def chain_properties(be: np.ndarray, ids, thr: float, clip: bool = True) -> Tuple[float, float]:
    """(the smallest IoU of neighbours, the largest IoU of any two members that are not neighbours) of a chain, from the oracle's iou."""
    boxes = decode(be)[list(ids)]
    if clip:
        boxes = post.clip_to_unit_window(boxes)
    n = len(ids)
    lo, hi = 1.0, 0.0
    for k in range(n):
        q = post.iou_many(boxes[k], boxes)
        if k + 1 < n:
            lo = min(lo, float(q[k + 1]))
        far = np.ones(n, bool)
        far[max(k - 1, 0):k + 2] = False
        if far.any():
            hi = max(hi, float(q[far].max()))
    return lo, hi
