"""Class heads that look trained, for ANY arch.Program (test infrastructure, beside trained_like.py which spreads the activations).

The seeded synthetic weights give every class logit the same distribution: bias logit(0.01), a narrow spread, ~170 scores above 0.3 in
a handful of classes and never a tie.  `trained_heads` rewrites the ClassPredictor variables of the program's head ops -- nothing else,
so every activation tensor and every box encoding is that of the seeded weights:

  bias      every class column gets CLASS_BIAS (negative: most scores are tiny), the background column BACKGROUND_BIAS (positive)
  gain      the class weights are multiplied by GAIN: the logits of a frame run from below logit(1e-6) to above logit(0.9)
  hot       HOT columns -- one (anchor of the location, class) each of head HOT_HEAD -- take HOT_GAIN on top: some of their logits
            exceed 17, where sigmoid is 1.0f exactly and only the anchor index orders the candidates
  dead      the DEAD classes' columns (every head, every anchor of a location) have all-zero weights and the one bias DEAD_BIAS: one
            logit at all 1917 anchors, len(DEAD) x 1917 equal scores in ONE score bin (the top 12 bits of the float) -- more than the
            NMS kernel's candidate list holds (WZ_CAND_CAP = 4096), so whoever walks down to that bin takes the exact serial walk

Who walks down to it depends on the frame.  The seeded network's features move with the input by about half of their spread, so a
frame of noise has 140 .. 160 NMS survivors above the dead bin and keeps its 100 rows without touching it (the busy scene), while a
constant frame has 50 .. 70 and has to take the rest from the dead bin (the quiet, or dead-column, scene: fewer than 100 candidates
above 0.3).  A synthetic frame lies between the two (100 .. 125 survivors): good for the rows, not for forcing a regime.

A head column is (anchor of the location) * 91 + class, class 0 the background (arch.py: OUT_HEAD).  The numbers were tuned on the CPU
against the fp32 oracle network; tests/test_trained_like_heads_cpu.py asserts the populations they give.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from watsor_amd import arch

NUM_COLS = 91
CLASS_BIAS = -8.2
BACKGROUND_BIAS = 4.0
GAIN = 2.0
HOT_GAIN = 30.0
HOT = 3                      # columns
HOT_HEAD = 1                 # ... of this head (the 10 x 10 map: large anchors, so the NMS keeps few of a column's candidates)
DEAD = (11, 37, 52, 64, 83)  # classes (columns 1 .. 90)
DEAD_BIAS = -1.02            # sigmoid = 0.265, bin [0.25, 0.28125): a busy frame keeps its 100 rows above it, a quiet one has to walk it
WZ_CAND_CAP = 4096           # csrc/wz_common.h
WZ_HIST_BINS = 1024


def head_ops(prog: "arch.Program") -> List["arch.Op"]:
    return [op for op in prog.ops if op.out_mode == arch.OUT_HEAD]


def hot_columns(prog: "arch.Program", seed: int) -> List[Tuple[str, int]]:
    """(head scope, column) of the HOT columns: drawn from the first two heads (the large maps), never a dead class or the background."""
    rng = np.random.Generator(np.random.PCG64([int(seed), 4242]))
    op = head_ops(prog)[HOT_HEAD]
    out = []
    while len(out) < HOT:
        a = len(out) % op.anchors_per_loc
        c = int(rng.integers(1, NUM_COLS))
        if c in DEAD or (op.scope, a * NUM_COLS + c) in out:
            continue
        out.append((op.scope, a * NUM_COLS + c))
    return out


def trained_heads(weights: Dict[str, np.ndarray], prog: "arch.Program", seed: int) -> Dict[str, np.ndarray]:
    """A copy of `weights` with the ClassPredictor variables of `prog`'s heads rewritten as the module docstring says."""
    W = dict(weights)
    hot = hot_columns(prog, seed)
    for op in head_ops(prog):
        wn, bn = op.scope + "/ClassPredictor/weights", op.scope + "/ClassPredictor/biases"
        w = np.asarray(weights[wn], np.float32).copy()
        cols = w.shape[3]
        assert cols == op.anchors_per_loc * NUM_COLS
        cls = np.arange(cols) % NUM_COLS
        w *= np.float32(GAIN)
        for scope, col in hot:
            if scope == op.scope:
                w[..., col] *= np.float32(HOT_GAIN)
        b = np.where(cls == 0, BACKGROUND_BIAS, CLASS_BIAS).astype(np.float32)
        dead = np.isin(cls, DEAD)
        w[..., dead] = 0.0
        b[dead] = DEAD_BIAS
        W[wn], W[bn] = w, b
    return W


def score_bins(scores: np.ndarray) -> np.ndarray:
    """The NMS kernel's score bin of float32 scores: the top 12 bits of the float."""
    return (np.ascontiguousarray(scores, np.float32).view(np.uint32) >> np.uint32(20)).astype(np.int64)


def dead_bin() -> int:
    from oracle.postprocess import sigmoid
    return int(score_bins(sigmoid(np.float32([DEAD_BIAS])))[0])


def populations(logits: np.ndarray) -> dict:
    """What the CPU test asserts, of ONE frame's logits [A, 91]: candidates above 0.3, scores exactly 1.0, the smallest and the largest
    class score, and the most crowded score bin with its population."""
    from oracle.postprocess import sigmoid
    s = sigmoid(np.asarray(logits, np.float32))[:, 1:]
    hist = np.bincount(score_bins(s).ravel(), minlength=WZ_HIST_BINS)
    return dict(above_03=int((s > 0.3).sum()), ones=int((s == 1.0).sum()), smin=float(s.min()), smax=float(s.max()),
                top_bin=int(hist.argmax()), top_bin_count=int(hist.max()), hist=hist)


def frame_kinds(seed: int, width: int = 300, height: int = 300) -> Dict[str, np.ndarray]:
    """The frame kinds of the op-conformance module as uint8 RGB frames: a synthetic frame, noise (the busy scene), a constant frame
    (the quiet scene; away from the border every location of a shallow layer ties)."""
    from watsor_amd.synth import synthetic_frame
    rng = np.random.Generator(np.random.PCG64([int(seed), 99]))
    return dict(synthetic=synthetic_frame(width, height, 9500 + seed),
                noise=rng.integers(0, 256, (height, width, 3), dtype=np.uint8),
                constant=np.full((height, width, 3), (128, 40, 220)[seed % 3], np.uint8))
