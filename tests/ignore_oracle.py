"""CPU restatement of ignore masks (include/watsor_hip.h: wz_ignore_cells / wz_set_camera_ignore; csrc/wz_ignore.cpp, k_motion.hip, k_gate.hip;
DESIGN.md section 19c) on top of the three oracles it touches, which stay as they are: numpy / Python integers only.
    cells(mask, rect=None)                        -> M, bool [cell rows, cell columns] of the rectangle (None: the whole frame): a cell is
                                                     ignored iff at least one of its pixels is
    regions(now, ref, M, W, H, fmt, thr, ...)     -> (rectangles, their n, components, ignored): motion_oracle.regions_of on C & ~M
    hold_step(now, ref, G, M, W, H, fmt, thr, hold, ...) -> motion_hold_oracle.step with C & ~M in the place of C, + ignored
    activity(now, ref, M, rect, thr)              -> the tile's changed cells that are not ignored
    IgnoreMotionState / IgnoreGateState           -> motion_oracle.MotionState / gate_oracle.GateState of a camera with a mask
"""
import numpy as np

import gate_oracle as go
import motion_hold_oracle as mho
import motion_oracle as mo

CELL = go.CELL


def cells(mask, rect=None) -> np.ndarray:
    mask = np.asarray(mask)
    assert mask.ndim == 2
    H, W = mask.shape
    x0, y0, w, h = (0, 0, W, H) if rect is None else rect
    assert w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= W and y0 + h <= H
    rows, cols = go.grid_shape((x0, y0, w, h))
    padded = np.zeros((rows * CELL, cols * CELL), bool)
    padded[:h, :w] = mask[y0:y0 + h, x0:x0 + w] != 0
    return padded.reshape(rows, CELL, cols, CELL).any(axis=(1, 3))


def regions(now, ref, M, W: int, H: int, fmt: int, threshold: int, **kw):
    """what one region launch of a camera with a mask (and no hold) reports; M None: no mask"""
    C = mo.changed(now, ref, W, H, threshold)
    M = np.zeros(C.shape, bool) if M is None else np.asarray(M, bool)
    return mo.regions_of(C & ~M, W, H, fmt, **kw) + (int((C & M).sum()),)


def hold_step(now, ref, G, M, W: int, H: int, fmt: int, threshold: int, hold: int, **kw):
    """motion_hold_oracle.step of a camera with a mask: (rectangles, their n, components, active, held, G1, ignored)"""
    C = mo.changed(now, ref, W, H, threshold)
    M = np.zeros(C.shape, bool) if M is None else np.asarray(M, bool)
    G = np.zeros(C.shape, np.uint8) if G is None else np.asarray(G, np.uint8)
    C1 = C & ~M
    A = mho.active(C1, G)
    rects, n, comps = mo.regions_of(A, W, H, fmt, **kw)
    return rects, n, comps, int(A.sum()), int((A & ~C1).sum()), mho.decay(G, C1, hold), int((C & M).sum())


def activity(now, ref, M, rect, pixel_thr: int) -> int:
    C = go.changed_cells(now, ref, rect, pixel_thr)
    return int((C & ~np.asarray(M, bool)).sum()) if M is not None else int(C.sum())


class IgnoreMotionState:
    """One motion camera without a hold and with the ignore plane `mask` (None: no mask)."""

    def __init__(self, W: int, H: int, fmt: int, threshold: int, mask, whole_frame: bool = True, **kw):
        self.W, self.H, self.fmt, self.threshold, self.whole_frame, self.kw = W, H, fmt, int(threshold), bool(whole_frame), kw
        self.M = None if mask is None else cells(mask)
        self.ref = None

    def reset(self):
        self.ref = None

    def step(self, frame):
        """-> (tile list, the regions' n, components, ignored)"""
        now = go.cell_sums(frame, self.W, self.H, self.fmt, (0, 0, self.W, self.H))
        rects, n, comps, ignored = regions(now, self.ref, self.M, self.W, self.H, self.fmt, self.threshold, **self.kw)
        self.ref = now                      # (ignored cells included: the whole grid becomes the reference)
        return ([(0, 0, self.W, self.H)] if self.whole_frame else []) + rects, n, comps, ignored


class IgnoreGateState(go.GateState):
    """gate_oracle.GateState whose activity leaves out every tile's ignored cells: masks[t] = cells(mask, rects[t])"""

    def __init__(self, rects, mask, pixel_thr: int, min_cells: int = 1, max_age: int = 0):
        super().__init__(len(rects), pixel_thr, min_cells, max_age)
        self.masks = [None if mask is None else cells(mask, r) for r in rects]

    def step(self, grids, rects):
        ran, acts = [], []
        for t in range(self.n):
            act = 0 if self.ref[t] is None else activity(grids[t], self.ref[t], self.masks[t], rects[t], self.pixel_thr)
            acts.append(act)
            if self.ref[t] is None or act >= self.min_cells or (self.max_age > 0 and self.skipped[t] >= self.max_age):
                ran.append(t)
                self.ref[t] = np.array(grids[t], np.uint16)
                self.skipped[t] = 0
            else:
                self.skipped[t] += 1
        return ran, acts
