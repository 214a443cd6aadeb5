"""CPU restatement of the motion hold (include/watsor_hip.h: wz_set_camera_motion_hold; csrc/k_motion.hip) on top of
motion_oracle, equal to the engine in every integer.  G is the camera's grid of ages, uint8 [gh, gw] over motion_oracle's cells.

    active(C, G)                                 -> A = C or (G > 0)
    decay(G, C, hold)                            -> G1 = max(hold if C else 0, G - 1 if G > 0 else 0)
    stamp(age, rows, passes, W, H, object_hold)  -> G2: every cell under a row whose pass byte is 1 raised to object_hold
    step(now, ref, G, W, H, fmt, thr, hold, ...) -> (rectangles, their n, components, active, held, G1): one region launch
    HoldState(W, H, fmt, thr, hold, object_hold) .begin(frame) -> (tile list, n, components, active, held); .finish(rows, passes); .reset()
"""
import numpy as np

import gate_oracle as go
import motion_oracle as mo

CELL_SHIFT = 4
assert 1 << CELL_SHIFT == mo.CELL


def active(C: np.ndarray, G: np.ndarray) -> np.ndarray:
    return C | (G > 0)


def decay(G: np.ndarray, C: np.ndarray, hold: int) -> np.ndarray:
    older = np.where(G > 0, G.astype(np.int64) - 1, 0)
    return np.maximum(np.where(C, int(hold), 0), older).astype(np.uint8)


def stamp(age: np.ndarray, rows, passes, W: int, H: int, object_hold: int) -> np.ndarray:
    """rows: 100 records with x_min, y_min, x_max, y_max (runtime.ROW_DTYPE); passes: their 100 pass bytes"""
    out = np.array(age, np.uint8)
    if object_hold == 0:
        return out
    for row, ok in zip(rows, passes):
        if int(ok) != 1:
            continue
        x0, x1 = max(int(row["x_min"]), 0), min(int(row["x_max"]), W - 1)
        y0, y1 = max(int(row["y_min"]), 0), min(int(row["y_max"]), H - 1)
        if x0 > x1 or y0 > y1:
            continue
        box = out[y0 >> CELL_SHIFT:(y1 >> CELL_SHIFT) + 1, x0 >> CELL_SHIFT:(x1 >> CELL_SHIFT) + 1]
        np.maximum(box, object_hold, out=box)
    return out


def step(now, ref, G, W: int, H: int, fmt: int, threshold: int, hold: int, **kw):
    """what one region launch of a camera with a hold reports and leaves; G None: all zero"""
    C = mo.changed(now, ref, W, H, threshold)
    G = np.zeros(C.shape, np.uint8) if G is None else np.asarray(G, np.uint8)
    A = active(C, G)
    rects, cells, comps = mo.regions_of(A, W, H, fmt, **kw)
    return rects, cells, comps, int(A.sum()), int((A & ~C).sum()), decay(G, C, hold)


class HoldState:
    """One camera with a hold: motion_oracle.MotionState plus the ages.  begin() is the call up to its tile list and changes nothing;
    finish() is what an ACCEPTED call leaves behind (a refused call never gets there)."""

    def __init__(self, W: int, H: int, fmt: int, threshold: int, hold: int, object_hold: int, whole_frame: bool = True, **motion_kw):
        assert 0 <= hold <= 255 and 0 <= object_hold <= 255 and (hold or object_hold)
        self.W, self.H, self.fmt, self.threshold, self.whole_frame, self.kw = W, H, fmt, int(threshold), bool(whole_frame), motion_kw
        self.hold, self.object_hold = int(hold), int(object_hold)
        self.reset()

    def reset(self):
        self.ref = None
        self.G = np.zeros(mo.grid_shape(self.W, self.H), np.uint8)
        self._pending = None

    def begin(self, frame):
        """-> (tile list, the regions' n, components, active, held)"""
        now = go.cell_sums(frame, self.W, self.H, self.fmt, (0, 0, self.W, self.H))
        rects, cells, comps, act, held, G1 = step(now, self.ref, self.G, self.W, self.H, self.fmt, self.threshold, self.hold, **self.kw)
        self._pending = (now, G1)
        return ([(0, 0, self.W, self.H)] if self.whole_frame else []) + rects, cells, comps, act, held

    def finish(self, rows, passes):
        now, G1 = self._pending
        self.G = stamp(G1, rows, passes, self.W, self.H, self.object_hold)
        self.ref, self._pending = now, None
