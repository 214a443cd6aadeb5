"""CPU restatement of motion regions (include/watsor_hip.h: wz_set_camera_motion / wz_detect_motion; csrc/k_motion.hip; DESIGN.md section
19), equal to the engine in every integer: numpy / Python integers only.  Luma, cells and cell sums are gate_oracle's.

    changed(now, ref, W, H, thr)                 -> C, bool [gh, gw]; ref None: all False
    dilated(C, d)                                -> D
    components(D)                                -> int [gh, gw]: the component's id (smallest linear index) of every D cell, -1 elsewhere
    candidates(C, D, min_cells)                  -> [(n, id, cx0, cx1, cy0, cy1), ...] ranked; all of them (the walk looks at CANDIDATES)
    walk(cands, W, H, fmt, ...)                  -> ([(x0, y0, w, h), ...], [n, ...])
    regions(now, ref, W, H, fmt, ...)            -> (rectangles, their n, components with n >= min_cells)
    MotionState(W, H, fmt, ...).step(frame)      -> the frame's tile list, replaying the reference
"""
from collections import deque

import numpy as np

import gate_oracle as go

CELL = go.CELL
CANDIDATES = 64
MAX_REGIONS = 16
MAX_CELLS = 32768
DEFAULTS = dict(min_cells=1, dilate=1, max_regions=3, min_side=300, pad=8)


def grid_shape(W: int, H: int):
    return -(-H // CELL), -(-W // CELL)


def changed(now, ref, W: int, H: int, thr: int) -> np.ndarray:
    if ref is None:
        return np.zeros(grid_shape(W, H), bool)
    return go.changed_cells(now, ref, (0, 0, W, H), thr)


def dilated(C: np.ndarray, d: int) -> np.ndarray:
    gh, gw = C.shape
    D = np.zeros_like(C, dtype=bool)
    for y, x in zip(*np.nonzero(C)):
        D[max(0, y - d):min(gh, y + d + 1), max(0, x - d):min(gw, x + d + 1)] = True
    return D


def components(D: np.ndarray) -> np.ndarray:
    """8-connected components by breadth-first search in raster order: the first cell of a component met is its smallest linear index"""
    gh, gw = D.shape
    ids = np.full((gh, gw), -1, np.int64)
    for y0, x0 in zip(*np.nonzero(D)):
        if ids[y0, x0] >= 0:
            continue
        cid = int(y0) * gw + int(x0)
        ids[y0, x0] = cid
        todo = deque([(int(y0), int(x0))])
        while todo:
            y, x = todo.popleft()
            for yy in range(max(0, y - 1), min(gh, y + 2)):
                for xx in range(max(0, x - 1), min(gw, x + 2)):
                    if D[yy, xx] and ids[yy, xx] < 0:
                        ids[yy, xx] = cid
                        todo.append((yy, xx))
    return ids


def candidates(C: np.ndarray, D: np.ndarray, min_cells: int):
    ids = components(D)
    out = []
    for cid in np.unique(ids[ids >= 0]):
        ys, xs = np.nonzero(ids == cid)
        n = int(C[ys, xs].sum())                      # dilated cells do not count
        if n >= min_cells:
            out.append((n, int(cid), int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())))
    return sorted(out, key=lambda c: (-c[0], c[1]))


def even_axes(fmt: int):
    """(x, y): the format cuts at even pixels only"""
    base = fmt & 0xFF
    planar = base in (1, 2, 0x10, 0x11)
    return planar or base in (3, 4), planar


def _axis(a0: int, a1: int, size: int, min_side: int, even: bool):
    m = min(min_side, size)
    d = m - (a1 - a0)
    if d > 0:
        a0 -= d // 2
        a1 += d - d // 2
        if a0 < 0:
            a1 -= a0
            a0 = 0
        if a1 > size:
            a0 -= a1 - size
            a1 = size
    if even:
        a0 -= a0 & 1
        a1 = min(size, a1 + (a1 & 1))
    return a0, a1


def walk(cands, W: int, H: int, fmt: int, max_regions: int, min_side: int, pad: int):
    rects, cells = [], []
    ex, ey = even_axes(fmt)
    for n, _, cx0, cx1, cy0, cy1 in cands[:CANDIDATES]:
        if len(rects) >= max_regions:
            break
        x0, x1 = max(0, CELL * cx0 - pad), min(W, min(W, CELL * (cx1 + 1)) + pad)
        y0, y1 = max(0, CELL * cy0 - pad), min(H, min(H, CELL * (cy1 + 1)) + pad)
        if any(ax <= x0 and x1 <= ax + aw and ay <= y0 and y1 <= ay + ah for ax, ay, aw, ah in rects):
            continue                                  # a region already accepted shows it
        x0, x1 = _axis(x0, x1, W, min_side, ex)
        y0, y1 = _axis(y0, y1, H, min_side, ey)
        rects.append((x0, y0, x1 - x0, y1 - y0))
        cells.append(n)
    return rects, cells


def regions_of(C: np.ndarray, W: int, H: int, fmt: int = 0, min_cells=1, dilate=1, max_regions=3, min_side=300, pad=8):
    """(rectangles, their n, components with n >= min_cells) of a grid of changed cells"""
    cands = candidates(C, dilated(C, dilate), min_cells)
    rects, cells = walk(cands, W, H, fmt, max_regions, min_side, pad)
    return rects, cells, len(cands)


def regions(now, ref, W: int, H: int, fmt: int, threshold: int, **kw):
    return regions_of(changed(now, ref, W, H, threshold), W, H, fmt, **kw)


class MotionState:
    """One camera: the reference is the grid of the previous step, replaced on every step."""

    def __init__(self, W: int, H: int, fmt: int, threshold: int, whole_frame: bool = True, **kw):
        self.W, self.H, self.fmt, self.threshold, self.whole_frame, self.kw = W, H, fmt, int(threshold), bool(whole_frame), kw
        self.ref = None

    def reset(self):
        self.ref = None

    def step(self, frame):
        """-> (tile list, the regions' n, components)"""
        now = go.cell_sums(frame, self.W, self.H, self.fmt, (0, 0, self.W, self.H))
        rects, cells, comps = regions(now, self.ref, self.W, self.H, self.fmt, self.threshold, **self.kw)
        self.ref = now
        return ([(0, 0, self.W, self.H)] if self.whole_frame else []) + rects, cells, comps


# ---- grids for tests: what a change looks like in luma sums ------------------------------------------------------------------------------
def grids_for(C: np.ndarray, W: int, H: int, thr: int):
    """(now, ref) with ref = 0 and now = thr * npix + 1 where C wants a change, thr * npix where it does not (the largest sum that is none)"""
    npix = go.cell_pixels((0, 0, W, H))
    assert C.shape == npix.shape and thr * CELL * CELL + 1 <= 65535
    return (thr * npix + C.astype(np.int64)).astype(np.uint16), np.zeros(C.shape, np.uint16)


def serpentine(gh: int, gw: int) -> np.ndarray:
    """a one-cell-wide path: every second row is full, the rows between hold one cell at alternating ends"""
    C = np.zeros((gh, gw), bool)
    C[0::2] = True
    for k, y in enumerate(range(1, gh, 2)):
        C[y, gw - 1 if k % 2 == 0 else 0] = True
    return C


def comb(gh: int, gw: int) -> np.ndarray:
    """a full last row with teeth on every second column: components that join only at the end of a raster scan"""
    C = np.zeros((gh, gw), bool)
    C[:, 0::2] = True
    C[gh - 1] = True
    return C
