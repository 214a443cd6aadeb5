"""CPU restatement of gated tiled detection (include/watsor_hip.h: wz_set_camera_tiles / wz_detect_gated; csrc/k_gate.hip), bit-equal to
the engine: numpy / Python integers only.

    luma(frame, w, h, fmt)                    -> uint8 [h, w], on the bytes as stored (colour flags play no part)
    cell_sums(frame, w, h, fmt, rect)         -> uint16 [cell rows, cell columns] of rectangle (x0, y0, tw, th)
    activity(now, ref, rect, pixel_thr)       -> cells with |S_now - S_ref| > pixel_thr * (pixels of the cell)
    GateState(n_tiles, min_cells, max_age)    -> replays which tiles run
"""
import numpy as np

CELL = 16


def luma(frame, w: int, h: int, fmt: int) -> np.ndarray:
    """Base formats: 0 RGB24, 1 NV12, 2 I420, 3 YUYV422, 4 UYVY422, 5 GRAY8, 6 BGR24.  NV12 / I420: the luma plane (chroma is not read)."""
    buf = np.asarray(frame, np.uint8).reshape(-1)
    base = fmt & 0xFF
    if base in (1, 2, 5):
        return buf[:w * h].reshape(h, w).copy()
    if base in (3, 4):
        return buf[:w * h * 2].reshape(h, w, 2)[:, :, 0 if base == 3 else 1].copy()
    px = buf[:w * h * 3].reshape(h, w, 3).astype(np.int64)
    r, g, b = (px[:, :, 0], px[:, :, 1], px[:, :, 2]) if base == 0 else (px[:, :, 2], px[:, :, 1], px[:, :, 0])
    return ((77 * r + 150 * g + 29 * b + 128) >> 8).astype(np.uint8)


def grid_shape(rect):
    return -(-rect[3] // CELL), -(-rect[2] // CELL)


def cell_pixels(rect) -> np.ndarray:
    """pixels of every cell of the rectangle: the last column and row of cells are partial"""
    rows, cols = grid_shape(rect)
    ch = np.minimum(CELL, rect[3] - CELL * np.arange(rows))
    cw = np.minimum(CELL, rect[2] - CELL * np.arange(cols))
    return np.outer(ch, cw).astype(np.int64)


def cell_sums(frame, w: int, h: int, fmt: int, rect) -> np.ndarray:
    x0, y0, tw, th = rect
    y = luma(frame, w, h, fmt)[y0:y0 + th, x0:x0 + tw].astype(np.int64)
    rows, cols = grid_shape(rect)
    padded = np.zeros((rows * CELL, cols * CELL), np.int64)
    padded[:th, :tw] = y
    sums = padded.reshape(rows, CELL, cols, CELL).sum(axis=(1, 3))
    assert sums.max() <= 255 * CELL * CELL
    return sums.astype(np.uint16)


def changed_cells(now, ref, rect, pixel_thr: int) -> np.ndarray:
    d = np.abs(np.asarray(now, np.uint16).astype(np.int64) - np.asarray(ref, np.uint16).astype(np.int64))
    return d > int(pixel_thr) * cell_pixels(rect)


def activity(now, ref, rect, pixel_thr: int) -> int:
    return int(changed_cells(now, ref, rect, pixel_thr).sum())


class GateState:
    """Which tiles of one camera run.  A tile runs iff it has no reference, or its activity >= min_cells, or max_age > 0 and it was
    skipped in the last max_age consecutive calls.  Its reference is replaced only when it runs."""

    def __init__(self, n_tiles: int, pixel_thr: int, min_cells: int = 1, max_age: int = 0):
        self.n, self.pixel_thr, self.min_cells, self.max_age = int(n_tiles), int(pixel_thr), int(min_cells), int(max_age)
        self.reset()

    def reset(self):
        self.ref = [None] * self.n
        self.skipped = [0] * self.n

    def step(self, grids, rects):
        """grids[t] = cell_sums of tile t in the new frame -> (the tiles that run, every tile's activity; 0 without a reference)"""
        ran, acts = [], []
        for t in range(self.n):
            act = 0 if self.ref[t] is None else activity(grids[t], self.ref[t], rects[t], self.pixel_thr)
            acts.append(act)
            if self.ref[t] is None or act >= self.min_cells or (self.max_age > 0 and self.skipped[t] >= self.max_age):
                ran.append(t)
                self.ref[t] = np.array(grids[t], np.uint16)
                self.skipped[t] = 0
            else:
                self.skipped[t] += 1
        return ran, acts
