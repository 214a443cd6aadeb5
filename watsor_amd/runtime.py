"""Thin Python handle around one `wz_engine_t` (one MI355X).  numpy in, numpy / ctypes rows out.

Used by the detector plugin (`watsor_amd/detection/hip_gpu.py`), by `bench.py` and by the parity
tests.  No torch here: device memory, streams and graphs are owned by libwatsor_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, List, Optional, Sequence

import numpy as np

from . import _lib
from .share import Detection, DetectionArray, MAX_DETECTIONS

ROW_DTYPE = np.dtype([("label", "<i4"), ("zones", "<i4", (10,)), ("_pad", "<i4"), ("confidence", "<f8"),
                      ("x_min", "<i4"), ("y_min", "<i4"), ("x_max", "<i4"), ("y_max", "<i4")])
assert ROW_DTYPE.itemsize == C.sizeof(Detection) == 72
FMT_RGB24, FMT_NV12, FMT_I420 = _lib.WZ_FMT_RGB24, _lib.WZ_FMT_NV12, _lib.WZ_FMT_I420   # pixel formats of a frame (include/watsor_hip.h)
FMT_YUYV422, FMT_UYVY422, FMT_GRAY8, FMT_BGR24 = _lib.WZ_FMT_YUYV422, _lib.WZ_FMT_UYVY422, _lib.WZ_FMT_GRAY8, _lib.WZ_FMT_BGR24
# 10-bit 4:2:0, a little-endian 16-bit word per sample: P010 (ffmpeg's p010le: the sample in the word's high bits) and YUV420P10
# (yuv420p10le: in its low bits).  3*W*H bytes, as many as RGB24: what they save is the host's conversion, not bytes.
FMT_P010, FMT_YUV420P10 = _lib.WZ_FMT_P010, _lib.WZ_FMT_YUV420P10
TEN_BIT_FORMATS = (FMT_P010, FMT_YUV420P10)
# a frame's format WORD is one of the above or'ed with colour flags (the YUV formats only): BT.709 matrix instead of BT.601,
# full range (ffmpeg's yuvj*) instead of limited
CSP_BT709, RANGE_FULL, FMT_BASE_MASK = _lib.WZ_CSP_BT709, _lib.WZ_RANGE_FULL, _lib.WZ_FMT_BASE_MASK
YUV_FORMATS = (FMT_NV12, FMT_I420, FMT_YUYV422, FMT_UYVY422, FMT_P010, FMT_YUV420P10)


def frame_shape(base: int, rows: int, cols: int, channels: Optional[int], itemsize: int):
    """(width, height) of a `rows` x `cols` array with `channels` items of `itemsize` bytes per position (None: the array has no channel
    axis -- not 0, which is an empty array and no frame) read as a frame of base format `base`, or None when that shape is no frame of it.  The one rule behind `HipEngine.frame_geometry`
    (arrays) and the plugin's frame table (frame buffers).  RGB24 / BGR24: (H, W, 3).  GRAY8: (H, W[, 1]).  YUYV422 / UYVY422: (H, W, 2)
    or (H, 2W), W even.  NV12 / I420: the planar view (H*3/2, W[, 1]), H and W even.  P010 / YUV420P10: the planar view in 16-bit words,
    (H*3/2, W[, 1]), or its bytes, (H*3/2, W, 2) or (H*3/2, 2W[, 1]); 16-bit items are these two formats' only."""
    if itemsize != 1 and not (itemsize == 2 and base in TEN_BIT_FORMATS):
        return None
    flat = channels is None or channels == 1
    if base in (FMT_RGB24, FMT_BGR24):
        return (cols, rows) if channels == 3 else None
    if base == FMT_GRAY8:
        return (cols, rows) if flat else None
    if base in (FMT_YUYV422, FMT_UYVY422):
        if channels == 2 and cols % 2 == 0:
            return cols, rows
        return (cols // 2, rows) if channels is None and cols % 4 == 0 else None
    if base in TEN_BIT_FORMATS:
        if itemsize == 1 and flat and cols % 2 == 0:
            cols //= 2                                   # two bytes a word
        elif not (flat if itemsize == 2 else channels == 2):
            return None
    elif base not in (FMT_NV12, FMT_I420) or not flat:
        return None
    if rows % 3 or (rows // 3 * 2) % 2 or cols % 2:      # 4:2:0: H rows of luma, H/2 of chroma
        return None
    return cols, rows // 3 * 2


_FRAME_SHAPES = {   # what `HipEngine.frame_geometry` says of an array that is no frame of its format
    **dict.fromkeys((FMT_RGB24, FMT_BGR24), "an RGB24 / BGR24 frame must be (H,W,3) uint8"),
    **dict.fromkeys((FMT_NV12, FMT_I420), "an NV12 / I420 frame must be (H*3/2, W) uint8 with even H and W"),
    **dict.fromkeys((FMT_YUYV422, FMT_UYVY422), "a YUYV422 / UYVY422 frame must be (H,W,2) or (H,2W) uint8 with even W"),
    **dict.fromkeys(TEN_BIT_FORMATS, "a P010 / YUV420P10 frame must be (H*3/2, W) uint16, or (H*3/2, W, 2) or (H*3/2, 2W) uint8, with even H and W"),
    FMT_GRAY8: "a GRAY8 frame must be (H,W) or (H,W,1) uint8",
}


def device_count() -> int:
    return int(_lib.load().wz_device_count())


def hw_queues(dev: bool = False) -> int:
    """GPU_MAX_HW_QUEUES in the C environment after the library loaded (include/watsor_hip.h: wz_hw_queues; 0: not a number): the
    library raises anything below 8 to 8, and an engine wants two per lane."""
    return int(_lib.load(dev=dev).wz_hw_queues())


SCHEDULES = {"throughput": _lib.WZ_SCHEDULE_THROUGHPUT, "latency": _lib.WZ_SCHEDULE_LATENCY}


def set_schedule(name: str, dev: bool = False) -> None:
    """The process's schedule (include/watsor_hip.h: wz_set_schedule): "latency" | "throughput".  Before its first engine; afterwards
    only the schedule already in force is accepted (ValueError otherwise)."""
    try:
        code = SCHEDULES[str(name).lower()]
    except KeyError:
        raise ValueError("schedule %r: expected one of %s" % (name, ", ".join(sorted(SCHEDULES)))) from None
    lib = _lib.load(dev=dev)
    _lib.check(lib.wz_set_schedule(code), "wz_set_schedule", lib)


def get_schedule(dev: bool = False) -> str:
    """The schedule in force ("latency" | "throughput"); asking fixes it (WZ_SCHEDULE in the environment, else throughput)."""
    code = _lib.load(dev=dev).wz_get_schedule()
    return next(k for k, v in SCHEDULES.items() if v == code)


def device_name(device: int) -> str:
    buf = C.create_string_buffer(256)
    _lib.check(_lib.load().wz_device_name_of(device, buf, 256))
    return buf.value.decode()


def _i32(n: int, values):
    """An optional per-frame argument (formats, camera ids) as an int32 array of n, None as NULL."""
    return (C.c_int32 * n)(*[int(v) for v in values]) if values is not None else None


class Tile(C.Structure):
    """`wz_tile_t`: a rectangle of a frame, in pixels."""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


def tile_grid(width: int, height: int, cols: int, rows: int, overlap: float = 0.0, full_frame: bool = True, even: bool = False):
    """The rectangles [(x0, y0, w, h), ...] of a cols x rows grid over a width x height frame, row by row.  The frame is split into cells
    of ceil(width / cols) x ceil(height / rows) pixels (the last column / row takes what is left); every cell then grows by half of
    `overlap` times the cell size on each side, clipped to the frame, so that neighbours share `overlap` of a tile.  even=True: origins
    and sizes are even numbers (what NV12 / I420 tiles need, and the 4:2:2 formats in x).  full_frame=True: the whole frame is one more
    tile, the last one -- the tile that sees the objects larger than a cell."""
    width, height, cols, rows, overlap = int(width), int(height), int(cols), int(rows), float(overlap)
    if width < 1 or height < 1 or cols < 1 or rows < 1:
        raise ValueError("tile_grid: width, height, cols and rows must be positive")
    if not 0.0 <= overlap < 1.0:
        raise ValueError("tile_grid: overlap %r, expected 0 <= overlap < 1" % (overlap,))
    if even:
        width, height = width & ~1, height & ~1
        if width < 2 or height < 2:
            raise ValueError("tile_grid: no even rectangle fits the frame")

    def spans(size, parts):
        cell = -(-size // parts)
        grow = int(np.ceil(overlap * cell / 2.0))
        if even:
            cell, grow = cell + (cell & 1), grow + (grow & 1)
        return [(max(0, a - grow), min(size, a + cell + grow)) for a in range(0, size, cell)][:parts]

    out = [(x0, y0, x1 - x0, y1 - y0) for y0, y1 in spans(height, rows) for x0, x1 in spans(width, cols)]
    if full_frame and (0, 0, width, height) not in out:
        out.append((0, 0, width, height))
    return out


class HipEngine:
    def __init__(self, engine_path: str, device: int = 0, max_batch: int = 8, max_width: int = 1920,
                 max_height: int = 1080, dev: Optional[bool] = None, schedule: Optional[str] = None):
        """dev=True: on the DEVELOPMENT library (libwatsor_hip_dev.so: stage-level entry points, per-kernel profiling, the WZ_*
        tuning knobs) -- parity tests, bench.py's roofline table and tools/; the product path never asks for it.  Default: the
        product library, unless WATSOR_HIP_DEV=1 is set (how tools/ switch every engine they create).
        schedule: "latency" | "throughput" -- the PROCESS's launch shapes (`set_schedule`), asked for before the engine exists; None:
        whatever is in force (WZ_SCHEDULE, else throughput)."""
        if dev is None:
            dev = os.environ.get("WATSOR_HIP_DEV", "0") not in ("", "0")
        self.dev = bool(dev)
        self._lib = _lib.load(dev=self.dev)
        if schedule is not None:
            set_schedule(schedule, dev=self.dev)
        self._h = C.c_void_p()
        self.max_batch = max_batch
        rc = self._lib.wz_create(os.fsencode(engine_path), device, max_batch, max_width, max_height, C.byref(self._h))
        self._ck(rc, "wz_create")
        self.input_size = self._lib.wz_input_size(self._h)
        self.precision = self._lib.wz_precision(self._h)
        self.num_anchors = self._lib.wz_num_anchors(self._h)
        self.num_classes = self._lib.wz_num_classes(self._h)
        self.num_slots = self._lib.wz_num_slots(self._h)
        self.hp_blocks = self._lib.wz_hp_blocks(self._h)   # leading blocks with split (hi + lo) matrix operands
        self.nms_iou = float(self._lib.wz_nms_iou(self._h))   # the IoU threshold of the engine's own NMS (engine file)
        self.schedule = get_schedule(dev=self.dev)
        self._dev_allocs: List[int] = []
        self._gate_tiles = {}                              # camera id -> tiles of its layout (set_camera_tiles)
        self._gate_last = {}                               # lane -> the camera ids of the last gated call accepted on it
        self._motion_whole = {}                            # camera id -> whole_frame of its motion settings (set_camera_motion)
        self._motion_last = {}                             # lane -> the camera ids of the last motion call accepted on it
        self._motion_grid = {}                             # camera id -> (cell rows, cell columns) of its motion settings
        self._bound_arrays = {}                            # (submit_bound before any bind_frames: the engine's EINVAL, not an AttributeError)
        self._bound_last = {}                              # lane -> frames of the last bound batch accepted on it (bound_source)
        self._bound_cams = []                              # camera id of every table entry (bind_frames) ...
        self._bound_tiled = {}                             # ... and entry -> its camera id where bind_tiles(gated=True) described it, -1 where rects did
        self._bound_motion = {}                            # ... and entry -> its camera id where bind_motion described it

    def _ck(self, rc: int, what: str = "") -> None:
        if rc:
            _lib.check(rc, what, self._lib)

    def _dev_only(self, what: str) -> None:
        if not self.dev:
            raise AttributeError("%s needs the development library: HipEngine(..., dev=True) (libwatsor_hip_dev.so, `make dev`)" % what)

    # -- lifecycle ------------------------------------------------------------------------------
    def close(self) -> None:
        if self._h:
            for p in self._dev_allocs:
                self._lib.wz_dev_free(self._h, C.c_void_p(p))
            self._dev_allocs = []
            self._lib.wz_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_name(self) -> str:
        return self._lib.wz_device_name(self._h).decode()

    # -- hot call -------------------------------------------------------------------------------
    @staticmethod
    def _addr(obj) -> int:
        if isinstance(obj, np.ndarray):
            return obj.ctypes.data
        if isinstance(obj, int):
            return obj
        return C.addressof(obj)

    @staticmethod
    def frame_geometry(f: np.ndarray, fmt: int = FMT_RGB24):
        """(width, height) of a frame array.  `fmt` is a format word: a base format, for the YUV ones or'ed with CSP_BT709 / RANGE_FULL.
        RGB24 / BGR24: (H,W,3) uint8.  NV12 / I420: the usual planar view (H*3/2, W) [or (H*3/2, W, 1)] uint8 -- H rows of luma, then
        H/2 rows holding the subsampled chroma (the bytes a decoder writes with `-pix_fmt nv12` / `yuv420p`).  YUYV422 / UYVY422:
        (H, W, 2) or (H, 2W), W even.  GRAY8: (H, W) or (H, W, 1).  P010 / YUV420P10 (10-bit, a 16-bit word per sample): the planar view
        as uint16 (H*3/2, W) [or (H*3/2, W, 1)], or its bytes as uint8 (H*3/2, W, 2), (H*3/2, 2W) [or (H*3/2, 2W, 1): a uint8 frame buffer
        of the reference]; uint16 arrays are these two formats' only.  Raises ValueError for anything else, and for a format word the
        library refuses (unknown bits, a colour flag on a format that is not YUV)."""
        fmt = int(fmt)
        flags, fmt = fmt & ~FMT_BASE_MASK, fmt & FMT_BASE_MASK
        if f.dtype != np.uint8 and not (f.dtype == np.uint16 and fmt in TEN_BIT_FORMATS):
            raise ValueError("frames are uint8 arrays (P010 / YUV420P10 frames: uint8 or uint16)")
        if flags & ~(CSP_BT709 | RANGE_FULL) or fmt < 0:
            raise ValueError("unknown flag bits in pixel format word 0x%x" % (flags | fmt,))
        if flags and fmt not in YUV_FORMATS:
            raise ValueError("colour flags (BT.709 / full range) apply to the YUV pixel formats only")
        if fmt not in _FRAME_SHAPES:
            raise ValueError("unknown pixel format %r" % (fmt,))
        geo = frame_shape(fmt, f.shape[0], f.shape[1], f.shape[2] if f.ndim == 3 else None, f.itemsize) if f.ndim in (2, 3) else None
        if geo is None or (fmt in TEN_BIT_FORMATS and min(geo) < 1):
            raise ValueError(_FRAME_SHAPES[fmt])
        return geo

    def detect_batch(self, frames: Sequence[np.ndarray], out_rows: Sequence, cams: Optional[Sequence[int]] = None,
                     out_pass: Optional[Sequence[np.ndarray]] = None, formats: Optional[Sequence[int]] = None) -> float:
        """frames: (H,W,3) uint8 C-contiguous arrays (host) -- or, with `formats[i]` = FMT_NV12 / FMT_I420, (H*3/2, W) planar
        views, or any other format word `frame_geometry` describes; out_rows[i]: ctypes Detection[100] (or a ROW_DTYPE array of 100) written in place.  Returns the batch wall
        time in ms."""
        n, (ptrs, ws, hs, outs, keep) = len(frames), self._host_frames(frames, formats, out_rows)
        fmtv = _i32(n, formats)
        camv = _i32(n, cams)
        passv = (C.c_void_p * n)(*[p.ctypes.data for p in out_pass]) if out_pass is not None else None
        ms = (C.c_float * n)()
        self._ck(self._lib.wz_detect_batch_fmt(self._h, n, ptrs, ws, hs, fmtv, camv, outs, passv, ms))
        return float(ms[0])

    def _host_frames(self, frames, formats, out_rows):
        """(pointers, widths, heights, addresses of the rows, what keeps the frames alive) of host frames a synchronous call hands over:
        a frame that is not C-contiguous goes as a copy."""
        n = len(frames)
        ptrs, ws, hs, outs, keep = (C.c_void_p * n)(), (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_void_p * n)(), []
        for i, f in enumerate(frames):
            try:
                ws[i], hs[i] = self.frame_geometry(f, formats[i] if formats is not None else FMT_RGB24)
            except ValueError as exc:
                raise ValueError("frame %d: %s" % (i, exc)) from None
            if not f.flags["C_CONTIGUOUS"]:
                f = np.ascontiguousarray(f)
            keep.append(f)
            ptrs[i] = f.ctypes.data
            outs[i] = self._addr(out_rows[i])
        return ptrs, ws, hs, outs, keep

    @staticmethod
    def _tile_array(rects, where=None):
        """[(x0, y0, w, h), ...] as a `wz_tile_t` array (of one element at least).  where: what the ValueError for a rectangle that is not
        four numbers says in front of its number (None: not checked here)."""
        arr = (Tile * max(1, len(rects)))()
        for k, r in enumerate(rects):
            if where is not None and len(r) != 4:
                raise ValueError("%stile %d: expected (x0, y0, w, h)" % (where, k))
            arr[k] = Tile(*[int(v) for v in r])
        return arr

    def _thresholds(self, iou, ios):
        """The merge thresholds of a call: None = the engine's own NMS threshold / 1.0 (off)."""
        return float(self.nms_iou if iou is None else iou), float(1.0 if ios is None else ios)

    # -- tiled detection (include/watsor_hip.h: wz_detect_tiled) ------------------------------------
    def _tile_args(self, tiles, n: int, iou, ios):
        """(n_tiles, pointers to the frames' wz_tile_t arrays, what keeps them alive, iou, ios) of a tiled call."""
        if len(tiles) != n:
            raise ValueError("tiles: one list of rectangles per frame (%d frames, %d lists)" % (n, len(tiles)))
        keep = [self._tile_array(rects, "frame %d, " % i) for i, rects in enumerate(tiles)]
        counts = (C.c_int32 * n)(*[len(rects) for rects in tiles])
        ptrs = (C.c_void_p * n)(*[C.addressof(arr) for arr in keep])
        return (counts, ptrs, keep) + self._thresholds(iou, ios)

    def detect_tiled(self, frames: Sequence[np.ndarray], tiles: Sequence, out_rows: Sequence, cams: Optional[Sequence[int]] = None,
                     passes: Optional[Sequence[np.ndarray]] = None, formats: Optional[Sequence[int]] = None,
                     iou: Optional[float] = None, ios: Optional[float] = None) -> float:
        """`detect_batch` on rectangles of the frames: tiles[i] = [(x0, y0, w, h), ...] of frame i (`tile_grid`), all the tiles of the
        call at most max_batch; out_rows[i] receives ONE merged list of 100 rows in frame coordinates.  iou / ios: a row is dropped when
        a more confident row of the same label overlaps it by more than `iou` (intersection over union; None: the engine's own NMS
        threshold) or by more than `ios` of the smaller box (None: 1.0 = off).  Returns the wall time in ms."""
        n, (ptrs, ws, hs, outs, keep) = len(frames), self._host_frames(frames, formats, out_rows)
        counts, tptrs, tkeep, iou, ios = self._tile_args(tiles, n, iou, ios)
        fmtv = _i32(n, formats)
        camv = _i32(n, cams)
        passv = (C.c_void_p * n)(*[p.ctypes.data for p in passes]) if passes is not None else None
        ms = (C.c_float * n)()
        self._ck(self._lib.wz_detect_tiled(self._h, n, ptrs, ws, hs, fmtv, camv, counts, tptrs, iou, ios, outs, passv, ms))
        return float(ms[0])

    def submit_tiled_device(self, slot: int, d_frames: Sequence[int], widths: Sequence[int], heights: Sequence[int], tiles: Sequence,
                            cams: Optional[Sequence[int]] = None, formats: Optional[Sequence[int]] = None,
                            iou: Optional[float] = None, ios: Optional[float] = None) -> None:
        """Asynchronous `detect_tiled` of frames resident in HBM on lane `slot`; `collect()` / `wait()` + `slot_rows()` hand over one
        merged list of rows per FRAME."""
        n = len(d_frames)
        counts, tptrs, tkeep, iou, ios = self._tile_args(tiles, n, iou, ios)
        camv = _i32(n, cams)
        fmtv = _i32(n, formats)
        self._ck(self._lib.wz_submit_tiled_device(self._h, slot, n, (C.c_void_p * n)(*d_frames), (C.c_int32 * n)(*widths),
                                                  (C.c_int32 * n)(*heights), fmtv, camv, counts, tptrs, iou, ios))

    # -- what the gated and the motion calls share: one frame per camera, the tiles come from the cameras' settings --------
    def _detect_per_camera(self, fn, last, frames, cams, out_rows, passes, formats, iou, ios) -> float:
        """The synchronous call `fn` (wz_detect_gated | wz_detect_motion) of host frames; `last` remembers lane 0's cameras for the stats."""
        n, (ptrs, ws, hs, outs, keep) = len(frames), self._host_frames(frames, formats, out_rows)
        passv = (C.c_void_p * n)(*[p.ctypes.data for p in passes]) if passes is not None else None
        ms = (C.c_float * n)()
        self._ck(fn(self._h, n, ptrs, ws, hs, _i32(n, formats), _i32(n, cams), *self._thresholds(iou, ios), outs, passv, ms))
        last[0] = [int(c) for c in cams]
        return float(ms[0])

    def _submit_per_camera(self, fn, last, slot, d_frames, widths, heights, cams, formats, iou, ios) -> None:
        """... and its twin `fn` (wz_submit_gated_device | wz_submit_motion_device) of frames resident in HBM on lane `slot`."""
        n = len(d_frames)
        self._ck(fn(self._h, slot, n, (C.c_void_p * n)(*d_frames), (C.c_int32 * n)(*widths), (C.c_int32 * n)(*heights), _i32(n, formats),
                    _i32(n, cams), *self._thresholds(iou, ios)))
        last[slot] = [int(c) for c in cams]

    # -- gated tiled detection (include/watsor_hip.h: wz_set_camera_tiles / wz_detect_gated) ----------------
    def set_camera_tiles(self, cam: int, width: int, height: int, tiles, threshold: int, min_cells: int = 1, max_age: int = 0,
                         fmt: int = FMT_RGB24) -> None:
        """The tile layout of camera `cam` for width x height frames of format `fmt`, and its gate: a cell of 16 x 16 pixels has
        changed when its luma sum moved by more than `threshold` (0 .. 255) per pixel, a tile runs when at least `min_cells` cells
        changed, when it has no reference yet, or -- max_age > 0 -- after `max_age` gated calls in a row that skipped it.  Waits for
        every lane; the camera starts without references (its next gated call runs every tile)."""
        gate = (C.c_int32 * 4)(int(threshold), int(min_cells), int(max_age), 0)
        self._ck(self._lib.wz_set_camera_tiles(self._h, int(cam), int(width), int(height), int(fmt), len(tiles), C.byref(self._tile_array(tiles)),
                                               C.byref(gate)))
        self._gate_tiles[int(cam)] = len(tiles)

    def reset_camera_tiles(self, cam: int) -> None:
        """Forget the references and cached rows of camera `cam` (its next gated call runs every tile); the layout stays."""
        self._ck(self._lib.wz_reset_camera_tiles(self._h, int(cam)))

    def clear_camera_tiles(self, cam: int) -> None:
        self._ck(self._lib.wz_clear_camera_tiles(self._h, int(cam)))
        self._gate_tiles.pop(int(cam), None)

    def detect_gated(self, frames: Sequence[np.ndarray], cams: Sequence[int], out_rows: Sequence,
                     passes: Optional[Sequence[np.ndarray]] = None, formats: Optional[Sequence[int]] = None,
                     iou: Optional[float] = None, ios: Optional[float] = None) -> float:
        """`detect_tiled` with the tiles `set_camera_tiles` gave the frames' cameras, run only where the picture changed: a tile that
        did not drift from the picture it last ran on contributes the rows it produced then.  One frame per camera and call; the
        cameras' configured tiles together at most max_batch.  Returns the wall time in ms; `gate_stats()` tells which tiles ran."""
        return self._detect_per_camera(self._lib.wz_detect_gated, self._gate_last, frames, cams, out_rows, passes, formats, iou, ios)

    def submit_gated_device(self, slot: int, d_frames: Sequence[int], widths: Sequence[int], heights: Sequence[int], cams: Sequence[int],
                            formats: Optional[Sequence[int]] = None, iou: Optional[float] = None, ios: Optional[float] = None) -> None:
        """`detect_gated` of frames resident in HBM on lane `slot`.  Returns once the engine has decided which tiles run (it waits for
        the activity launch); the batch behind is asynchronous and collected like a tiled slot's."""
        self._submit_per_camera(self._lib.wz_submit_gated_device, self._gate_last, slot, d_frames, widths, heights, cams, formats, iou, ios)

    def gate_stats(self, slot: int = 0):
        """What the last gated call accepted on lane `slot` decided: ([per frame: bit t set = tile t ran], [per frame: the tiles'
        activity = changed cells, 0 for a tile that had no reference])."""
        cams = self._gate_last.get(slot)
        if not cams:
            raise ValueError("no gated call was made on lane %d" % slot)
        n = len(cams)
        counts = [self._gate_tiles[c] for c in cams]
        ran = (C.c_uint64 * n)()
        act = (C.c_int32 * max(1, sum(counts)))()
        self._ck(self._lib.wz_gate_stats(self._h, slot, n, C.byref(ran), C.byref(act)))
        flat = np.array(act[:sum(counts)], np.int32)
        return [int(m) for m in ran], [a.copy() for a in np.split(flat, np.cumsum(counts)[:-1])]

    # -- motion regions (include/watsor_hip.h: wz_set_camera_motion / wz_detect_motion) -------------------------
    @staticmethod
    def _motion_words(threshold, min_cells, dilate, max_regions, min_side, pad, whole_frame):
        return (C.c_int32 * 8)(int(threshold), int(min_cells), int(dilate), int(max_regions), int(min_side), int(pad), int(bool(whole_frame)), 0)

    def set_camera_motion(self, cam: int, width: int, height: int, threshold: int, min_cells: int = 1, dilate: int = 1, max_regions: int = 3,
                          min_side: int = 300, pad: int = 8, whole_frame: bool = True, fmt: int = FMT_RGB24) -> None:
        """Camera `cam` detects in the parts of its width x height frames of format `fmt` that moved since its previous motion call: a cell
        of 16 x 16 pixels has changed when its luma sum moved by more than `threshold` (0 .. 255) per pixel; changed cells are dilated by
        `dilate` (0 .. 2) cells and joined into 8-connected components; the heaviest components with at least `min_cells` changed cells
        become at most `max_regions` (1 .. 16) rectangles, `pad` (0 .. 64) pixels around the cells and at least `min_side` (>= 16) pixels
        a side, that run at the camera's own resolution -- beside the whole frame if `whole_frame`.  Waits for every lane; the camera
        starts without a reference (its next motion call sees no motion)."""
        words = self._motion_words(threshold, min_cells, dilate, max_regions, min_side, pad, whole_frame)
        self._ck(self._lib.wz_set_camera_motion(self._h, int(cam), int(width), int(height), int(fmt), C.byref(words)))
        self._motion_whole[int(cam)] = 1 if whole_frame else 0
        self._motion_grid[int(cam)] = (-(-int(height) // _lib.WZ_GATE_CELL), -(-int(width) // _lib.WZ_GATE_CELL))

    def set_camera_motion_hold(self, cam: int, hold: int = 0, object_hold: int = 0) -> None:
        """Camera `cam`, which has motion settings, keeps a cell active -- part of its regions -- for `hold` (0 .. 255) further motion calls
        after it changed, and for `object_hold` (0 .. 255) further calls after a detection that passed the camera's filter covered it
        (include/watsor_hip.h: wz_set_camera_motion_hold).  Both 0: the camera has no hold any more.  Waits for every lane; the ages start
        at zero.  `set_camera_motion` drops the hold: set it after the motion settings."""
        words = (C.c_int32 * 4)(int(hold), int(object_hold), 0, 0)
        self._ck(self._lib.wz_set_camera_motion_hold(self._h, int(cam), C.byref(words)))

    def reset_camera_motion(self, cam: int) -> None:
        """Forget the reference (and the ages of a hold) of camera `cam`: its next motion call sees no motion; the settings stay."""
        self._ck(self._lib.wz_reset_camera_motion(self._h, int(cam)))

    def clear_camera_motion(self, cam: int) -> None:
        self._ck(self._lib.wz_clear_camera_motion(self._h, int(cam)))
        self._motion_whole.pop(int(cam), None)
        self._motion_grid.pop(int(cam), None)

    def detect_motion(self, frames: Sequence[np.ndarray], cams: Sequence[int], out_rows: Sequence,
                      passes: Optional[Sequence[np.ndarray]] = None, formats: Optional[Sequence[int]] = None,
                      iou: Optional[float] = None, ios: Optional[float] = None) -> float:
        """`detect_tiled` on the rectangles the engine finds itself: per frame the whole frame (if its camera's settings say so) and the
        regions that changed since the camera's previous motion call.  One frame per camera and call; the cameras' configured whole_frame +
        max_regions together at most max_batch.  A frame without any tile gets padding rows and pass bytes 0.  Returns the wall time in
        ms; `motion_stats()` tells which rectangles ran."""
        return self._detect_per_camera(self._lib.wz_detect_motion, self._motion_last, frames, cams, out_rows, passes, formats, iou, ios)

    def submit_motion_device(self, slot: int, d_frames: Sequence[int], widths: Sequence[int], heights: Sequence[int], cams: Sequence[int],
                             formats: Optional[Sequence[int]] = None, iou: Optional[float] = None, ios: Optional[float] = None) -> None:
        """`detect_motion` of frames resident in HBM on lane `slot`.  Returns once the engine has read the rectangles (it waits for the
        activity and the region launch); the batch behind is asynchronous and collected like a tiled slot's."""
        self._submit_per_camera(self._lib.wz_submit_motion_device, self._motion_last, slot, d_frames, widths, heights, cams, formats, iou, ios)

    def motion_stats(self, slot: int = 0):
        """What the last motion call accepted on lane `slot` found: ([per frame: its tile list [(x0, y0, w, h), ...] -- the whole frame first
        if configured, then the regions in rank order], [per frame: the changed cells of every region], [per frame: the components with
        at least min_cells changed cells])."""
        cams = self._motion_last.get(slot)
        if not cams:
            raise ValueError("no motion call was made on lane %d" % slot)
        n, per, most = len(cams), 1 + _lib.WZ_MOTION_MAX_REGIONS, _lib.WZ_MOTION_MAX_REGIONS
        counts, tiles, cells, comps = (C.c_int32 * n)(), (Tile * (n * per))(), (C.c_int32 * (n * most))(), (C.c_int32 * n)()
        self._ck(self._lib.wz_motion_stats(self._h, slot, n, C.byref(counts), C.byref(tiles), C.byref(cells), C.byref(comps)))
        lists = [[(t.x0, t.y0, t.w, t.h) for t in tiles[i * per:i * per + counts[i]]] for i in range(n)]
        regions = [counts[i] - self._motion_whole[c] for i, c in enumerate(cams)]
        return lists, [[int(v) for v in cells[i * most:i * most + regions[i]]] for i in range(n)], [int(v) for v in comps]

    def motion_hold_stats(self, slot: int = 0):
        """Per frame of the last motion call accepted on lane `slot`: ([its active cells: changed, or held by an age], [those of them that
        did not change]); 0 and 0 for a frame whose camera has no hold."""
        cams = self._motion_last.get(slot)
        if not cams:
            raise ValueError("no motion call was made on lane %d" % slot)
        n = len(cams)
        active, held = (C.c_int32 * n)(), (C.c_int32 * n)()
        self._ck(self._lib.wz_motion_hold_stats(self._h, slot, n, C.byref(active), C.byref(held)))
        return [int(v) for v in active], [int(v) for v in held]

    # -- ignore masks (include/watsor_hip.h: wz_set_camera_ignore) ------------------------------------------------
    def set_camera_ignore(self, cam: int, mask: Optional[np.ndarray]) -> None:
        """Camera `cam`, which has motion settings, a gate layout or both, ignores change where `mask` -- (height, width) uint8, the size
        its settings were made for -- is nonzero: a 16 x 16-pixel cell with at least one ignored pixel never counts as changed, neither
        for its motion regions nor for its tiles' activity (`ignore_cells` is the rule).  None removes the mask.  Waits for every lane.
        `set_camera_motion` drops the motion part and `set_camera_tiles` the gate part: set the mask after them."""
        if mask is None:
            self._ck(self._lib.wz_set_camera_ignore(self._h, int(cam), 0, 0, None))
            return
        m = _ignore_plane(mask)
        self._ck(self._lib.wz_set_camera_ignore(self._h, int(cam), m.shape[1], m.shape[0], C.c_void_p(m.ctypes.data)))

    def motion_ignore_stats(self, slot: int = 0):
        """Per frame of the last motion call accepted on lane `slot`: the changed cells that its camera's ignore mask removed (0 for a
        camera without one)."""
        cams = self._motion_last.get(slot)
        if not cams:
            raise ValueError("no motion call was made on lane %d" % slot)
        n = len(cams)
        ignored = (C.c_int32 * n)()
        self._ck(self._lib.wz_motion_ignore_stats(self._h, slot, n, C.byref(ignored)))
        return [int(v) for v in ignored]

    def submit_device(self, slot: int, d_frames: Sequence[int], widths: Sequence[int], heights: Sequence[int],
                      cams: Optional[Sequence[int]] = None, formats: Optional[Sequence[int]] = None) -> None:
        n = len(d_frames)
        ptrs = (C.c_void_p * n)(*d_frames)
        ws = (C.c_int32 * n)(*widths)
        hs = (C.c_int32 * n)(*heights)
        camv = _i32(n, cams)
        fmtv = _i32(n, formats)
        self._ck(self._lib.wz_submit_device_fmt(self._h, slot, n, ptrs, ws, hs, fmtv, camv))

    def submit_host(self, slot: int, frames: Sequence[np.ndarray], cams: Optional[Sequence[int]] = None,
                    formats: Optional[Sequence[int]] = None) -> None:
        """Asynchronous detect of host frames ((H,W,3) uint8, C-contiguous; other pixel formats: see `frame_geometry`) on lane
        `slot`; collect with `collect()` / `slot_rows()`.  The arrays must stay alive and unchanged until the slot is collected."""
        n = len(frames)
        ws = (C.c_int32 * n)()
        hs = (C.c_int32 * n)()
        for i, f in enumerate(frames):
            try:
                ws[i], hs[i] = self.frame_geometry(f, formats[i] if formats is not None else FMT_RGB24)
            except ValueError as exc:
                raise ValueError("frame %d: %s" % (i, exc)) from None
            if not f.flags["C_CONTIGUOUS"]:
                raise ValueError("frame %d must be C-contiguous (it is read in place, asynchronously)" % i)
        ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        camv = _i32(n, cams)
        fmtv = _i32(n, formats)
        self._ck(self._lib.wz_submit_host_fmt(self._h, slot, n, ptrs, ws, hs, fmtv, camv))

    def host_register(self, arr: np.ndarray) -> None:
        """Page-lock the memory behind `arr` (frames handed over from it then travel by DMA)."""
        self._ck(self._lib.wz_host_register(self._h, C.c_void_p(arr.ctypes.data), arr.nbytes))

    def host_unregister(self, arr: np.ndarray) -> None:
        self._ck(self._lib.wz_host_unregister(self._h, C.c_void_p(arr.ctypes.data)))

    def host_register_address(self, address: int, nbytes: int) -> None:
        """The same for raw memory, e.g. a `multiprocessing.sharedctypes` array shared with other processes."""
        self._ck(self._lib.wz_host_register(self._h, C.c_void_p(address), nbytes))

    def host_unregister_address(self, address: int) -> None:
        self._ck(self._lib.wz_host_unregister(self._h, C.c_void_p(address)))

    # -- the worker's frame table (include/watsor_hip.h: wz_bind_frames) ----------------------------
    def bind_frames(self, pixel_addresses: Sequence[int], widths: Sequence[int], heights: Sequence[int],
                    formats: Sequence[int], cams: Sequence[int], row_addresses: Sequence[int]) -> None:
        """Describe every frame of every frame buffer once: entry i = (address of its pixels, width, height, WZ_FMT_*, camera id
        or -1, address of its `Detection[100]` rows).  Replaces the previous table."""
        n = len(pixel_addresses)
        self._ck(self._lib.wz_bind_frames(
            self._h, n, (C.c_void_p * n)(*pixel_addresses), (C.c_int32 * n)(*widths), (C.c_int32 * n)(*heights),
            (C.c_int32 * n)(*[int(f) for f in formats]), (C.c_int32 * n)(*[int(c) for c in cams]),
            (C.c_void_p * n)(*row_addresses)))
        self._bound_arrays = {}
        self._bound_cams = [int(c) for c in cams]
        self._bound_tiled = {}
        self._bound_motion = {}

    def bind_tiles(self, first: int, count: int, rects=None, iou: Optional[float] = None, ios: Optional[float] = 1.0, gated: bool = False) -> None:
        """Table entries first .. first + count - 1 (normally one camera's frames) are detected TILED from now on (include/watsor_hip.h:
        wz_bind_tiles): `rects` = [(x0, y0, w, h), ...] as `detect_tiled` takes them, or gated=True (and no rects): the tiles and the gate
        `set_camera_tiles` gave the entries' camera, looked up at every submit.  rects=None without `gated`: untiled again.  iou / ios as in
        `detect_tiled` (None: the engine's own NMS threshold / 1.0).  Waits for every lane."""
        n = 0 if rects is None else len(rects)
        arr = C.byref(self._tile_array(rects, "")) if rects is not None else None
        self._ck(self._lib.wz_bind_tiles(self._h, int(first), int(count), n, arr, *self._thresholds(iou, ios), 1 if gated else 0))
        for i in range(int(first), int(first) + int(count)):
            self._bound_motion.pop(i, None)
            if gated:
                self._bound_tiled[i] = self._bound_cams[i]
            elif rects is not None:
                self._bound_tiled[i] = -1
            else:
                self._bound_tiled.pop(i, None)

    def bind_motion(self, first: int, count: int, iou: Optional[float] = None, ios: Optional[float] = 1.0) -> None:
        """Table entries first .. first + count - 1 -- the frames of one camera, which carry its id -- are detected in their MOTION REGIONS
        from now on (include/watsor_hip.h: wz_bind_motion): settings, hold and ignore mask are the ones `set_camera_motion`,
        `set_camera_motion_hold` and `set_camera_ignore` gave the camera, looked up at every submit.  iou / ios as in `detect_motion` (None:
        the engine's own NMS threshold / 1.0).  `bind_tiles(first, count, None)` makes them untiled again.  Waits for every lane."""
        self._ck(self._lib.wz_bind_motion(self._h, int(first), int(count), *self._thresholds(iou, ios)))
        for i in range(int(first), int(first) + int(count)):
            self._bound_tiled.pop(i, None)
            self._bound_motion[i] = self._bound_cams[i]

    def bound_source(self, slot: int) -> List[int]:
        """Development library: per frame of the last tiled, gated or motion bound batch on lane `slot`, 1 = read in place from page-locked
        memory, 0 = staged by DMA (a motion batch: always 0)."""
        self._dev_only("bound_source")
        n = self._bound_last.get(slot, 0)
        out = (C.c_int32 * max(1, n))()
        self._ck(self._lib.wz_debug_bound_source(self._h, slot, C.byref(out)))
        return [int(v) for v in out[:n]]

    def submit_bound(self, slot: int, entries: Sequence[int]) -> None:
        """Asynchronous detect of the frames with these table indices on lane `slot` (one C call, no per-frame work here).  Entries with a
        tiled description (`bind_tiles`) run tiled / gated, entries with a motion description (`bind_motion`) in their motion regions; a
        batch holds one kind."""
        n = len(entries)
        arr_t = self._bound_arrays.get(n)
        if arr_t is None:
            arr_t = self._bound_arrays[n] = C.c_int32 * n
        rc = self._lib.wz_submit_bound(self._h, slot, n, arr_t(*entries))
        if rc:
            self._ck(rc)
        if self._bound_tiled:                                          # (what bound_source / gate_stats need to know about the lane)
            cam = self._bound_tiled.get(entries[0])
            if cam is not None:
                self._bound_last[slot] = n
                if cam >= 0:
                    self._gate_last[slot] = [self._bound_tiled[i] for i in entries]
        if self._bound_motion and entries[0] in self._bound_motion:    # (... and motion_stats / motion_hold_stats / motion_ignore_stats)
            self._bound_last[slot] = n
            self._motion_last[slot] = [self._bound_motion[i] for i in entries]

    def collect_bound(self, slot: int) -> None:
        """Waits for lane `slot`; its rows are written into the bound frames' own `Detection[100]` arrays."""
        rc = self._lib.wz_collect_bound(self._h, slot)
        if rc:
            self._ck(rc)

    def collect(self, slot: int, out_rows: Sequence, out_pass: Optional[Sequence[np.ndarray]] = None) -> None:
        n = len(out_rows)
        outs = (C.c_void_p * n)(*[self._addr(r) for r in out_rows])
        passv = (C.c_void_p * n)(*[p.ctypes.data for p in out_pass]) if out_pass is not None else None
        self._ck(self._lib.wz_collect(self._h, slot, outs, passv))

    def wait(self, slot: int) -> None:
        self._ck(self._lib.wz_wait(self._h, slot))

    def slot_rows(self, slot: int, n: int) -> np.ndarray:
        """View (no copy) of the pinned result rows of `slot`: ROW_DTYPE [n,100]."""
        p = self._lib.wz_slot_rows(self._h, slot)
        buf = (C.c_uint8 * (72 * MAX_DETECTIONS * n)).from_address(p)
        return np.frombuffer(buf, dtype=ROW_DTYPE).reshape(n, MAX_DETECTIONS)

    def graph_nodes(self, slot: int = 0) -> int:
        """Nodes of the hipGraph last replayed on lane `slot` (kernel launches + the descriptor copy); 0 when graphs are off."""
        return int(self._lib.wz_graph_nodes(self._h, slot))

    def sync(self) -> None:
        self._ck(self._lib.wz_sync(self._h))

    # -- device memory --------------------------------------------------------------------------
    def upload(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        self._ck(self._lib.wz_dev_alloc(self._h, arr.nbytes, C.byref(p)))
        self._dev_allocs.append(p.value)
        self._ck(self._lib.wz_dev_upload(self._h, p, C.c_void_p(arr.ctypes.data), arr.nbytes))
        return p.value

    def download(self, d_ptr: int, nbytes: int) -> np.ndarray:
        """`nbytes` of device memory at `d_ptr` as a uint8 array (wz_dev_download: waits for lane 0, like `upload`)."""
        out = np.empty(int(nbytes), np.uint8)
        self._ck(self._lib.wz_dev_download(self._h, C.c_void_p(out.ctypes.data), C.c_void_p(d_ptr), out.nbytes))
        return out

    def free(self, d_ptr: int) -> None:
        self._dev_allocs.remove(d_ptr)
        self._ck(self._lib.wz_dev_free(self._h, C.c_void_p(d_ptr)))

    # -- filters --------------------------------------------------------------------------------
    def set_camera_filter(self, cam: int, width: int, height: int, conf_thr: np.ndarray, area_thr: np.ndarray,
                          zone_fill: Optional[np.ndarray] = None, zone_allow: Optional[np.ndarray] = None) -> None:
        conf = np.ascontiguousarray(conf_thr, np.float64)
        area = np.ascontiguousarray(area_thr, np.float64)
        assert conf.shape == (_lib.WZ_NUM_LABELS,) and area.shape == (_lib.WZ_NUM_LABELS,)
        nz = 0 if zone_fill is None else int(zone_fill.shape[0])
        fill_p = allow_p = None
        if zone_fill is not None and nz == 0:      # a mask without zones: nothing can hit it (mask.py:44-59)
            self._no_zones = np.zeros(1, np.uint8)
            fill_p = C.c_void_p(self._no_zones.ctypes.data)
        if nz:
            zone_fill = np.ascontiguousarray(zone_fill, np.uint8)
            assert zone_fill.shape == (nz, height, width)
            fill_p = C.c_void_p(zone_fill.ctypes.data)
            if zone_allow is not None:
                zone_allow = np.ascontiguousarray(zone_allow, np.uint8)
                assert zone_allow.shape == (_lib.WZ_NUM_LABELS, nz)
                allow_p = C.c_void_p(zone_allow.ctypes.data)
        self._ck(self._lib.wz_set_camera_filter(
            self._h, cam, width, height, conf.ctypes.data_as(_lib.c_f64p), area.ctypes.data_as(_lib.c_f64p),
            nz, allow_p, fill_p))

    def set_camera_drop(self, cam: int, drop: bool) -> None:
        """Rows of camera `cam` that fail its filters are written as all-zero rows (include/watsor_hip.h)."""
        self._ck(self._lib.wz_set_camera_drop(self._h, cam, 1 if drop else 0))

    def clear_camera_filter(self, cam: int) -> None:
        self._ck(self._lib.wz_clear_camera_filter(self._h, cam))

    def filter_rows(self, cam: int, rows) -> np.ndarray:
        """Runs Confidence/Area/Mask of camera `cam` on 100 rows in place; returns pass[100] (uint8)."""
        out = np.zeros(MAX_DETECTIONS, np.uint8)
        self._ck(self._lib.wz_filter_rows(self._h, cam, C.c_void_p(self._addr(rows)), C.c_void_p(out.ctypes.data)))
        return out

    # -- introspection / profiling ---------------------------------------------------------------
    def tensors(self):
        self._dev_only("tensors()")
        out = []
        name = C.create_string_buffer(64)
        h, w, c = C.c_int32(), C.c_int32(), C.c_int32()
        for i in range(self._lib.wz_num_tensors(self._h)):
            self._ck(self._lib.wz_tensor_info(self._h, i, name, 64, C.byref(h), C.byref(w), C.byref(c)))
            out.append((name.value.decode(), h.value, w.value, c.value))
        return out

    def ops(self):
        self._dev_only("ops()")
        out = []
        name = C.create_string_buffer(80)
        dims = (C.c_int32 * 12)()
        keys = ("kind", "cin", "cout", "ksize", "stride", "hin", "win", "hout", "wout", "n_pad", "kc", "cmid")
        for i in range(self._lib.wz_num_ops(self._h)):
            self._ck(self._lib.wz_op_info(self._h, i, name, 80, dims))
            d = dict(zip(keys, list(dims)))
            d["name"] = name.value.decode()
            out.append(d)
        return out

    def stage_names(self) -> List[str]:
        self._dev_only("stage_names()")
        name = C.create_string_buffer(96)
        out = []
        for i in range(self._lib.wz_num_stages(self._h)):
            self._ck(self._lib.wz_stage_name(self._h, i, name, 96))
            out.append(name.value.decode())
        return out

    def profile_device(self, d_frames: Sequence[int], widths: Sequence[int], heights: Sequence[int], reps: int = 10,
                       inner: int = 1):
        """[(stage name, ms of its event bracket)]; inner > 1: every network kernel `inner` times back to back in its bracket."""
        self._dev_only("profile_device()")
        n = len(d_frames)
        ns = self._lib.wz_num_stages(self._h)
        ms = (C.c_float * ns)()
        self._ck(self._lib.wz_profile_stages(self._h, n, (C.c_void_p * n)(*d_frames), (C.c_int32 * n)(*widths),
                                               (C.c_int32 * n)(*heights), reps, inner, ms))
        return list(zip(self.stage_names(), [float(x) for x in ms]))

    # -- stage-level entry points (parity tests) --------------------------------------------------
    def tensor_is_pair(self, idx: int) -> bool:
        self._dev_only("tensor_is_pair()")
        return bool(self._lib.wz_tensor_flags(self._h, idx) & 1)

    def stage_preprocess(self, frame: np.ndarray, fmt: int = FMT_RGB24) -> np.ndarray:
        """(S,S,4) float16; for a pair input tensor (S,S,8): hi (r,g,b,0) then lo (r,g,b,0)."""
        self._dev_only("stage_preprocess()")
        frame = np.ascontiguousarray(frame) if frame.dtype == np.uint16 else np.ascontiguousarray(frame, np.uint8)
        w, h = self.frame_geometry(frame, fmt)
        S = self.input_size
        out = np.empty((S, S, 8 if self.tensor_is_pair(0) else 4), np.float16)
        self._ck(self._lib.wz_stage_preprocess_fmt(self._h, C.c_void_p(frame.ctypes.data), w, h, int(fmt),
                                                     C.c_void_p(out.ctypes.data)))
        return out

    def stage_forward(self, x_half: np.ndarray):
        """x_half float16 [n,S,S,4] -> (box_enc float32 [n,A,4], logits float32 [n,A,C])."""
        self._dev_only("stage_forward()")
        x = np.ascontiguousarray(x_half, np.float16)
        n = x.shape[0]
        be = np.empty((n, self.num_anchors, 4), np.float32)
        lg = np.empty((n, self.num_anchors, self.num_classes), np.float32)
        self._ck(self._lib.wz_stage_forward(self._h, n, C.c_void_p(x.ctypes.data), C.c_void_p(be.ctypes.data),
                                              C.c_void_p(lg.ctypes.data)))
        return be, lg

    def stage_read_tensor(self, idx: int, frame: int = 0, halves: bool = False):
        """(h,w,c) array as stored; a pair tensor comes back as float32 hi + lo (not always exact: 1 + 2^-24 needs 25 bits).
        halves=True: (hi, lo), the two float16 planes of a pair tensor exactly as stored; (the tensor, None) for any other."""
        self._dev_only("stage_read_tensor()")
        name, h, w, c = self.tensors()[idx]
        pair = self.tensor_is_pair(idx)
        out = np.empty((h, w, 2 * c if pair else c), np.float16 if (self.precision == 16 or name == "input") else np.float32)
        self._ck(self._lib.wz_stage_read_tensor(self._h, idx, frame, C.c_void_p(out.ctypes.data)))
        if halves:
            return (out[..., :c].copy(), out[..., c:].copy()) if pair else (out, None)
        if pair:
            return out[..., :c].astype(np.float32) + out[..., c:].astype(np.float32)
        return out

    def stage_block_at(self, op: int, n: int, d_in: int, launch_frames: int = 0) -> None:
        """Fused block `op` (index into ops()) of the last forward again for its n frames, its source tensor read at the device
        address `d_in` (`upload`); the outputs land where the network puts them (stage_read_tensor).  launch_frames > 0: a
        split-operand block in launches of at most that many frames."""
        self._dev_only("stage_block_at()")
        self._ck(self._lib.wz_stage_block_at(self._h, int(op), int(n), C.c_void_p(d_in), int(launch_frames)))

    def stage_postprocess(self, box_enc: np.ndarray, logits: np.ndarray):
        self._dev_only("stage_postprocess()")
        be = np.ascontiguousarray(box_enc, np.float32)
        lg = np.ascontiguousarray(logits, np.float32)
        n = be.shape[0]
        boxes = np.empty((n, MAX_DETECTIONS, 4), np.float32)
        scores = np.empty((n, MAX_DETECTIONS), np.float32)
        classes = np.empty((n, MAX_DETECTIONS), np.int32)
        num = np.empty((n,), np.int32)
        self._ck(self._lib.wz_stage_postprocess(
            self._h, n, C.c_void_p(be.ctypes.data), C.c_void_p(lg.ctypes.data), C.c_void_p(boxes.ctypes.data),
            C.c_void_p(scores.ctypes.data), C.c_void_p(classes.ctypes.data), C.c_void_p(num.ctypes.data)))
        return boxes, scores, classes, num

    def stage_post_lane(self, slot: int, n: int) -> dict:
        """What the post-processing of the batch of `n` frames last run -- and collected -- on lane `slot` left in device memory
        (include/watsor_hip.h: wz_debug_post_lane; no kernel is launched): box_enc [n,A,4], logits [n,A,C], boxes [n,100,4],
        scores [n,100], classes [n,100], num [n], dbg uint64 [n,16] and the two flags decode_fused, cands_listed.  The counts among
        the dbg words, unpacked: first_cnt (slot 8), first_kept (9), processed (10), listed (14), first_lo, hint_in and serial -- the
        exact serial walk of a crowded bin ran -- (15).  Engines with max_total other than 100 are refused."""
        self._dev_only("stage_post_lane()")
        A, Cn = self.num_anchors, self.num_classes
        out = dict(box_enc=np.empty((n, A, 4), np.float32), logits=np.empty((n, A, Cn), np.float32),
                   boxes=np.empty((n, MAX_DETECTIONS, 4), np.float32), scores=np.empty((n, MAX_DETECTIONS), np.float32),
                   classes=np.empty((n, MAX_DETECTIONS), np.int32), num=np.empty((n,), np.int32), dbg=np.zeros((n, 16), np.uint64))
        flags = (C.c_int32 * 2)()
        self._ck(self._lib.wz_debug_post_lane(self._h, int(slot), int(n), *[C.c_void_p(out[k].ctypes.data) for k in
                                              ("box_enc", "logits", "boxes", "scores", "classes", "num", "dbg")], C.byref(flags)))
        d = out["dbg"]
        out.update(decode_fused=bool(flags[0]), cands_listed=bool(flags[1]),
                   first_cnt=d[:, 8].astype(np.int64), first_kept=d[:, 9].astype(np.int64), processed=d[:, 10].astype(np.int64),
                   listed=d[:, 14].astype(np.int64), first_lo=(d[:, 15] & np.uint64(0xFFFFFFFF)).astype(np.int64),
                   hint_in=((d[:, 15] >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64),
                   serial=((d[:, 15] >> np.uint64(48)) & np.uint64(1)).astype(bool))
        return out

    def stage_post_production(self, box_enc: np.ndarray, logits: np.ndarray, width: int, height: int) -> np.ndarray:
        """The post-processing of a real batch on caller-provided head outputs [n,A,4], [n,A,C], on lane 0 (include/watsor_hip.h:
        wz_stage_post_production): rows ROW_DTYPE [n,100] of frames width x height; `stage_post_lane(0, n)` reads back the rest."""
        self._dev_only("stage_post_production()")
        be = np.ascontiguousarray(box_enc, np.float32)
        lg = np.ascontiguousarray(logits, np.float32)
        n = be.shape[0]
        assert be.shape == (n, self.num_anchors, 4) and lg.shape == (n, self.num_anchors, self.num_classes)
        rows = np.zeros((n, MAX_DETECTIONS), ROW_DTYPE)
        self._ck(self._lib.wz_stage_post_production(self._h, n, C.c_void_p(be.ctypes.data), C.c_void_p(lg.ctypes.data), int(width),
                                                    int(height), C.c_void_p(rows.ctypes.data)))
        return rows

    def stage_crop_tile(self, frame: np.ndarray, tile, fmt: int = FMT_RGB24) -> np.ndarray:
        """The bytes of rectangle `tile` = (x0, y0, w, h) of `frame` as the crop kernel writes them (a flat uint8 array).  The frame
        is read where it lies: a view at an odd address reaches the kernel at an odd address."""
        self._dev_only("stage_crop_tile()")
        if not frame.flags["C_CONTIGUOUS"]:
            frame = np.ascontiguousarray(frame)
        w, h = self.frame_geometry(frame, fmt)
        t = Tile(*[int(v) for v in tile])
        out = np.empty(max(1, int(self._lib.wz_frame_bytes(max(t.w, 0), max(t.h, 0), int(fmt)))), np.uint8)
        self._ck(self._lib.wz_stage_crop_tile(self._h, C.c_void_p(frame.ctypes.data), w, h, int(fmt), C.byref(t),
                                                C.c_void_p(out.ctypes.data)))
        return out

    def stage_tile_activity(self, frame: np.ndarray, tile, fmt: int = FMT_RGB24, ref: Optional[np.ndarray] = None, pixel_thr: int = 0):
        """The activity kernel on rectangle `tile` = (x0, y0, w, h) of `frame`: (luma sums of its 16 x 16 cells, uint16 [cell rows, cell
        columns]; the number of cells that moved by more than pixel_thr a pixel against the grid `ref`, 0 without one).  The frame is
        read where it lies: a view at an odd address reaches the kernel at an odd address."""
        self._dev_only("stage_tile_activity()")
        if not frame.flags["C_CONTIGUOUS"]:
            frame = np.ascontiguousarray(frame)
        w, h = self.frame_geometry(frame, fmt)
        t = Tile(*[int(v) for v in tile])
        shape = (max(1, -(-t.h // _lib.WZ_GATE_CELL)), max(1, -(-t.w // _lib.WZ_GATE_CELL)))
        sums = np.zeros(shape, np.uint16)
        changed = C.c_int32(-1)
        if ref is not None:
            ref = np.ascontiguousarray(ref, np.uint16)
            if ref.shape != shape:
                raise ValueError("ref: expected a uint16 grid of shape %r, got %r" % (shape, ref.shape))
        self._ck(self._lib.wz_stage_tile_activity(self._h, C.c_void_p(frame.ctypes.data), w, h, int(fmt), C.byref(t),
                                                  C.c_void_p(ref.ctypes.data) if ref is not None else None, int(pixel_thr),
                                                  C.c_void_p(sums.ctypes.data), C.byref(changed)))
        return sums, int(changed.value)

    def stage_tile_activity_ignore(self, frame: np.ndarray, tile, cells_ignored: Optional[np.ndarray], fmt: int = FMT_RGB24,
                                   ref: Optional[np.ndarray] = None, pixel_thr: int = 0):
        """`stage_tile_activity` as a launch with a masked tile runs it: `cells_ignored` is the tile's cell mask (uint8 [cell rows, cell
        columns], nonzero: ignored; None: this tile has none); the count leaves the ignored cells out, the sums are the same."""
        self._dev_only("stage_tile_activity_ignore()")
        if not frame.flags["C_CONTIGUOUS"]:
            frame = np.ascontiguousarray(frame)
        w, h = self.frame_geometry(frame, fmt)
        t = Tile(*[int(v) for v in tile])
        shape = (max(1, -(-t.h // _lib.WZ_GATE_CELL)), max(1, -(-t.w // _lib.WZ_GATE_CELL)))
        ref, = self._motion_grids(shape, ref=(ref, np.uint16))
        cells_ignored, = self._motion_grids(shape, cells_ignored=(cells_ignored, np.uint8))
        sums = np.zeros(shape, np.uint16)
        changed = C.c_int32(-1)
        ptr = lambda g: C.c_void_p(g.ctypes.data) if g is not None else None      # noqa: E731
        self._ck(self._lib.wz_stage_tile_activity_ignore(self._h, C.c_void_p(frame.ctypes.data), w, h, int(fmt), C.byref(t), ptr(ref), int(pixel_thr),
                                                         ptr(cells_ignored), C.c_void_p(sums.ctypes.data), C.byref(changed)))
        return sums, int(changed.value)

    def stage_motion_ignore(self, now: np.ndarray, ref: Optional[np.ndarray], cells_ignored: Optional[np.ndarray], width: int, height: int,
                            threshold: int, hold: Optional[int] = None, age: Optional[np.ndarray] = None, min_cells: int = 1, dilate: int = 1,
                            max_regions: int = 3, min_side: int = 300, pad: int = 8, fmt: int = FMT_RGB24):
        """The region kernel alone as a launch with a masked camera runs it: `cells_ignored` is the grid's cell mask (uint8 [cell rows, cell
        columns], nonzero: ignored; None: this camera has none).  hold None: a camera without a hold -> (rectangles, the changed cells of
        every region, components, the changed cells the mask removed).  hold an int (with the ages `age`, None: all zero): a camera with
        one -> `stage_motion_hold`'s tuple with the removed cells as its last element."""
        self._dev_only("stage_motion_ignore()")
        shape = (-(-int(height) // _lib.WZ_GATE_CELL), -(-int(width) // _lib.WZ_GATE_CELL))
        now, ref, age, cells_ignored = self._motion_grids(shape, now=(now, np.uint16), ref=(ref, np.uint16), age=(age, np.uint8),
                                                          cells_ignored=(cells_ignored, np.uint8))
        if hold is None and age is not None:
            raise ValueError("ages without a hold")
        words = self._motion_words(threshold, min_cells, dilate, max_regions, min_side, pad, False)
        most = _lib.WZ_MOTION_MAX_REGIONS
        n, comps, active, held, ignored = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        tiles, cells = (Tile * most)(), (C.c_int32 * most)()
        out = None if hold is None else np.full(shape, 0xA5, np.uint8)
        ptr = lambda g: C.c_void_p(g.ctypes.data) if g is not None else None      # noqa: E731
        self._ck(self._lib.wz_stage_motion_ignore(self._h, ptr(now), ptr(ref), ptr(age), int(width), int(height), int(fmt), C.byref(words),
                                                  int(hold or 0), ptr(cells_ignored), C.byref(n), C.byref(tiles), C.byref(cells), C.byref(comps),
                                                  C.byref(active), C.byref(held), C.byref(ignored), ptr(out)))
        rects, ns = [(t.x0, t.y0, t.w, t.h) for t in tiles[:n.value]], [int(v) for v in cells[:n.value]]
        if hold is None:
            return rects, ns, int(comps.value), int(ignored.value)
        return rects, ns, int(comps.value), int(active.value), int(held.value), out, int(ignored.value)

    def profile_motion_ignore(self, now: np.ndarray, ref: Optional[np.ndarray], cells_ignored: np.ndarray, width: int, height: int, threshold: int,
                              min_cells: int = 1, dilate: int = 1, max_regions: int = 3, min_side: int = 300, pad: int = 8,
                              fmt: int = FMT_RGB24, reps: int = 100):
        """(ms of the region launch alone on these grids with this cell mask, ms of an empty bracket): HIP-event brackets, the mean of `reps`."""
        self._dev_only("profile_motion_ignore()")
        shape = (-(-int(height) // _lib.WZ_GATE_CELL), -(-int(width) // _lib.WZ_GATE_CELL))
        now, ref, cells_ignored = self._motion_grids(shape, now=(now, np.uint16), ref=(ref, np.uint16), cells_ignored=(cells_ignored, np.uint8))
        words = self._motion_words(threshold, min_cells, dilate, max_regions, min_side, pad, False)
        reg, empty = C.c_float(), C.c_float()
        ptr = lambda g: C.c_void_p(g.ctypes.data) if g is not None else None      # noqa: E731
        self._ck(self._lib.wz_profile_motion_ignore(self._h, ptr(now), ptr(ref), int(width), int(height), int(fmt), C.byref(words), ptr(cells_ignored),
                                                    int(reps), C.byref(reg), C.byref(empty)))
        return float(reg.value), float(empty.value)

    def stage_motion_regions(self, now: np.ndarray, ref: Optional[np.ndarray], width: int, height: int, threshold: int, min_cells: int = 1,
                             dilate: int = 1, max_regions: int = 3, min_side: int = 300, pad: int = 8, fmt: int = FMT_RGB24):
        """The region kernel alone on two grids of luma sums (uint16 [cell rows, cell columns] of a width x height frame of format `fmt`; ref
        None: no reference): ([(x0, y0, w, h), ...] in rank order, the changed cells of every region, the components with at least
        min_cells changed cells)."""
        self._dev_only("stage_motion_regions()")
        shape = (-(-int(height) // _lib.WZ_GATE_CELL), -(-int(width) // _lib.WZ_GATE_CELL))
        now = np.ascontiguousarray(now, np.uint16)
        ref = None if ref is None else np.ascontiguousarray(ref, np.uint16)
        for name, g in (("now", now), ("ref", ref)):
            if g is not None and g.shape != shape:
                raise ValueError("%s: expected a uint16 grid of shape %r, got %r" % (name, shape, g.shape))
        words = self._motion_words(threshold, min_cells, dilate, max_regions, min_side, pad, False)
        most = _lib.WZ_MOTION_MAX_REGIONS
        n, comps, tiles, cells = C.c_int32(-1), C.c_int32(-1), (Tile * most)(), (C.c_int32 * most)()
        self._ck(self._lib.wz_stage_motion_regions(self._h, C.c_void_p(now.ctypes.data), C.c_void_p(ref.ctypes.data) if ref is not None else None,
                                                   int(width), int(height), int(fmt), C.byref(words), C.byref(n), C.byref(tiles), C.byref(cells),
                                                   C.byref(comps)))
        return [(t.x0, t.y0, t.w, t.h) for t in tiles[:n.value]], [int(v) for v in cells[:n.value]], int(comps.value)

    def profile_motion(self, now: np.ndarray, ref: Optional[np.ndarray], width: int, height: int, threshold: int, min_cells: int = 1,
                       dilate: int = 1, max_regions: int = 3, min_side: int = 300, pad: int = 8, fmt: int = FMT_RGB24, reps: int = 100):
        """(ms of the region launch alone on these grids, ms of the whole-frame activity launch of such a frame alone, ms of an empty
        bracket, rounds the labelling took): HIP-event brackets, the mean of `reps` each."""
        self._dev_only("profile_motion()")
        now = np.ascontiguousarray(now, np.uint16)
        ref = None if ref is None else np.ascontiguousarray(ref, np.uint16)
        words = self._motion_words(threshold, min_cells, dilate, max_regions, min_side, pad, False)
        reg, act, empty, rounds = C.c_float(), C.c_float(), C.c_float(), C.c_int32()
        self._ck(self._lib.wz_profile_motion(self._h, C.c_void_p(now.ctypes.data), C.c_void_p(ref.ctypes.data) if ref is not None else None,
                                             int(width), int(height), int(fmt), C.byref(words), int(reps), C.byref(reg), C.byref(act), C.byref(empty),
                                             C.byref(rounds)))
        return float(reg.value), float(act.value), float(empty.value), int(rounds.value)

    @staticmethod
    def _motion_grids(shape, **grids):
        """the named grids (None stays None) as contiguous arrays of their dtype, checked against the cell grid's shape"""
        out = []
        for name, (g, dtype) in grids.items():
            g = None if g is None else np.ascontiguousarray(g, dtype)
            if g is not None and g.shape != shape:
                raise ValueError("%s: expected a %s grid of shape %r, got %r" % (name, np.dtype(dtype).name, shape, g.shape))
            out.append(g)
        return out

    @staticmethod
    def _rows_and_passes(rows, passes):
        rows, passes = np.ascontiguousarray(rows, ROW_DTYPE), np.ascontiguousarray(passes, np.uint8)
        if rows.shape != (100,) or passes.shape != (100,):
            raise ValueError("expected 100 rows and 100 pass bytes, got %r and %r" % (rows.shape, passes.shape))
        return rows, passes

    def stage_motion_hold(self, now: np.ndarray, ref: Optional[np.ndarray], age: Optional[np.ndarray], width: int, height: int, threshold: int,
                          hold: int, min_cells: int = 1, dilate: int = 1, max_regions: int = 3, min_side: int = 300, pad: int = 8,
                          fmt: int = FMT_RGB24):
        """The region kernel alone as a camera with a hold runs it: `stage_motion_regions` plus the ages `age` (uint8 [cell rows, cell columns];
        None: all zero) and `hold`: (rectangles, the active cells of every region, components, active cells, those of them that did not
        change, the decayed ages)."""
        self._dev_only("stage_motion_hold()")
        shape = (-(-int(height) // _lib.WZ_GATE_CELL), -(-int(width) // _lib.WZ_GATE_CELL))
        now, ref, age = self._motion_grids(shape, now=(now, np.uint16), ref=(ref, np.uint16), age=(age, np.uint8))
        words = self._motion_words(threshold, min_cells, dilate, max_regions, min_side, pad, False)
        most = _lib.WZ_MOTION_MAX_REGIONS
        n, comps, active, held = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        tiles, cells, out = (Tile * most)(), (C.c_int32 * most)(), np.full(shape, 0xA5, np.uint8)
        ptr = lambda g: C.c_void_p(g.ctypes.data) if g is not None else None      # noqa: E731
        self._ck(self._lib.wz_stage_motion_hold(self._h, ptr(now), ptr(ref), ptr(age), int(width), int(height), int(fmt), C.byref(words), int(hold),
                                                C.byref(n), C.byref(tiles), C.byref(cells), C.byref(comps), C.byref(active), C.byref(held), ptr(out)))
        return ([(t.x0, t.y0, t.w, t.h) for t in tiles[:n.value]], [int(v) for v in cells[:n.value]], int(comps.value), int(active.value),
                int(held.value), out)

    def stage_motion_stamp(self, age: np.ndarray, rows: np.ndarray, passes: np.ndarray, width: int, height: int, object_hold: int) -> np.ndarray:
        """The stamp kernel alone: the ages (uint8 [cell rows, cell columns] of a width x height frame) behind 100 rows (ROW_DTYPE) with their
        100 pass bytes."""
        self._dev_only("stage_motion_stamp()")
        shape = (-(-int(height) // _lib.WZ_GATE_CELL), -(-int(width) // _lib.WZ_GATE_CELL))
        age, = self._motion_grids(shape, age=(age, np.uint8))
        rows, passes = self._rows_and_passes(rows, passes)
        out = np.full(shape, 0xA5, np.uint8)
        self._ck(self._lib.wz_stage_motion_stamp(self._h, C.c_void_p(age.ctypes.data), C.c_void_p(rows.ctypes.data), C.c_void_p(passes.ctypes.data),
                                                 int(width), int(height), int(object_hold), C.c_void_p(out.ctypes.data)))
        return out

    def debug_motion_age(self, cam: int) -> np.ndarray:
        """The current ages of camera `cam`'s hold (uint8 [cell rows, cell columns]), once every lane has drained; ValueError if it has none."""
        self._dev_only("debug_motion_age()")
        out = np.full(self._motion_grid.get(int(cam), (1, 1)), 0xA5, np.uint8)
        self._ck(self._lib.wz_debug_motion_age(self._h, int(cam), C.c_void_p(out.ctypes.data)))
        return out

    def profile_motion_hold(self, now: np.ndarray, ref: Optional[np.ndarray], age: Optional[np.ndarray], rows: np.ndarray, passes: np.ndarray,
                            width: int, height: int, threshold: int, hold: int, object_hold: int, min_cells: int = 1, dilate: int = 1,
                            max_regions: int = 3, min_side: int = 300, pad: int = 8, fmt: int = FMT_RGB24, reps: int = 100):
        """(ms of the region launch alone with these ages, ms of the stamp launch alone with these rows and pass bytes, ms of an empty
        bracket): HIP-event brackets, the mean of `reps` each."""
        self._dev_only("profile_motion_hold()")
        shape = (-(-int(height) // _lib.WZ_GATE_CELL), -(-int(width) // _lib.WZ_GATE_CELL))
        now, ref, age = self._motion_grids(shape, now=(now, np.uint16), ref=(ref, np.uint16), age=(age, np.uint8))
        rows, passes = self._rows_and_passes(rows, passes)
        words = self._motion_words(threshold, min_cells, dilate, max_regions, min_side, pad, False)
        reg, stamp, empty = C.c_float(), C.c_float(), C.c_float()
        ptr = lambda g: C.c_void_p(g.ctypes.data) if g is not None else None      # noqa: E731
        self._ck(self._lib.wz_profile_motion_hold(self._h, ptr(now), ptr(ref), ptr(age), int(width), int(height), int(fmt), C.byref(words), int(hold),
                                                  ptr(rows), ptr(passes), int(object_hold), int(reps), C.byref(reg), C.byref(stamp), C.byref(empty)))
        return float(reg.value), float(stamp.value), float(empty.value)

    def profile_gated(self, d_frames: Sequence[int], widths: Sequence[int], heights: Sequence[int], cams: Sequence[int],
                      formats: Optional[Sequence[int]] = None, iou: Optional[float] = None, ios: Optional[float] = None, reps: int = 50):
        """(ms of the activity launch alone, ms of the commit launch alone, ms of an empty bracket) of one gated call on lane 0: HIP-event
        brackets, the mean of `reps` each."""
        self._dev_only("profile_gated()")
        n = len(d_frames)
        fmtv = _i32(n, formats)
        act, commit, empty = C.c_float(), C.c_float(), C.c_float()
        self._ck(self._lib.wz_profile_gated(self._h, n, (C.c_void_p * n)(*d_frames), (C.c_int32 * n)(*widths), (C.c_int32 * n)(*heights), fmtv,
                                            (C.c_int32 * n)(*[int(c) for c in cams]), *self._thresholds(iou, ios), int(reps), C.byref(act),
                                            C.byref(commit), C.byref(empty)))
        self._gate_last[0] = [int(c) for c in cams]
        return float(act.value), float(commit.value), float(empty.value)

    def stage_merge_tiles(self, width: int, height: int, tiles, tile_rows: np.ndarray, iou: float, ios: float, cam: int = -1):
        """The merge kernel on caller-provided rows: tiles = [(x0, y0, w, h), ...], tile_rows ROW_DTYPE [len(tiles), 100] ->
        (rows ROW_DTYPE [100], pass uint8 [100])."""
        self._dev_only("stage_merge_tiles()")
        n = len(tiles)
        arr = self._tile_array(tiles)
        src = np.ascontiguousarray(tile_rows, ROW_DTYPE).reshape(n, MAX_DETECTIONS)
        rows = np.zeros(MAX_DETECTIONS, ROW_DTYPE)
        ok = np.zeros(MAX_DETECTIONS, np.uint8)
        self._ck(self._lib.wz_stage_merge_tiles(self._h, int(width), int(height), int(cam), n, C.byref(arr), C.c_void_p(src.ctypes.data),
                                                  float(iou), float(ios), C.c_void_p(rows.ctypes.data), C.c_void_p(ok.ctypes.data)))
        return rows, ok

    def profile_tiled(self, d_frames: Sequence[int], widths: Sequence[int], heights: Sequence[int], tiles: Sequence,
                      formats: Optional[Sequence[int]] = None, iou: Optional[float] = None, ios: Optional[float] = None, reps: int = 50):
        """(ms of the crop launch alone, ms of the merge launch alone, ms of an empty bracket): HIP-event brackets on lane 0, the mean of
        `reps` each."""
        self._dev_only("profile_tiled()")
        n = len(d_frames)
        counts, tptrs, tkeep, iou, ios = self._tile_args(tiles, n, iou, ios)
        fmtv = _i32(n, formats)
        crop, merge, empty = C.c_float(), C.c_float(), C.c_float()
        self._ck(self._lib.wz_profile_tiled(self._h, n, (C.c_void_p * n)(*d_frames), (C.c_int32 * n)(*widths), (C.c_int32 * n)(*heights),
                                              fmtv, counts, tptrs, iou, ios, int(reps), C.byref(crop), C.byref(merge), C.byref(empty)))
        return float(crop.value), float(merge.value), float(empty.value)

    def stage_rows(self, width: int, height: int, boxes: np.ndarray, scores: np.ndarray, classes: np.ndarray):
        self._dev_only("stage_rows()")
        b = np.ascontiguousarray(boxes, np.float32)
        s = np.ascontiguousarray(scores, np.float32)
        c = np.ascontiguousarray(classes, np.int32)
        rows = np.zeros(MAX_DETECTIONS, ROW_DTYPE)
        self._ck(self._lib.wz_stage_rows(self._h, width, height, C.c_void_p(b.ctypes.data),
                                           C.c_void_p(s.ctypes.data), C.c_void_p(c.ctypes.data),
                                           C.c_void_p(rows.ctypes.data)))
        return rows


def _ignore_plane(mask) -> np.ndarray:
    m = np.asarray(mask)
    if m.ndim != 2 or m.dtype != np.uint8 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError("an ignore mask is a (height, width) uint8 array, got %s of shape %r" % (m.dtype, m.shape))
    return np.ascontiguousarray(m)


def ignore_cells(mask: np.ndarray, rect=None) -> np.ndarray:
    """Host-side: the cell rule of an ignore mask (include/watsor_hip.h: wz_ignore_cells).  mask (H, W) uint8, nonzero = ignore -> uint8
    [cell rows, cell columns] of `rect` = (x0, y0, w, h) (None: the whole frame), 1 where at least one pixel of the 16 x 16-pixel cell
    -- anchored at the rectangle's origin, the last column and row partial -- is ignored."""
    m = _ignore_plane(mask)
    h, w = m.shape
    t = Tile(0, 0, w, h) if rect is None else Tile(*[int(v) for v in rect])
    cells = np.zeros((max(1, -(-t.h // _lib.WZ_GATE_CELL)), max(1, -(-t.w // _lib.WZ_GATE_CELL))), np.uint8)
    rc = _lib.load().wz_ignore_cells(C.c_void_p(m.ctypes.data), w, h, None if rect is None else C.byref(t), C.c_void_p(cells.ctypes.data))
    if rc != _lib.WZ_OK:
        raise ValueError("rectangle (%d, %d, %d x %d) is empty or lies outside the %dx%d ignore mask" % (t.x0, t.y0, t.w, t.h, w, h))
    return cells


def zones_from_alpha(alpha: np.ndarray, max_zones: int = 40):
    """Host-side: alpha plane (H,W) uint8 -> (zone_fill uint8 [nz,H,W], centroids int32 [nz,2])."""
    a = np.ascontiguousarray(alpha, np.uint8)
    h, w = a.shape
    fill = np.zeros((max_zones, h, w), np.uint8)
    cent = np.zeros((max_zones, 2), np.int32)
    rc = _lib.load().wz_zones_from_alpha(C.c_void_p(a.ctypes.data), w, h, max_zones, C.c_void_p(fill.ctypes.data),
                                         C.c_void_p(cent.ctypes.data))
    if rc == _lib.WZ_EFORMAT:
        raise ZeroDivisionError("float division by zero")     # what mask.py:80 raises for a degenerate contour
    if rc < 0:
        raise ValueError("wz_zones_from_alpha failed (%d)" % rc)
    return fill[:rc].copy(), cent[:rc].copy()
