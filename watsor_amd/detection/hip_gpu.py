"""`HipObjectDetector` -- the MI355X detector plugin.

Satisfies the duck-typed protocol every reference detector implements
(`watsor/detection/tensorflow_cpu.py:13,64-92`, `tensorrt_gpu.py:20,55-91`,
`tensorflow_lite_cpu.py:16,25-62`, `edge_tpu.py:17,24-57`):

    __init__(model_path, device)    raises FileNotFoundError when model/mi355x.bin is absent
    device_name -> str
    __enter__ / __exit__            frees device state
    detect(image_shape, image_np, detections) -> milliseconds

so `ObjectDetector._run/_next_frame` (`watsor/detection/detector.py:84-112`) drives it unchanged.
`detect()` hands the frame pointer and the ctypes `Detection[100]` array straight to
`wz_detect_batch`; the 100 rows (class, score, pixel box -- `tensorflow_cpu.py:79-90`) are produced
on the GPU and written in place.  `detect_batch()` is the same call for several frames (BASELINE
config 2: batch = 8), used by `BatchedObjectDetector`.
"""
from __future__ import annotations

import itertools
import os
from typing import List, Optional, Sequence

import numpy as np

from ..runtime import (CSP_BT709, FMT_BASE_MASK, FMT_BGR24, FMT_GRAY8, FMT_I420, FMT_NV12, FMT_P010, FMT_RGB24, FMT_UYVY422, FMT_YUV420P10,
                       FMT_YUYV422, RANGE_FULL, TEN_BIT_FORMATS, YUV_FORMATS, HipEngine, frame_shape, tile_grid)
from .._lib import WZ_MAX_TILES, WZ_MOTION_MAX_REGIONS
from ..share import Detection

# what a decoder's `-pix_fmt` may say (watsor/stream/ffmpeg.py:78-88 reads whatever it writes; the reference's schema asks for
# rgb24, `watsor/config/schema.py:161` -- NV12 / yuv420p frames are half the bytes and are converted on the GPU, SURVEY 8f-3;
# yuyv422 / uyvy422 is what USB / V4L2 cameras and capture cards write, gray what IR / thermal cameras do, yuvj420p -- yuv420p with
# full-range levels -- what MJPEG cameras decode to; p010le / yuv420p10le -- 10-bit 4:2:0, a 16-bit word per sample -- what an HEVC
# Main10 stream decodes to on a hardware / in a software decoder: as many bytes as rgb24, but no conversion on the host)
PIXEL_FORMATS = {"rgb24": FMT_RGB24, "nv12": FMT_NV12, "yuv420p": FMT_I420, "i420": FMT_I420, "yuyv422": FMT_YUYV422,
                 "uyvy422": FMT_UYVY422, "gray": FMT_GRAY8, "yuvj420p": FMT_I420 | RANGE_FULL,
                 "p010le": FMT_P010, "yuv420p10le": FMT_YUV420P10}
# how a camera's YUV frames turn into RGB (include/watsor_hip.h: the colour flags of the format word)
COLOR_MATRICES = {"bt601": 0, "bt709": CSP_BT709}
COLOR_RANGES = {"limited": 0, "full": RANGE_FULL}

ENGINE_FILE = "mi355x.bin"       # the analogue of gpu.trt (watsor/detection/detector.py:44)


def pixel_format_code(name) -> int:
    try:
        return PIXEL_FORMATS[str(name).lower()]
    except KeyError:
        raise ValueError("pixel_format %r: expected one of %s" % (name, ", ".join(sorted(PIXEL_FORMATS)))) from None


def _option_code(option: str, table: dict, name) -> int:
    try:
        return table[str(name).lower()]
    except KeyError:
        raise ValueError("%s %r: expected one of %s" % (option, name, ", ".join(sorted(table)))) from None


def format_words(options: dict):
    """(default format word, {camera name: format word}) from the plugin options `pixel_format`, `color_matrix` ("bt601" | "bt709") and
    `color_range` ("limited" | "full"), each a single value or {camera name: value}.  The matrix and the range only mean something
    for a YUV format: an RGB24 or gray camera under a detector-wide "bt709" keeps its plain word.  Unknown names, options and values
    raise ValueError."""
    tables = (("pixel_format", PIXEL_FORMATS, "rgb24"), ("color_matrix", COLOR_MATRICES, "bt601"), ("color_range", COLOR_RANGES, "limited"))
    defaults, by_name = [], []
    for option, table, plain in tables:
        v = options.get(option) or plain
        per = {str(k): _option_code(option, table, x) for k, x in v.items()} if isinstance(v, dict) else {}
        defaults.append(table[plain] if isinstance(v, dict) else _option_code(option, table, v))
        by_name.append(per)

    def word(fmt, matrix, rng):
        return fmt | matrix | rng if (fmt & FMT_BASE_MASK) in YUV_FORMATS else fmt

    names = set().union(*by_name)
    return word(*defaults), {n: word(*[per.get(n, dflt) for per, dflt in zip(by_name, defaults)]) for n in names}


def _planar_format(default: int, by_camera: dict) -> int:
    """What a one-channel buffer shaped (H*3/2, W) holds when its camera says RGB24: the one planar 4:2:0 format that is configured
    (NV12 if none is).  Only NV12 / I420 have that shape -- a configured gray or 4:2:2 camera is never the answer, and neither is a
    10-bit one (p010le / yuv420p10le are taken by configuration only)."""
    return next((f for f in [default] + list(by_camera.values()) if (f & FMT_BASE_MASK) in (FMT_NV12, FMT_I420)), FMT_NV12)


_TABLE_SHAPES = {   # what the frame table says of a frame buffer whose header is no frame of its camera's format (runtime.frame_shape)
    **dict.fromkeys((FMT_NV12, FMT_I420), "an NV12 / I420 frame buffer must be (H*3/2, W, 1) with even H and W"),
    **dict.fromkeys(TEN_BIT_FORMATS, "a P010 / YUV420P10 frame buffer must be (H*3/2, W, 2) or (H*3/2, 2W, 1) with even H and W"),
    **dict.fromkeys((FMT_YUYV422, FMT_UYVY422), "a YUYV422 / UYVY422 frame buffer must be (H, W, 2) or (H, 2W, 1) with even W"),
    FMT_GRAY8: "a gray frame buffer must have 1 channel",
    **dict.fromkeys((FMT_RGB24, FMT_BGR24), "an RGB24 / BGR24 frame buffer must have 3 channels"),
}


def frame_formats(frames: Sequence[np.ndarray], cameras: Optional[Sequence[int]], default: int, by_camera: dict):
    """Format word of every frame of a call: the camera's configured one, else the detector's; a planar (2-D) array that would
    be read as RGB24 takes the one planar YUV format that is configured (NV12 if none is).  None = all RGB24."""
    yuv = _planar_format(default, by_camera)
    out = []
    for i, f in enumerate(frames):
        fmt = by_camera.get(cameras[i], default) if cameras is not None else default
        if fmt == FMT_RGB24 and (f.ndim == 2 or (f.ndim == 3 and f.shape[2] == 1)):
            fmt = yuv
        out.append(fmt)
    return out if any(f != FMT_RGB24 for f in out) else None


_TILE_KEYS = {"grid", "overlap", "full_frame", "iou", "ios", "rects", "gate"}
_GATE_KEYS = {"threshold", "min_cells", "max_age"}


def _tile_spec(spec, where: str) -> dict:
    """One checked `tiles` option: {"grid": [cols, rows], "overlap": 0.2, "full_frame": True, "iou": ..., "ios": ...} or
    {"rects": [[x0, y0, w, h], ...], "iou": ..., "ios": ...}, either with "gate": {"threshold": 0 .. 255, "min_cells": >= 1 (default 1),
    "max_age": >= 0 (default 0)} -- run a tile only where its picture changed (`HipEngine.set_camera_tiles`).  Anything else raises
    ValueError."""
    if not isinstance(spec, dict) or ("grid" in spec) == ("rects" in spec):
        raise ValueError("%s: expected {\"grid\": [cols, rows], ...} or {\"rects\": [[x0, y0, w, h], ...]}, got %r" % (where, spec))
    if set(spec) - _TILE_KEYS:
        raise ValueError("%s: unknown key(s) %s" % (where, ", ".join(sorted(map(str, set(spec) - _TILE_KEYS)))))
    out = {"iou": spec.get("iou"), "ios": spec.get("ios")}
    for k in ("iou", "ios"):
        v = out[k]
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0):
            raise ValueError("%s: %s %r, expected a number >= 0" % (where, k, v))
    def whole(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if "grid" in spec:
        g = spec["grid"]
        if not isinstance(g, (list, tuple)) or len(g) != 2 or not all(whole(v) and v >= 1 for v in g):
            raise ValueError("%s: grid %r, expected [cols, rows] with both >= 1" % (where, g))
        ov = spec.get("overlap", 0.0)
        if isinstance(ov, bool) or not isinstance(ov, (int, float)) or not 0.0 <= ov < 1.0:
            raise ValueError("%s: overlap %r, expected 0 <= overlap < 1" % (where, ov))
        full = spec.get("full_frame", True)
        if not isinstance(full, bool):
            raise ValueError("%s: full_frame %r, expected true or false" % (where, full))
        out.update(grid=(g[0], g[1]), overlap=float(ov), full_frame=full, count=g[0] * g[1] + (1 if full and g[0] * g[1] > 1 else 0))
    else:
        if "overlap" in spec or "full_frame" in spec:
            raise ValueError("%s: overlap / full_frame belong to a grid, not to rects" % where)
        r = spec["rects"]
        if not isinstance(r, (list, tuple)) or not r or not all(
                isinstance(t, (list, tuple)) and len(t) == 4 and all(whole(v) for v in t) and t[0] >= 0 and t[1] >= 0 and t[2] >= 1 and t[3] >= 1
                for t in r):
            raise ValueError("%s: rects %r, expected a non-empty list of [x0, y0, w, h] with x0, y0 >= 0 and w, h >= 1" % (where, r))
        out.update(rects=[tuple(t) for t in r], count=len(r))
    if out["count"] > WZ_MAX_TILES:
        raise ValueError("%s: %d tiles, a frame takes at most %d" % (where, out["count"], WZ_MAX_TILES))
    if "gate" in spec:
        g = spec["gate"]
        if not isinstance(g, dict) or "threshold" not in g:
            raise ValueError("%s: gate %r, expected {\"threshold\": 0 .. 255, \"min_cells\": >= 1, \"max_age\": >= 0}" % (where, g))
        if set(g) - _GATE_KEYS:
            raise ValueError("%s: gate: unknown key(s) %s" % (where, ", ".join(sorted(map(str, set(g) - _GATE_KEYS)))))
        gate = (g["threshold"], g.get("min_cells", 1), g.get("max_age", 0))
        if not all(whole(v) for v in gate):
            raise ValueError("%s: gate %r, expected whole numbers" % (where, g))
        if not 0 <= gate[0] <= 255:
            raise ValueError("%s: gate: threshold %r, expected 0 .. 255" % (where, gate[0]))
        if gate[1] < 1:
            raise ValueError("%s: gate: min_cells %r, expected >= 1" % (where, gate[1]))
        if gate[2] < 0:
            raise ValueError("%s: gate: max_age %r, expected >= 0" % (where, gate[2]))
        out["gate"] = gate
    return out


def tile_options(options: dict):
    """(the detector's tiles or None, {camera name: tiles}) from the plugin option `tiles`: one description (see `_tile_spec`) for
    every camera, or {camera name: description}.  Bad options raise ValueError."""
    v = options.get("tiles")
    if v is None:
        return None, {}
    if isinstance(v, dict) and ("grid" in v or "rects" in v):
        return _tile_spec(v, "tiles"), {}
    if not isinstance(v, dict) or not v:
        raise ValueError("tiles: expected a description of the tiles or {camera name: description}, got %r" % (v,))
    return None, {str(name): _tile_spec(spec, "tiles[%r]" % (name,)) for name, spec in v.items()}


_MOTION_KEYS = {"threshold", "min_cells", "dilate", "max_regions", "min_side", "pad", "whole_frame", "iou", "ios"}
# key -> (default, smallest, largest or None) of the whole numbers of a `motion` description
_MOTION_RANGES = {"threshold": (None, 0, 255), "min_cells": (1, 1, None), "dilate": (1, 0, 2), "max_regions": (3, 1, WZ_MOTION_MAX_REGIONS),
                  "min_side": (300, 16, None), "pad": (8, 0, 64)}


def _motion_spec(spec, where: str) -> dict:
    """One checked `motion` option: {"threshold": 0 .. 255, "min_cells": >= 1 (default 1), "dilate": 0 .. 2 (1), "max_regions": 1 .. 16 (3),
    "min_side": >= 16 (300), "pad": 0 .. 64 (8), "whole_frame": true | false (true), "iou": ..., "ios": ...} -- find the parts of the picture
    that moved since the camera's previous frame and run the detector there at the camera's own resolution
    (`HipEngine.set_camera_motion`).  Anything else raises ValueError."""
    if not isinstance(spec, dict) or "threshold" not in spec:
        raise ValueError("%s: expected {\"threshold\": 0 .. 255, \"min_cells\": >= 1, \"dilate\": 0 .. 2, \"max_regions\": 1 .. %d, \"min_side\": >= 16, "
                         "\"pad\": 0 .. 64, \"whole_frame\": true | false}, got %r" % (where, WZ_MOTION_MAX_REGIONS, spec))
    if set(spec) - _MOTION_KEYS:
        raise ValueError("%s: unknown key(s) %s" % (where, ", ".join(sorted(map(str, set(spec) - _MOTION_KEYS)))))
    out = {"iou": spec.get("iou"), "ios": spec.get("ios")}
    for k in ("iou", "ios"):
        v = out[k]
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0):
            raise ValueError("%s: %s %r, expected a number >= 0" % (where, k, v))
    for k, (default, low, high) in _MOTION_RANGES.items():
        v = spec.get(k, default)
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError("%s: %s %r, expected a whole number" % (where, k, v))
        if v < low or (high is not None and v > high):
            raise ValueError("%s: %s %r, expected %s" % (where, k, v, ">= %d" % low if high is None else "%d .. %d" % (low, high)))
        out[k] = v
    whole = spec.get("whole_frame", True)
    if not isinstance(whole, bool):
        raise ValueError("%s: whole_frame %r, expected true or false" % (where, whole))
    out.update(whole_frame=whole, count=(1 if whole else 0) + out["max_regions"])
    return out


def motion_options(options: dict):
    """(the detector's motion settings or None, {camera name: settings}) from the plugin option `motion`: one description (see
    `_motion_spec`) for every camera, or {camera name: description}.  Bad options raise ValueError."""
    v = options.get("motion")
    if v is None:
        return None, {}
    if isinstance(v, dict) and "threshold" in v:
        return _motion_spec(v, "motion"), {}
    if not isinstance(v, dict) or not v or not all(isinstance(d, dict) for d in v.values()):
        raise ValueError("motion: expected a description of the motion settings or {camera name: description}, got %r" % (v,))
    return None, {str(name): _motion_spec(d, "motion[%r]" % (name,)) for name, d in v.items()}


def check_motion_options(motion_default, motion_by_name: dict, tiles_default, tiles_by_name: dict, max_batch: int) -> None:
    """What `motion_options` cannot see on its own: the settings' whole_frame + max_regions must fit max_batch, and a camera takes `motion`
    or `tiles`, not both.  Raises ValueError; the message begins with the option at fault."""
    for where, spec in [("motion", motion_default)] + [("motion[%r]" % n, m) for n, m in motion_by_name.items()]:
        if spec is not None and spec["count"] > max_batch:
            raise ValueError("%s: whole_frame + max_regions = %d tiles per frame exceed max_batch %d" % (where, spec["count"], max_batch))
    if motion_default is not None and (tiles_default is not None or tiles_by_name):
        raise ValueError("motion: set for every camera together with tiles: a camera takes one of the two")
    if tiles_default is not None and motion_by_name:
        raise ValueError("motion[%r]: tiles are set for every camera: a camera takes one of the two" % (sorted(motion_by_name)[0],))
    both = sorted(set(motion_by_name) & set(tiles_by_name))
    if both:
        raise ValueError("motion[%r]: the camera has tiles too: a camera takes one of the two" % (both[0],))


_MOTION_HOLD_KEYS = ("hold", "object_hold")


def _motion_hold_spec(spec, where: str) -> dict:
    """One checked `motion_hold` option: {"hold": 0 .. 255 (default 0), "object_hold": 0 .. 255 (0)}, not both 0."""
    if not isinstance(spec, dict):
        raise ValueError("%s: expected {\"hold\": 0 .. 255, \"object_hold\": 0 .. 255}, got %r" % (where, spec))
    if set(spec) - set(_MOTION_HOLD_KEYS):
        raise ValueError("%s: unknown key(s) %s" % (where, ", ".join(sorted(map(str, set(spec) - set(_MOTION_HOLD_KEYS))))))
    out = {}
    for k in _MOTION_HOLD_KEYS:
        v = spec.get(k, 0)
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError("%s: %s %r, expected a whole number" % (where, k, v))
        if v < 0 or v > 255:
            raise ValueError("%s: %s %r, expected 0 .. 255" % (where, k, v))
        out[k] = v
    if not any(out.values()):
        raise ValueError("%s: hold and object_hold are both 0: leave the option out for a camera without a hold" % where)
    return out


def motion_hold_options(options: dict, motion_default, motion_by_name: dict):
    """(the detector's hold or None, {camera name: hold}) from the plugin option `motion_hold`: {"hold": 0 .. 255, "object_hold": 0 .. 255}
    for every camera with motion settings, or {camera name: such a description} -- a motion camera keeps a cell in its regions for `hold`
    further frames after it changed, and for `object_hold` further frames after a detection that passed the camera's filters covered it
    (`HipEngine.set_camera_motion_hold`).  motion_default, motion_by_name: what `motion_options` returned -- a hold needs motion settings.
    Bad options raise ValueError; the message begins with the option at fault."""
    v = options.get("motion_hold")
    if v is None:
        return None, {}
    if isinstance(v, dict) and v and not any(isinstance(d, dict) for d in v.values()):
        spec = _motion_hold_spec(v, "motion_hold")
        if motion_default is None and not motion_by_name:
            raise ValueError("motion_hold: there is no motion option: a hold keeps motion regions alive")
        return spec, {}
    if not isinstance(v, dict) or not v or not all(isinstance(d, dict) for d in v.values()):
        raise ValueError("motion_hold: expected {\"hold\": 0 .. 255, \"object_hold\": 0 .. 255} or {camera name: such a description}, got %r" % (v,))
    by_name = {str(name): _motion_hold_spec(d, "motion_hold[%r]" % (name,)) for name, d in v.items()}
    for name in by_name:
        if motion_default is None and name not in motion_by_name:
            raise ValueError("motion_hold[%r]: the camera has no motion option: a hold keeps motion regions alive" % (name,))
    return None, by_name


_IGNORE_FORMS = "a list of [x, y, w, h] pixel rectangles, an (H, W) uint8 array or the name of a mask file"


def _ignore_spec(spec, where: str):
    """One checked `ignore` description -> ("rects", [(x, y, w, h), ...]) | ("mask", (H, W) uint8 array) | ("file", name)."""
    if isinstance(spec, np.ndarray):
        if spec.ndim != 2 or spec.dtype != np.uint8 or 0 in spec.shape:
            raise ValueError("%s: an array of shape %r and type %s, expected (H, W) uint8" % (where, spec.shape, spec.dtype))
        return "mask", np.ascontiguousarray(spec)
    if isinstance(spec, (str, os.PathLike)):
        return "file", os.fspath(spec)
    if not isinstance(spec, (list, tuple)) or not spec:
        raise ValueError("%s: expected %s, got %r" % (where, _IGNORE_FORMS, spec))
    whole = lambda v: isinstance(v, int) and not isinstance(v, bool)      # noqa: E731
    rects = []
    for r in spec:
        if not isinstance(r, (list, tuple)) or len(r) != 4 or not all(whole(v) for v in r) or r[0] < 0 or r[1] < 0 or r[2] < 1 or r[3] < 1:
            raise ValueError("%s: rectangle %r, expected [x, y, w, h]: whole numbers, x and y >= 0, w and h >= 1" % (where, r))
        rects.append(tuple(r))
    return "rects", rects


def ignore_options(options: dict, motion_default, motion_by_name: dict, tiles_default, tiles_by_name: dict) -> dict:
    """{camera name: checked description} from the plugin option `ignore`: {camera name: a list of [x, y, w, h] pixel rectangles (a
    burnt-in clock) | an (H, W) uint8 array, nonzero = ignore | the name of a mask file read with `read_mask_alpha`, alpha > 0 = ignore}
    -- where the camera's picture changes without anything moving (`HipEngine.set_camera_ignore`).  Per camera name only: a mask is a
    picture of one camera's view.  The other arguments are what `motion_options` and `tile_options` returned: a mask silences change,
    so its camera needs `motion` or tiles with a "gate".  Bad options raise ValueError; the message begins with the option at fault."""
    v = options.get("ignore")
    if v is None:
        return {}
    if not isinstance(v, dict) or not v:
        raise ValueError("ignore: expected {camera name: %s}, got %r" % (_IGNORE_FORMS, v))
    out = {}
    for name, spec in v.items():
        where = "ignore[%r]" % (name,)
        out[str(name)] = _ignore_spec(spec, where)
        tiles = tiles_by_name.get(str(name), tiles_default)
        if motion_default is None and str(name) not in motion_by_name and (tiles is None or "gate" not in tiles):
            raise ValueError("%s: the camera has neither a motion option nor tiles with a gate: an ignore mask silences change, and nothing "
                             "of this camera looks for change" % where)
    return out


def check_ignore_cameras(ignore_by_name: dict, names) -> None:
    """What `ignore_options` cannot see on its own: every camera it names must be one of the detector's cameras `names` (the keys of the
    worker's frame buffers).  Raises ValueError."""
    for name in sorted(set(ignore_by_name) - {str(n) for n in names}):
        raise ValueError("ignore[%r]: unknown camera, this detector's cameras are %s" % (name, ", ".join(repr(str(n)) for n in names) or "none"))


def ignore_plane(spec, where: str, width: int, height: int) -> np.ndarray:
    """The (height, width) uint8 ignore plane, nonzero = ignore, of a checked `ignore` description for a camera's width x height frames.
    ValueError for a rectangle that does not lie inside the frame and for a mask of another size."""
    kind, v = spec
    if kind == "rects":
        plane = np.zeros((height, width), np.uint8)
        for x, y, w, h in v:
            if x + w > width or y + h > height:
                raise ValueError("%s: rectangle %r does not lie inside the camera's %dx%d frame" % (where, [x, y, w, h], width, height))
            plane[y:y + h, x:x + w] = 1
        return plane
    if kind == "file":
        from ..filter.hip_filter import read_mask_alpha
        try:
            v = (read_mask_alpha(v) > 0).astype(np.uint8)
        except AssertionError as e:
            raise ValueError("%s: %s" % (where, e))
    if v.shape != (height, width):
        raise ValueError("%s: the mask is %dx%d (width x height) but the camera's frames are %dx%d" % (where, v.shape[1], v.shape[0], width, height))
    return v


def cut_calls(items, max_batch: int):
    """Cuts a list of frames into the consecutive calls one rule allows: items[i] = (key, cost, camera that may appear once per call, or
    None); a new call starts when the key changes, when the cost would pass max_batch, or when such a camera appears again.  Returns the
    calls as lists of indices into `items`, in order.  A pure function."""
    calls, call, key, used, once = [], [], None, 0, set()
    for i, (k, cost, cam) in enumerate(items):
        if call and (k != key or used + cost > max_batch or (cam is not None and cam in once)):
            calls.append(call)
            call, used, once = [], 0, set()
        key = k
        call.append(i)
        used += cost
        if cam is not None:
            once.add(cam)
    if call:
        calls.append(call)
    return calls


def plan_bound(descriptions, entries, max_batch: int):
    """Cuts a list of frame-table indices into the calls `wz_submit_bound` accepts, in order (include/watsor_hip.h): every call holds one
    kind -- untiled, tiled, gated or motion -- and one pair of merge thresholds, at most max_batch frames whose tiles (gated: their cameras'
    configured tiles; motion: their cameras' configured whole_frame + max_regions) together fit max_batch, and at most one frame of a gated
    or motion camera.  The calls are consecutive pieces of `entries`, so a camera's frames keep their order.  descriptions[i] = (kind, iou,
    ios, tiles, camera id) of table entry i with kind "plain" | "tiled" | "gated" | "motion" (what `bind_tiled_frame_table` recorded); an
    index beyond them counts as plain.  A pure function."""
    items = []
    for e in entries:
        kind, iou, ios, tiles, cam = descriptions[e] if 0 <= e < len(descriptions) else ("plain", None, None, 1, -1)
        if kind == "plain":
            items.append((("plain",), 1, None))      # (a cost of 1 each: at most max_batch frames)
        else:
            items.append(((kind, iou, ios), tiles, cam if kind in ("gated", "motion") else None))
    return [[entries[i] for i in call] for call in cut_calls(items, max_batch)]


class HipObjectDetector:
    """Performs object detection on AMD Instinct MI355X GPUs (hand-written HIP kernels)."""

    bound_max_batch = None          # the batch limit `plan_bound` cuts for (None: the engine's max_batch)

    def __init__(self, model_path, device: int = 0, options: Optional[dict] = None, max_batch: Optional[int] = None,
                 max_width: Optional[int] = None, max_height: Optional[int] = None):
        """`options` (third positional argument, what `create_object_detectors` passes in `detector_args`):
        dict(max_batch=, max_width=, max_height=) -- the factory derives the frame size from the cameras' frame buffers;
        the keyword forms and the WATSOR_HIP_MAX_* environment variables are the fallbacks.
        `options["pixel_format"]`: "rgb24" (default) | "nv12" | "yuv420p" | "yuvj420p" | "yuyv422" | "uyvy422" | "gray" | "p010le" |
        "yuv420p10le", or {camera name: one of these} -- what the cameras' decoders write into their frame buffers.  An NV12 / yuv420p
        frame is handed over as the (H*3/2, W) uint8 array of its bytes (that is its `image_shape`), a yuyv422 / uyvy422 frame as
        (H, W, 2) or (H, 2W), a gray frame as (H, W) or (H, W, 1), a 10-bit p010le / yuv420p10le frame (a 16-bit word per sample: as many
        bytes as rgb24 -- what it saves is swscale's conversion on the host, not bytes) as (H*3/2, W) uint16 or as its bytes, (H*3/2, W, 2)
        or (H*3/2, 2W) uint8.
        `options["color_matrix"]`: "bt601" (default) | "bt709", `options["color_range"]`: "limited" (default) | "full", each a single
        value or {camera name: value} -- how the YUV formats are converted (an HD stream tagged bt709; a full-range MJPEG camera);
        "yuvj420p" is "yuv420p" with the full range.
        `options["tiles"]`: run the detector on rectangles of every frame instead of the whole frame squeezed into the network's
        input, and report one merged list of rows in frame coordinates (include/watsor_hip.h: wz_detect_tiled).
        {"grid": [cols, rows], "overlap": 0.2, "full_frame": True, "iou": ..., "ios": ...} -- `tile_grid` of every frame's size; "iou" /
        "ios": a row goes when a more confident row of its label overlaps it by more than `iou` (intersection over union, default: the
        engine's NMS threshold) or by more than `ios` of the smaller box (default 1.0: off; 0.5 - 0.7 merges an object cut by a tile's
        border with its whole box) -- or explicit {"rects": [[x0, y0, w, h], ...]}, or {camera name: one of these}.  The tiles of one
        frame must fit max_batch; `detect_batch` cuts a batch into as many calls as its tiles need.  With "gate": {"threshold": 0 .. 255,
        "min_cells": 1, "max_age": 0} in a description, a frame that comes with a camera id runs only the tiles whose picture changed
        since they last ran (include/watsor_hip.h: wz_detect_gated; the luma sum of a 16 x 16 cell must move by more than `threshold`
        per pixel, in `min_cells` cells; `max_age` > 0 runs a tile after that many skipped calls whatever it shows) and reuses the
        other tiles' rows; a frame without a camera id runs every tile as before.  The batched worker's frame table
        takes tiles through `bind_tiled_frame_table` (the worker's `hip_tiled_table`); `bind_frame_table` raises for a camera with tiles.
        `options["motion"]`: run the detector at the camera's own resolution where the picture moved since the camera's previous
        frame (include/watsor_hip.h: wz_detect_motion): {"threshold": 0 .. 255, "min_cells": 1, "dilate": 1, "max_regions": 3, "min_side": 300,
        "pad": 8, "whole_frame": True, "iou": ..., "ios": ...} or {camera name: one of these}.  A 16 x 16 cell has changed when its luma sum
        moved by more than `threshold` per pixel; changed cells, dilated by `dilate` cells, are joined into components, and the heaviest
        components with at least `min_cells` changed cells become up to `max_regions` rectangles of at least `min_side` pixels a side,
        `pad` pixels around the cells; `whole_frame` runs the squeezed whole frame beside them; "iou" / "ios" merge as for `tiles`.  A
        camera takes `motion` or `tiles`, not both; its frames need a camera id and go through `detect_batch` (cut into calls whose
        configured whole_frame + max_regions fit max_batch) -- or through the batched worker's frame table: `bind_tiled_frame_table` (the
        worker's `hip_tiled_table`) binds such a camera's frames as motion entries (wz_bind_motion); `bind_frame_table` raises for it.
        `options["motion_hold"]`: {"hold": 0 .. 255, "object_hold": 0 .. 255} (not both 0) for every camera with `motion`, or {camera name:
        one of these}: a cell stays part of the camera's regions for `hold` further frames after it changed, and for `object_hold`
        further frames after a detection that passed the camera's filters covered it -- a person who stops moving, a parked car the
        whole-frame tile found (include/watsor_hip.h: wz_set_camera_motion_hold).  A camera without `motion` cannot have one.
        `options["ignore"]`: {camera name: [[x, y, w, h], ...] | (H, W) uint8 array | mask file name} -- the parts of that camera's picture
        that change without anything moving: a burnt-in clock (the rectangles), a flag, a hedge, a road behind the fence (an array,
        nonzero = ignore, or a 32-bit mask image as the zones use, alpha > 0 = ignore).  A 16 x 16 cell with at least one ignored pixel
        never counts as changed, neither for `motion` nor for a "gate" (include/watsor_hip.h: wz_set_camera_ignore); detections inside
        the area are reported as ever.  Per camera name only; the camera needs `motion` or tiles with a "gate", and -- like every
        per-camera option -- takes effect for the ids `bind_cameras` hands out.
        `options["schedule"]`: "latency" | "throughput" | "auto" (default) -- the launch shapes of this detector PROCESS
        (include/watsor_hip.h: wz_set_schedule).  "latency" makes a lone batch finish soonest -- the reference's normal load is one
        frame at a time (`_next_frame`, detector.py:102-112); "throughput" gets the most frames per second out of four batches in
        flight.  "auto" leaves what is in force (WZ_SCHEDULE, else throughput) -- the factory resolves it by the number of cameras
        (`hip_detector_options`: latency for up to 4).
        `options["numa"]`: True | False | "auto" (default) -- pin this process to the CPUs local to the GPU before the engine
        allocates its page-locked blocks (watsor_amd/numa.py); "auto": only on hosts with more than one GPU."""
        engine_path = os.path.join(model_path, ENGINE_FILE)
        if not os.path.isfile(engine_path):
            raise FileNotFoundError(engine_path)
        options = options or {}
        schedule = str(options.get("schedule") or "auto").lower()
        if schedule not in ("auto", "latency", "throughput", "auto:latency", "auto:throughput"):
            raise ValueError("schedule %r: expected latency, throughput or auto" % (options.get("schedule"),))
        # "auto:<name>" (what the factory's `auto` resolves to) is a PREFERENCE: the schedule is the process's (wz_set_schedule), and a
        # process that has fixed the other one already -- Thread delegates, an engine or filter created earlier, a second factory
        # call -- keeps it; only an operator's explicit "latency" / "throughput" is a demand (ValueError when it cannot be met)
        soft = schedule.startswith("auto:")
        schedule = None if schedule == "auto" else schedule.split(":")[-1]
        self.schedule_note = None
        if soft:
            from ..runtime import get_schedule, set_schedule
            try:
                set_schedule(schedule)
            except ValueError:
                self.schedule_note = "schedule %r preferred for this camera count, %r already in force in this process: kept" % (schedule, get_schedule())
                import logging
                logging.getLogger(__name__).info(self.schedule_note)
            schedule = None
        self.numa = None
        self.arena_nodes = None
        numa = options.get("numa", "auto")
        if numa is True or (numa == "auto" and self._several_gpus()):
            from ..numa import pin_to_gpu_node
            self.numa = pin_to_gpu_node(device)
        max_batch = max_batch or options.get("max_batch") or int(os.environ.get("WATSOR_HIP_MAX_BATCH", "8"))
        max_width = max_width or options.get("max_width") or int(os.environ.get("WATSOR_HIP_MAX_WIDTH", "1920"))
        max_height = max_height or options.get("max_height") or int(os.environ.get("WATSOR_HIP_MAX_HEIGHT", "1080"))
        self.__fmt_default, self.__fmt_by_name = format_words(options)
        self.__fmt_by_cam = {}
        self.__tiles_default, self.__tiles_by_name = tile_options(options)
        self.__tiles_by_cam = {}
        self.__tile_rects = {}
        self.__gate_layouts = {}        # camera id -> what its tiles were last set for: (width, height, base format, rectangles, gate)
        self.bound_descriptions = []    # per frame-table entry: (kind, iou, ios, tiles, camera id), see `plan_bound`
        self.__motion_default, self.__motion_by_name = motion_options(options)
        self.__motion_by_cam = {}
        self.__motion_layouts = {}      # camera id -> what its motion settings were last made for: (width, height, base format, settings)
        self.__hold_default, self.__hold_by_name = motion_hold_options(options, self.__motion_default, self.__motion_by_name)
        self.__hold_by_cam = {}
        self.__ignore_by_name = ignore_options(options, self.__motion_default, self.__motion_by_name, self.__tiles_default, self.__tiles_by_name)
        self.__ignore_by_cam = {}       # camera id -> (camera name, checked description)
        for where, spec in [("tiles", self.__tiles_default)] + [("tiles[%r]" % n, t) for n, t in self.__tiles_by_name.items()]:
            if spec is not None and spec["count"] > max_batch:
                raise ValueError("%s: %d tiles per frame exceed max_batch %d" % (where, spec["count"], max_batch))
        check_motion_options(self.__motion_default, self.__motion_by_name, self.__tiles_default, self.__tiles_by_name, max_batch)
        self._warn_short_of_queues()
        self.__engine = HipEngine(engine_path, device, max_batch, max_width, max_height, schedule=schedule)
        self.__device = device
        self.__filters = []
        self.__pinned = []

    _queues_warned = False

    def _warn_short_of_queues(self) -> None:
        """One warning per process when GPU_MAX_HW_QUEUES is below two per lane (include/watsor_hip.h: wz_hw_queues): lanes that share a
        hardware queue serialise.  The library sets 8 when it loads, so this means the variable was changed afterwards -- or that the
        process initialised HIP first and the figure below is not even what the runtime uses."""
        from ..runtime import hw_queues
        try:
            lanes = int(os.environ.get("WZ_LANES", ""))        # the lanes wz_create will make: WZ_LANES = 1 .. 8, else 4
        except ValueError:
            lanes = 0
        have, want = hw_queues(), 2 * (lanes if 1 <= lanes <= 8 else 4)
        if have < want and not HipObjectDetector._queues_warned:
            HipObjectDetector._queues_warned = True
            import logging
            logging.getLogger(__name__).warning(
                "GPU_MAX_HW_QUEUES is %s, %d lanes want %d hardware queues: lanes that share a queue run one after the other "
                "(set it to %d or leave it unset before this process's first HIP call)" % (have or "not a number", want // 2, want, want))

    @staticmethod
    def _several_gpus() -> bool:
        from ..runtime import device_count
        try:
            return device_count() > 1
        except (OSError, RuntimeError):
            return False

    @property
    def schedule(self) -> str:
        return self.__engine.schedule

    def _formats(self, frames: Sequence[np.ndarray], cameras: Optional[Sequence[int]]):
        return frame_formats(frames, cameras, self.__fmt_default, self.__fmt_by_cam)

    @property
    def tiled(self) -> bool:
        """A `tiles` option is set (for every camera or for some): frames go through `detect()` / `detect_batch()`, or through a frame
        table bound with `bind_tiled_frame_table`."""
        return self.__tiles_default is not None or bool(self.__tiles_by_name)

    @property
    def motion(self) -> bool:
        """A `motion` option is set (for every camera or for some): frames go through `detect_batch()` with camera ids, or through a frame
        table bound with `bind_tiled_frame_table`."""
        return self.__motion_default is not None or bool(self.__motion_by_name)

    @property
    def engine(self) -> HipEngine:
        return self.__engine

    @property
    def max_batch(self) -> int:
        return self.__engine.max_batch

    @property
    def device_name(self):
        return self.__engine.device_name

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        try:
            self.__engine.sync()
            for addr in self.__pinned:
                try:
                    self.__engine.host_unregister_address(addr)
                except (RuntimeError, ValueError):
                    pass
        finally:
            self.__pinned = []
            self.__engine.close()
            if self.numa:
                from ..numa import restore_affinity
                restore_affinity(self.numa)

    # -- what `BatchedObjectDetector` uses inside the worker process ----------------------------------------------------
    @property
    def num_lanes(self) -> int:
        return self.__engine.num_slots

    def bind_cameras(self, frame_buffers, camera_configs=None, drop: bool = False, logger=None):
        """Called once in the worker process.  Gives an id to every camera (key of `frame_buffers`) that needs one -- a
        configured GPU filter or a pixel format of its own; the others are -1, "no camera", so that any number of plain
        cameras fits beside the engine's 256 filter slots -- registers the GPU filters of the cameras whose (normalised)
        configuration is given -- `HipCameraFilter`, i.e. the reference's ConfidenceFilter / AreaFilter / MaskFilter
        constructors (`watsor/filter/{confidence,area,mask}.py`) -- and page-locks every `Frame.image` array
        (`watsor/stream/share.py:35-41`) so that frames travel without a host-side copy.  Returns {camera name: id}."""
        from ..filter.hip_filter import HipCameraFilter
        from .._lib import WZ_MAX_CAMS
        names = sorted(frame_buffers, key=str)
        check_ignore_cameras(self.__ignore_by_name, names)
        gate_all = self.__tiles_default is not None and "gate" in self.__tiles_default      # (a gate keeps state per camera: every camera needs an id)
        motion_all = self.__motion_default is not None                                      # (and so does the motion reference)
        need = [n for n in names if gate_all or motion_all or n in (camera_configs or {}) or str(n) in self.__fmt_by_name
                or str(n) in self.__tiles_by_name or str(n) in self.__motion_by_name]
        if len(need) > WZ_MAX_CAMS:
            raise ValueError("%d cameras with GPU filters / pixel formats of their own on one detector: the engine has %d slots"
                             % (len(need), WZ_MAX_CAMS))
        ids = {name: -1 for name in names}
        ids.update({name: i for i, name in enumerate(need)})
        self.__fmt_by_cam = {i: self.__fmt_by_name.get(str(name), self.__fmt_default) for name, i in ids.items() if i >= 0}
        self.__tiles_by_cam = {i: self.__tiles_by_name[str(name)] for name, i in ids.items() if i >= 0 and str(name) in self.__tiles_by_name}
        self.__motion_by_cam = {i: self.__motion_by_name[str(name)] for name, i in ids.items() if i >= 0 and str(name) in self.__motion_by_name}
        self.__hold_by_cam = {i: self.__hold_by_name[str(name)] for name, i in ids.items() if i >= 0 and str(name) in self.__hold_by_name}
        self.__ignore_by_cam = {i: (str(name), self.__ignore_by_name[str(name)]) for name, i in ids.items() if i >= 0 and str(name) in self.__ignore_by_name}
        for name, cfg in (camera_configs or {}).items():
            if name in ids:
                self.__filters.append(HipCameraFilter(self.__engine, ids[name], cfg, drop=drop))
        import ctypes
        arenas = {}
        for cam_name, fb in frame_buffers.items():
            for frame in fb.frames:
                obj = frame.image.get_obj() if hasattr(frame.image, "get_obj") else frame.image
                addr, size = ctypes.addressof(obj), ctypes.sizeof(obj)
                arenas.setdefault(cam_name, addr)
                try:
                    self.__engine.host_register_address(addr, size)
                    self.__pinned.append(addr)
                except (RuntimeError, ValueError) as e:      # still correct, just not DMA speed
                    if logger is not None:
                        logger.warning("frame memory at 0x%x could not be page-locked: %s" % (addr, e))
        if self.numa is not None:      # (multi-GPU hosts: where do the frames this detector will DMA from actually live?)
            from ..numa import report_arena_nodes
            self.arena_nodes = report_arena_nodes(arenas, self.numa.get("numa_node", -1), logger)
        return ids

    def bind_frame_table(self, frame_buffers, ids):
        """Called once in the worker process, after `bind_cameras`: describes every Frame of every FrameBuffer to the engine
        (`wz_bind_frames`: pixels, size, pixel format, camera id, the address of `header.detections`) -- what the reference
        worker looks up and rebuilds per payload (`watsor/detection/detector.py:104-106`, `share.py:68-73`) never changes
        after the buffers exist.  Returns {camera name: (index of its frame 0 in the table, [frame.latch.next, ...])}."""
        return self._bind_table(frame_buffers, ids, tiled=False)

    def bind_tiled_frame_table(self, frame_buffers, ids):
        """`bind_frame_table` for a detector with a `tiles` or a `motion` option (the worker's `hip_tiled_table`): after the table is bound
        every camera with a `tiles` description gets its rectangles -- `tile_grid` of the table's own width, height and format, or the
        explicit "rects" -- through `wz_bind_tiles`; a description with a "gate" on a camera that has an id sets the camera's layout
        (`set_camera_tiles`) and binds its frames gated; a gate without a camera id is tiled, not gated, as in `detect_batch`.  A camera
        with `motion` settings gets them, its hold and its ignore mask for the table's own width, height and format (`set_camera_motion`,
        `set_camera_motion_hold`, `set_camera_ignore`: its reference starts anew) and its frames a motion description (`wz_bind_motion`);
        it needs a camera id and one size and format for all its frames (ValueError).  Batches must then be cut by `plan_bound`.  Returns
        the same table."""
        return self._bind_table(frame_buffers, ids, tiled=True)

    def plan_bound(self, entries):
        """The calls `submit_bound` accepts for these table indices, in order: see the module's `plan_bound`."""
        return plan_bound(self.bound_descriptions, entries, self.bound_max_batch or self.max_batch)

    def _bind_table(self, frame_buffers, ids, tiled: bool):
        import ctypes
        pix, ws, hs, fmts, cams, rows, table = [], [], [], [], [], [], {}
        from .. import _lib
        frame_bytes = _lib.load().wz_frame_bytes              # (the library sizes a frame: one rule for the table and the engine)
        yuv = _planar_format(self.__fmt_default, self.__fmt_by_cam)
        for name in sorted(frame_buffers, key=str):
            if not tiled and (self.__tiles_default is not None or str(name) in self.__tiles_by_name):
                raise ValueError("camera %r has tiles configured: tiled detection does not go through the worker's frame table "
                                 "(bind_frame_table / submit_bound); use detect() / detect_batch() for it" % (name,))
            if not tiled and (self.__motion_default is not None or str(name) in self.__motion_by_name):
                raise ValueError("camera %r has motion configured: motion regions do not go through the untiled frame table "
                                 "(bind_frame_table); use bind_tiled_frame_table() or detect_batch() for it" % (name,))
            cam = ids.get(name, -1)
            fmt0 = self.__fmt_by_cam.get(cam, self.__fmt_default) if cam >= 0 else self.__fmt_default
            latches = []
            table[name] = (len(pix), latches)
            for frame in frame_buffers[name].frames:
                hdr = frame.header.get_obj() if hasattr(frame.header, "get_obj") else frame.header
                obj = frame.image.get_obj() if hasattr(frame.image, "get_obj") else frame.image
                w, h, fmt = int(hdr.width), int(hdr.height), fmt0
                channels = int(hdr.channels)
                if fmt == FMT_RGB24 and channels == 1:               # a planar buffer read as RGB24: the configured planar YUV format
                    fmt = yuv
                # a frame buffer's one-channel image is a 2-D array of bytes: (H*3/2, W, 1) planar, (H, 2W, 1) packed 4:2:2, (H*3/2, 2W, 1) 10-bit.
                # (A base the library does not know is held to RGB24's three channels here and refused by the library's sizing below.)
                base = fmt & FMT_BASE_MASK if fmt & FMT_BASE_MASK in _TABLE_SHAPES else FMT_RGB24
                geo = frame_shape(base, h, w, None if channels == 1 else channels, 1)
                if geo is None:
                    raise ValueError("camera %r: %s" % (name, _TABLE_SHAPES[base]))
                w, h = geo
                need = int(frame_bytes(w, h, fmt))
                if not need:
                    raise ValueError("camera %r: pixel format word 0x%x is not taken at %dx%d" % (name, fmt, w, h))
                if ctypes.sizeof(obj) < need:
                    raise ValueError("camera %r: frame memory smaller than its header says" % (name,))
                pix.append(ctypes.addressof(obj))
                ws.append(w)
                hs.append(h)
                fmts.append(fmt)
                cams.append(cam)
                rows.append(ctypes.addressof(hdr.detections))
                latches.append(frame.latch.next)
        self.__engine.bind_frames(pix, ws, hs, fmts, cams, rows)
        self.bound_descriptions = [("plain", None, None, 1, c) for c in cams]
        if tiled:
            self._bind_tiles(frame_buffers, table, ws, hs, fmts, cams)
            self._bind_motion(frame_buffers, table, ws, hs, fmts, cams)
        self.submit_bound = self.__engine.submit_bound      # (the worker calls these once per batch: no wrapper frames in between)
        self.collect_bound = self.__engine.collect_bound
        return table

    def _bind_tiles(self, frame_buffers, table, ws, hs, fmts, cams):
        """The tiled descriptions of a freshly bound table: per camera with a `tiles` option, one `bind_tiles` per run of frames that share
        their rectangles (all of them, unless a FrameBuffer holds frames of several sizes)."""
        eng = self.__engine
        for name in sorted(frame_buffers, key=str):
            base, latches = table[name]
            spec = self.__tiles_by_name.get(str(name), self.__tiles_default)
            if spec is None or not latches:
                continue
            iou = float(eng.nms_iou if spec["iou"] is None else spec["iou"])
            ios = float(1.0 if spec["ios"] is None else spec["ios"])
            cam = cams[base]
            gated = "gate" in spec and cam >= 0
            first = base
            while first < base + len(latches):
                w, h, fmt = ws[first], hs[first], fmts[first]
                rects = self._rects_of(spec, w, h, fmt)
                last = first + 1
                while last < base + len(latches) and (ws[last], hs[last], fmts[last]) == (w, h, fmt):
                    last += 1
                if gated:
                    if first != base:
                        raise ValueError("camera %r: the frames of a gated camera must share one size and format" % (name,))
                    self._set_gate_layout(cam, w, h, fmt, rects, spec["gate"])
                    eng.bind_tiles(first, last - first, None, iou, ios, gated=True)
                else:
                    eng.bind_tiles(first, last - first, rects, iou, ios)
                for i in range(first, last):
                    self.bound_descriptions[i] = ("gated" if gated else "tiled", iou, ios, len(rects), cam)
                first = last

    def _bind_motion(self, frame_buffers, table, ws, hs, fmts, cams):
        """The motion descriptions of a freshly bound table: per camera with `motion` settings, the settings, the hold and the ignore mask
        for the table's own width, height and format -- in the order `_detect_motion` sets them, and recorded as it records them: a piece
        the engine refuses is retried through `detect_batch()`, which must find the layout current and leave reference, ages and mask
        alone -- then one `bind_motion` over the camera's frames."""
        eng = self.__engine
        for name in sorted(frame_buffers, key=str):
            base, latches = table[name]
            m = self.__motion_by_name.get(str(name), self.__motion_default)
            if m is None or not latches:
                continue
            cam, last = cams[base], base + len(latches)
            if cam < 0:
                raise ValueError("camera %r: a motion camera needs a camera id: the reference is kept per camera (bind_cameras first)" % (name,))
            w, h, fmt = ws[base], hs[base], fmts[base]
            if any((ws[i], hs[i], fmts[i]) != (w, h, fmt) for i in range(base, last)):
                raise ValueError("camera %r: the frames of a motion camera must share one size and format" % (name,))
            eng.set_camera_motion(cam, w, h, m["threshold"], m["min_cells"], m["dilate"], m["max_regions"], m["min_side"], m["pad"],
                                  m["whole_frame"], fmt)
            hold = self.__hold_by_cam.get(cam) or self.__hold_default      # (new motion settings drop the hold: it is set behind them)
            if hold is not None:
                eng.set_camera_motion_hold(cam, hold["hold"], hold["object_hold"])
            self._set_ignore(cam, w, h)                                     # (... and the motion part of the mask)
            self.__motion_layouts[cam] = (w, h, fmt & FMT_BASE_MASK, id(m))
            iou = float(eng.nms_iou if m["iou"] is None else m["iou"])
            ios = float(1.0 if m["ios"] is None else m["ios"])
            eng.bind_motion(base, last - base, iou, ios)
            for i in range(base, last):
                self.bound_descriptions[i] = ("motion", iou, ios, m["count"], cam)

    def submit_host(self, lane: int, images: Sequence[np.ndarray], cameras: Optional[Sequence[int]] = None) -> None:
        """Asynchronous `detect_batch`: the frames (views of shared memory, unchanged until `collect`) are enqueued on `lane`."""
        if self.tiled:
            raise ValueError("this detector has tiles configured: the asynchronous host path (submit_host / collect) detects untiled; "
                             "use detect() / detect_batch()")
        if self.motion:
            raise ValueError("this detector has motion configured: the asynchronous host path (submit_host / collect) detects untiled; "
                             "use detect_batch()")
        self.__engine.submit_host(lane, images, cameras, self._formats(images, cameras))

    def collect(self, lane: int, detections: Sequence) -> None:
        """Waits for `lane` and writes its rows into the given `Detection[100]` arrays (the frame headers)."""
        self.__engine.collect(lane, detections)

    def _rects(self, spec: dict, frame: np.ndarray, fmt: int):
        """The rectangles of a frame under a `tiles` option (a grid is laid out once per frame size and format)."""
        if "rects" in spec:
            return spec["rects"]
        return self._rects_of(spec, *self.__engine.frame_geometry(frame, fmt), fmt)

    def _rects_of(self, spec: dict, w: int, h: int, fmt: int):
        """... of a w x h frame of format word `fmt`"""
        if "rects" in spec:
            return spec["rects"]
        key = (id(spec), w, h, fmt & FMT_BASE_MASK)
        rects = self.__tile_rects.get(key)
        if rects is None:
            cols, rows = spec["grid"]
            rects = self.__tile_rects[key] = tile_grid(w, h, cols, rows, spec["overlap"], spec["full_frame"],
                                                       even=(fmt & FMT_BASE_MASK) in YUV_FORMATS)
        return rects

    def _detect_motion(self, frames, detections, cameras, passes, formats, moving):
        """The frames `moving` = [(index, settings), ...] through `detect_motion`: frames with the same thresholds share a call while their
        cameras' configured whole_frame + max_regions fit max_batch, one frame per camera and call."""
        pick = lambda seq, idx: None if seq is None else [seq[i] for i in idx]      # noqa: E731
        # a frame without a camera id ends the list: the calls before the one it would have joined are made, then the error
        ok = list(itertools.takewhile(lambda im: cameras is not None and cameras[im[0]] >= 0, moving))
        calls = cut_calls([((m["iou"], m["ios"]), m["count"], cameras[i]) for i, m in ok], self.max_batch)
        ms = 0.0
        for n, call in enumerate(calls):
            for i, m in (ok[j] for j in call):
                fmt = formats[i] if formats is not None else FMT_RGB24
                w, h = self.__engine.frame_geometry(frames[i], fmt)
                layout = (w, h, fmt & FMT_BASE_MASK, id(m))
                if self.__motion_layouts.get(cameras[i]) != layout:      # the first frame of the camera, or another size or format
                    self.__engine.set_camera_motion(cameras[i], w, h, m["threshold"], m["min_cells"], m["dilate"], m["max_regions"], m["min_side"],
                                                    m["pad"], m["whole_frame"], fmt)
                    hold = self.__hold_by_cam.get(cameras[i]) or self.__hold_default      # (new motion settings drop the hold: it is set behind them)
                    if hold is not None:
                        self.__engine.set_camera_motion_hold(cameras[i], hold["hold"], hold["object_hold"])
                    self._set_ignore(cameras[i], w, h)      # (... and the motion part of the mask)
                    self.__motion_layouts[cameras[i]] = layout
            if len(ok) < len(moving) and n == len(calls) - 1:
                break
            idx, m = [ok[j][0] for j in call], ok[call[0]][1]
            ms += self.__engine.detect_motion(pick(frames, idx), pick(cameras, idx), pick(detections, idx), pick(passes, idx), pick(formats, idx),
                                              iou=m["iou"], ios=m["ios"])
        if len(ok) < len(moving):
            raise ValueError("motion: frame %d comes without a camera id: the reference is kept per camera (detect_batch(..., cameras=...))"
                             % moving[len(ok)][0])
        return ms

    def _detect(self, frames, detections, cameras, passes):
        formats = self._formats(frames, cameras)
        ms = 0.0
        if self.motion:      # frames of a camera with motion settings go their own way; the rest as without the option
            spec_of = lambda i: (self.__motion_by_cam.get(cameras[i]) if cameras is not None else None) or self.__motion_default      # noqa: E731
            moving = [(i, spec_of(i)) for i in range(len(frames)) if spec_of(i) is not None]
            if moving:
                ms += self._detect_motion(frames, detections, cameras, passes, formats, moving)
                rest = [i for i in range(len(frames)) if i not in {j for j, _ in moving}]
                if not rest:
                    return ms
                pick = lambda seq: None if seq is None else [seq[i] for i in rest]      # noqa: E731
                frames, detections, cameras, passes, formats = pick(frames), pick(detections), pick(cameras), pick(passes), pick(formats)
        specs = [self.__tiles_by_cam.get(cameras[i], self.__tiles_default) if cameras is not None else self.__tiles_default
                 for i in range(len(frames))]
        if not any(s is not None for s in specs):
            return ms + self.__engine.detect_batch(frames, detections, cameras, passes, formats)
        pick = lambda seq, idx: None if seq is None else [seq[i] for i in idx]      # noqa: E731
        plain = [i for i, s in enumerate(specs) if s is None]
        if plain:
            ms += self.__engine.detect_batch(pick(frames, plain), pick(detections, plain), pick(cameras, plain), pick(passes, plain),
                                             pick(formats, plain))
        # frames with the same thresholds share a call while their tiles fit max_batch (all the tiles of a call are one batch); frames of a
        # gated description that come with a camera id go through detect_gated, one frame per camera and call
        tiled = [i for i, s in enumerate(specs) if s is not None]
        fmt_of = lambda i: formats[i] if formats is not None else FMT_RGB24      # noqa: E731
        rects = {i: self._rects(specs[i], frames[i], fmt_of(i)) for i in tiled}
        gated = {i: "gate" in specs[i] and cameras is not None and cameras[i] >= 0 for i in tiled}
        items = [((specs[i]["iou"], specs[i]["ios"], gated[i]), len(rects[i]), cameras[i] if gated[i] else None) for i in tiled]
        for call in cut_calls(items, self.max_batch):
            call = [tiled[j] for j in call]
            s = specs[call[0]]
            if gated[call[0]]:
                for i in call:
                    self._gate_layout(cameras[i], frames[i], fmt_of(i), rects[i], specs[i]["gate"])
                ms += self.__engine.detect_gated(pick(frames, call), pick(cameras, call), pick(detections, call), pick(passes, call),
                                                 pick(formats, call), iou=s["iou"], ios=s["ios"])
            else:
                ms += self.__engine.detect_tiled(pick(frames, call), [rects[i] for i in call], pick(detections, call), pick(cameras, call),
                                                 pick(passes, call), pick(formats, call), iou=s["iou"], ios=s["ios"])
        return ms

    def _gate_layout(self, cam: int, frame: np.ndarray, fmt: int, rects, gate) -> None:
        """Camera `cam`'s tiles in the engine: set the first time a frame of it is seen, and again when its size, format or tiles change."""
        self._set_gate_layout(cam, *self.__engine.frame_geometry(frame, fmt), fmt, rects, gate)

    def _set_gate_layout(self, cam: int, w: int, h: int, fmt: int, rects, gate) -> None:
        layout = (w, h, fmt & FMT_BASE_MASK, tuple(rects), gate)
        if self.__gate_layouts.get(cam) != layout:
            self.__engine.set_camera_tiles(cam, w, h, rects, gate[0], gate[1], gate[2], fmt)
            self._set_ignore(cam, w, h)      # (a new layout drops the gate part of the mask: it is set behind it)
            self.__gate_layouts[cam] = layout

    def _set_ignore(self, cam: int, w: int, h: int) -> None:
        """Camera `cam`'s ignore mask in the engine, behind every (re)configuration of its motion settings or tiles."""
        named = self.__ignore_by_cam.get(cam)
        if named is not None:
            self.__engine.set_camera_ignore(cam, ignore_plane(named[1], "ignore[%r]" % (named[0],), w, h))

    def detect(self, image_shape, image_np, detections: List[Detection]):
        return self._detect([image_np.reshape(image_shape)], [detections], None, None)

    def detect_batch(self, image_shapes: Sequence, images: Sequence[np.ndarray], detections: Sequence,
                     cameras: Optional[Sequence[int]] = None, passes: Optional[Sequence[np.ndarray]] = None):
        return self._detect([im.reshape(sh) for sh, im in zip(image_shapes, images)], detections, cameras, passes)
