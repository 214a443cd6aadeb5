"""The detector plugin's options, the part that needs no engine: what `HipObjectDetector` (hip_gpu.py) is configured with -- pixel formats,
tiles, motion, motion hold, ignore masks -- parsed and cross-checked once (`DetectorOptions`) and resolved per camera (`CameraSettings`),
and the pure rules that cut frames into engine calls (`cut_calls`, `plan_bound`).  Nothing here loads the library or touches a GPU."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Sequence

import numpy as np

from ..runtime import (CSP_BT709, FMT_BASE_MASK, FMT_BGR24, FMT_GRAY8, FMT_I420, FMT_NV12, FMT_P010, FMT_RGB24, FMT_UYVY422, FMT_YUV420P10,
                       FMT_YUYV422, RANGE_FULL, TEN_BIT_FORMATS, YUV_FORMATS)
from .._lib import WZ_MAX_TILES, WZ_MOTION_MAX_REGIONS

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


def _option_code(option: str, table: dict, name) -> int:
    try:
        return table[str(name).lower()]
    except KeyError:
        raise ValueError("%s %r: expected one of %s" % (option, name, ", ".join(sorted(table)))) from None


def pixel_format_code(name) -> int:
    return _option_code("pixel_format", PIXEL_FORMATS, name)


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


# ---- the rules every description shares -------------------------------------------------------------------------------------------------
def _whole(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _merge_thresholds(spec: dict, where: str) -> dict:
    """{"iou": ..., "ios": ...} of a `tiles` or `motion` description: None (the engine's default) or a number >= 0."""
    out = {"iou": spec.get("iou"), "ios": spec.get("ios")}
    for k, v in out.items():
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0):
            raise ValueError("%s: %s %r, expected a number >= 0" % (where, k, v))
    return out


def _whole_in(where: str, k: str, v, low: int, high: Optional[int]) -> int:
    """v, a whole number with low <= v (<= high, unless None), or ValueError."""
    if not _whole(v):
        raise ValueError("%s: %s %r, expected a whole number" % (where, k, v))
    if v < low or (high is not None and v > high):
        raise ValueError("%s: %s %r, expected %s" % (where, k, v, ">= %d" % low if high is None else "%d .. %d" % (low, high)))
    return v


def _per_camera(option: str, v, single, check, expected: str, dicts_only: bool = True):
    """(the detector's description or None, {camera name: description}) of an option that is one description for every camera --
    `single(v)` says so -- or {camera name: description}; `check(description, where)` checks one."""
    if v is None:
        return None, {}
    if isinstance(v, dict) and single(v):
        return check(v, option), {}
    if not isinstance(v, dict) or not v or (dicts_only and not all(isinstance(d, dict) for d in v.values())):
        raise ValueError("%s: expected %s, got %r" % (option, expected, v))
    return None, {str(name): check(d, "%s[%r]" % (option, name)) for name, d in v.items()}


def _check_counts(option: str, default, by_name: dict, max_batch: int, what: str = "") -> None:
    """The tiles a description makes of one frame are one batch: they must fit max_batch."""
    for where, spec in [(option, default)] + [("%s[%r]" % (option, n), s) for n, s in by_name.items()]:
        if spec is not None and spec["count"] > max_batch:
            raise ValueError("%s: %s%d tiles per frame exceed max_batch %d" % (where, what, spec["count"], max_batch))


# ---- tiles ------------------------------------------------------------------------------------------------------------------------------
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
    out = _merge_thresholds(spec, where)
    if "grid" in spec:
        g = spec["grid"]
        if not isinstance(g, (list, tuple)) or len(g) != 2 or not all(_whole(v) and v >= 1 for v in g):
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
                isinstance(t, (list, tuple)) and len(t) == 4 and all(_whole(v) for v in t) and t[0] >= 0 and t[1] >= 0 and t[2] >= 1 and t[3] >= 1
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
        if not all(_whole(v) for v in gate):
            raise ValueError("%s: gate %r, expected whole numbers" % (where, g))
        for k, v, (low, high) in zip(("threshold", "min_cells", "max_age"), gate, ((0, 255), (1, None), (0, None))):
            _whole_in(where + ": gate", k, v, low, high)
        out["gate"] = gate
    return out


def tile_options(options: dict):
    """(the detector's tiles or None, {camera name: tiles}) from the plugin option `tiles`: one description (see `_tile_spec`) for
    every camera, or {camera name: description}.  Bad options raise ValueError."""
    return _per_camera("tiles", options.get("tiles"), lambda v: "grid" in v or "rects" in v, _tile_spec,
                       "a description of the tiles or {camera name: description}", dicts_only=False)


# ---- motion -----------------------------------------------------------------------------------------------------------------------------
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
    out = _merge_thresholds(spec, where)
    for k, (default, low, high) in _MOTION_RANGES.items():
        out[k] = _whole_in(where, k, spec.get(k, default), low, high)
    whole = spec.get("whole_frame", True)
    if not isinstance(whole, bool):
        raise ValueError("%s: whole_frame %r, expected true or false" % (where, whole))
    out.update(whole_frame=whole, count=(1 if whole else 0) + out["max_regions"])
    return out


def motion_options(options: dict):
    """(the detector's motion settings or None, {camera name: settings}) from the plugin option `motion`: one description (see
    `_motion_spec`) for every camera, or {camera name: description}.  Bad options raise ValueError."""
    return _per_camera("motion", options.get("motion"), lambda v: "threshold" in v, _motion_spec,
                       "a description of the motion settings or {camera name: description}")


def check_motion_options(motion_default, motion_by_name: dict, tiles_default, tiles_by_name: dict, max_batch: int) -> None:
    """What `motion_options` cannot see on its own: the settings' whole_frame + max_regions must fit max_batch, and a camera takes `motion`
    or `tiles`, not both.  Raises ValueError; the message begins with the option at fault."""
    _check_counts("motion", motion_default, motion_by_name, max_batch, "whole_frame + max_regions = ")
    if motion_default is not None and (tiles_default is not None or tiles_by_name):
        raise ValueError("motion: set for every camera together with tiles: a camera takes one of the two")
    if tiles_default is not None and motion_by_name:
        raise ValueError("motion[%r]: tiles are set for every camera: a camera takes one of the two" % (sorted(motion_by_name)[0],))
    both = sorted(set(motion_by_name) & set(tiles_by_name))
    if both:
        raise ValueError("motion[%r]: the camera has tiles too: a camera takes one of the two" % (both[0],))


# ---- motion_hold ------------------------------------------------------------------------------------------------------------------------
_MOTION_HOLD_KEYS = ("hold", "object_hold")


def _motion_hold_spec(spec, where: str) -> dict:
    """One checked `motion_hold` option: {"hold": 0 .. 255 (default 0), "object_hold": 0 .. 255 (0)}, not both 0."""
    if not isinstance(spec, dict):
        raise ValueError("%s: expected {\"hold\": 0 .. 255, \"object_hold\": 0 .. 255}, got %r" % (where, spec))
    if set(spec) - set(_MOTION_HOLD_KEYS):
        raise ValueError("%s: unknown key(s) %s" % (where, ", ".join(sorted(map(str, set(spec) - set(_MOTION_HOLD_KEYS))))))
    out = {k: _whole_in(where, k, spec.get(k, 0), 0, 255) for k in _MOTION_HOLD_KEYS}
    if not any(out.values()):
        raise ValueError("%s: hold and object_hold are both 0: leave the option out for a camera without a hold" % where)
    return out


def motion_hold_options(options: dict, motion_default, motion_by_name: dict):
    """(the detector's hold or None, {camera name: hold}) from the plugin option `motion_hold`: {"hold": 0 .. 255, "object_hold": 0 .. 255}
    for every camera with motion settings, or {camera name: such a description} -- a motion camera keeps a cell in its regions for `hold`
    further frames after it changed, and for `object_hold` further frames after a detection that passed the camera's filters covered it
    (`HipEngine.set_camera_motion_hold`).  motion_default, motion_by_name: what `motion_options` returned -- a hold needs motion settings.
    Bad options raise ValueError; the message begins with the option at fault."""
    default, by_name = _per_camera("motion_hold", options.get("motion_hold"), lambda v: v and not any(isinstance(d, dict) for d in v.values()),
                                   _motion_hold_spec, "{\"hold\": 0 .. 255, \"object_hold\": 0 .. 255} or {camera name: such a description}")
    if default is not None and motion_default is None and not motion_by_name:
        raise ValueError("motion_hold: there is no motion option: a hold keeps motion regions alive")
    for name in by_name:
        if motion_default is None and name not in motion_by_name:
            raise ValueError("motion_hold[%r]: the camera has no motion option: a hold keeps motion regions alive" % (name,))
    return default, by_name


# ---- ignore -----------------------------------------------------------------------------------------------------------------------------
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
    rects = []
    for r in spec:
        if not isinstance(r, (list, tuple)) or len(r) != 4 or not all(_whole(v) for v in r) or r[0] < 0 or r[1] < 0 or r[2] < 1 or r[3] < 1:
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


# ---- one record per camera --------------------------------------------------------------------------------------------------------------
class CameraSettings(NamedTuple):
    """What one camera is configured with: `name` (None: the detector-wide settings, of a frame without a camera id), its format word
    `fmt`, and its checked `tiles`, `motion`, `hold` and `ignore` descriptions, None where it has none."""
    name: Optional[str]
    fmt: int
    tiles: Optional[dict]
    motion: Optional[dict]
    hold: Optional[dict]
    ignore: Optional[tuple]


class DetectorOptions:
    """The per-camera options of `HipObjectDetector`, parsed and cross-checked once for a detector of `max_batch` frames a call; the
    first fault raises ValueError, its message beginning with the option at fault.
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
    per-camera option -- takes effect for the ids `bind_cameras` hands out."""

    def __init__(self, options: dict, max_batch: int):
        fmt, self._fmt = format_words(options)
        tiles, self._tiles = tile_options(options)
        motion, self._motion = motion_options(options)
        hold, self._hold = motion_hold_options(options, motion, self._motion)
        self.ignore = ignore_options(options, motion, self._motion, tiles, self._tiles)      # {camera name: description}, for `check_ignore_cameras`
        _check_counts("tiles", tiles, self._tiles, max_batch)
        check_motion_options(motion, self._motion, tiles, self._tiles, max_batch)
        self.default = CameraSettings(None, fmt, tiles, motion, hold, None)      # what a frame without a camera id gets
        self.tiled = tiles is not None or bool(self._tiles)                      # a `tiles` option is set, for every camera or for some
        self.motion = motion is not None or bool(self._motion)                   # ... a `motion` option

    def for_name(self, name) -> CameraSettings:
        """Camera `name`'s settings: its own where the option names it, else the detector-wide ones; `ignore` is per name only."""
        n, d = str(name), self.default
        return CameraSettings(n, self._fmt.get(n, d.fmt), self._tiles.get(n, d.tiles), self._motion.get(n, d.motion),
                              self._hold.get(n) or d.hold, self.ignore.get(n))

    def needs_id(self, name, configured: bool) -> bool:
        """Whether camera `name` needs one of the engine's camera slots: GPU filters (`configured`), a pixel format, tiles or motion
        settings of its own -- or any camera under a detector-wide gate or motion option, which keep state per camera."""
        n, d = str(name), self.default
        return (d.tiles is not None and "gate" in d.tiles) or d.motion is not None or configured or n in self._fmt or n in self._tiles \
            or n in self._motion

    def planar_format(self, cameras=()) -> int:
        """`_planar_format` of the detector-wide format and of the cameras' `cameras` (their `CameraSettings`, in id order)."""
        return _planar_format(self.default.fmt, {i: c.fmt for i, c in enumerate(cameras)})


# ---- cutting frames into calls ----------------------------------------------------------------------------------------------------------
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
