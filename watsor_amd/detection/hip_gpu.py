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

from ..runtime import FMT_BASE_MASK, FMT_RGB24, YUV_FORMATS, HipEngine, frame_shape, tile_grid
from ..share import Detection
from .options import _TABLE_SHAPES, CameraSettings, DetectorOptions, check_ignore_cameras, cut_calls, frame_formats, ignore_plane, plan_bound
# what tests, tools and the factory have always imported from here (the option parsing lives in options.py)
from .options import (COLOR_MATRICES, COLOR_RANGES, PIXEL_FORMATS, _planar_format, check_motion_options,      # noqa: F401
                      format_words, ignore_options, motion_hold_options, motion_options, pixel_format_code, tile_options)

ENGINE_FILE = "mi355x.bin"       # the analogue of gpu.trt (watsor/detection/detector.py:44)


def _pick(seq, idx):
    """The elements `idx` of an argument of a call that may be absent."""
    return None if seq is None else [seq[i] for i in idx]


class HipObjectDetector:
    """Performs object detection on AMD Instinct MI355X GPUs (hand-written HIP kernels)."""

    bound_max_batch = None          # the batch limit `plan_bound` cuts for (None: the engine's max_batch)

    def __init__(self, model_path, device: int = 0, options: Optional[dict] = None, max_batch: Optional[int] = None,
                 max_width: Optional[int] = None, max_height: Optional[int] = None):
        """`options` (third positional argument, what `create_object_detectors` passes in `detector_args`):
        dict(max_batch=, max_width=, max_height=) -- the factory derives the frame size from the cameras' frame buffers;
        the keyword forms and the WATSOR_HIP_MAX_* environment variables are the fallbacks.
        `options["pixel_format"]`, `["color_matrix"]`, `["color_range"]`, `["tiles"]`, `["motion"]`, `["motion_hold"]`, `["ignore"]`: what the
        cameras' frames hold and where the detector runs on them, for every camera or per camera name -- see `DetectorOptions`.
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
        self._opts = DetectorOptions(options, max_batch)
        # a `tiles` / a `motion` option is set (for every camera or for some): frames go through `detect()` / `detect_batch()` (motion:
        # `detect_batch()` with camera ids), or through a frame table bound with `bind_tiled_frame_table`
        self.tiled, self.motion = self._opts.tiled, self._opts.motion
        self._default = self._opts.default      # the settings of a frame without a camera id, or with one `bind_cameras` never saw
        self._cams = {}                         # camera id -> CameraSettings (`_adopt_ids`)
        self._tile_rects = {}
        self._layouts = {}                      # camera id -> what its tiles or its motion settings were last set for in the engine
        self.bound_descriptions = []            # per frame-table entry: (kind, iou, ios, tiles, camera id), see `plan_bound`
        self._warn_short_of_queues()
        self._engine = HipEngine(engine_path, device, max_batch, max_width, max_height, schedule=schedule)
        self._filters = []
        self._pinned = []

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
        return self._engine.schedule

    def _settings(self, cam: int) -> CameraSettings:
        return self._cams.get(cam, self._default)

    def _formats(self, frames: Sequence[np.ndarray], cameras: Optional[Sequence[int]]):
        return frame_formats(frames, cameras, self._default.fmt, {i: c.fmt for i, c in self._cams.items()})

    @property
    def engine(self) -> HipEngine:
        return self._engine

    @property
    def max_batch(self) -> int:
        return self._engine.max_batch

    @property
    def device_name(self):
        return self._engine.device_name

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        try:
            self._engine.sync()
            for addr in self._pinned:
                try:
                    self._engine.host_unregister_address(addr)
                except (RuntimeError, ValueError):
                    pass
        finally:
            self._pinned = []
            self._engine.close()
            if self.numa:
                from ..numa import restore_affinity
                restore_affinity(self.numa)

    # -- what `BatchedObjectDetector` uses inside the worker process ----------------------------------------------------
    @property
    def num_lanes(self) -> int:
        return self._engine.num_slots

    def bind_cameras(self, frame_buffers, camera_configs=None, drop: bool = False, logger=None):
        """Called once in the worker process.  Gives an id to every camera (key of `frame_buffers`) that needs one -- a
        configured GPU filter or a pixel format of its own; the others are -1, "no camera", so that any number of plain
        cameras fits beside the engine's 256 filter slots -- registers the GPU filters of the cameras whose (normalised)
        configuration is given -- `HipCameraFilter`, i.e. the reference's ConfidenceFilter / AreaFilter / MaskFilter
        constructors (`watsor/filter/{confidence,area,mask}.py`) -- and page-locks every `Frame.image` array
        (`watsor/stream/share.py:35-41`) so that frames travel without a host-side copy.  Returns {camera name: id}."""
        from ..filter.hip_filter import HipCameraFilter
        ids = self._assign_ids(sorted(frame_buffers, key=str), camera_configs or {})
        for name, cfg in (camera_configs or {}).items():
            if name in ids:
                self._filters.append(HipCameraFilter(self._engine, ids[name], cfg, drop=drop))
        import ctypes
        arenas = {}
        for cam_name, fb in frame_buffers.items():
            for frame in fb.frames:
                obj = frame.image.get_obj() if hasattr(frame.image, "get_obj") else frame.image
                addr, size = ctypes.addressof(obj), ctypes.sizeof(obj)
                arenas.setdefault(cam_name, addr)
                try:
                    self._engine.host_register_address(addr, size)
                    self._pinned.append(addr)
                except (RuntimeError, ValueError) as e:      # still correct, just not DMA speed
                    if logger is not None:
                        logger.warning("frame memory at 0x%x could not be page-locked: %s" % (addr, e))
        if self.numa is not None:      # (multi-GPU hosts: where do the frames this detector will DMA from actually live?)
            from ..numa import report_arena_nodes
            self.arena_nodes = report_arena_nodes(arenas, self.numa.get("numa_node", -1), logger)
        return ids

    def _assign_ids(self, names, camera_configs):
        """{camera name: id} for the detector's cameras `names`: 0, 1, ... in their order for those that need one of the engine's slots
        (`DetectorOptions.needs_id`), -1 for the others; the ids are adopted.  A pure function of the options but for that."""
        from .._lib import WZ_MAX_CAMS
        check_ignore_cameras(self._opts.ignore, names)
        need = [n for n in names if self._opts.needs_id(n, n in camera_configs)]
        if len(need) > WZ_MAX_CAMS:
            raise ValueError("%d cameras with GPU filters / pixel formats of their own on one detector: the engine has %d slots"
                             % (len(need), WZ_MAX_CAMS))
        ids = {name: -1 for name in names}
        ids.update({name: i for i, name in enumerate(need)})
        self._adopt_ids(ids)
        return ids

    def _adopt_ids(self, ids) -> None:
        """Takes {camera name: id} as the detector's cameras: a frame that comes with an id >= 0 gets that camera's settings from here
        on.  `bind_cameras` ends its id assignment with this; a caller that assigns ids itself calls it in its place."""
        self._cams = {i: self._opts.for_name(name) for name, i in ids.items() if i >= 0}

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
        yuv = self._opts.planar_format(self._cams.values())
        for name in sorted(frame_buffers, key=str):
            named = self._opts.for_name(name)
            if not tiled and named.tiles is not None:
                raise ValueError("camera %r has tiles configured: tiled detection does not go through the worker's frame table "
                                 "(bind_frame_table / submit_bound); use detect() / detect_batch() for it" % (name,))
            if not tiled and named.motion is not None:
                raise ValueError("camera %r has motion configured: motion regions do not go through the untiled frame table "
                                 "(bind_frame_table); use bind_tiled_frame_table() or detect_batch() for it" % (name,))
            cam = ids.get(name, -1)
            fmt0 = self._settings(cam).fmt
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
        self._engine.bind_frames(pix, ws, hs, fmts, cams, rows)
        self.bound_descriptions = [("plain", None, None, 1, c) for c in cams]
        if tiled:
            layout = list(zip(ws, hs, fmts))
            self._bind_tiles(table, layout, cams)
            self._bind_motion(table, layout, cams)
        self.submit_bound = self._engine.submit_bound      # (the worker calls these once per batch: no wrapper frames in between)
        self.collect_bound = self._engine.collect_bound
        return table

    def _table_cameras(self, table, layout, cams, option: str):
        """The cameras of a freshly bound table that have frames in it and an `option` ("tiles" | "motion"), by name: (name, its checked
        description, index of its first entry, its camera id, [(first, last, w, h, fmt), ...] -- its entries as runs of frames that share
        size and format: one, unless a FrameBuffer holds frames of several)."""
        for name in sorted(table, key=str):
            (base, latches), spec = table[name], getattr(self._opts.for_name(name), option)
            if spec is None or not latches:
                continue
            runs, first = [], base
            for key, run in itertools.groupby(layout[base:base + len(latches)]):
                runs.append((first, first + len(list(run))) + key)
                first = runs[-1][1]
            yield name, spec, base, cams[base], runs

    def _bound_thresholds(self, spec: dict):
        """(iou, ios) of a `tiles` / `motion` description as a table entry holds them: the engine's defaults written out."""
        return float(self._engine.nms_iou if spec["iou"] is None else spec["iou"]), float(1.0 if spec["ios"] is None else spec["ios"])

    def _bind_tiles(self, table, layout, cams):
        """The tiled descriptions of a freshly bound table: per camera with a `tiles` option, one `bind_tiles` per run of frames that share
        their rectangles (all of them, unless a FrameBuffer holds frames of several sizes)."""
        for name, spec, base, cam, runs in self._table_cameras(table, layout, cams, "tiles"):
            iou, ios = self._bound_thresholds(spec)
            gated = "gate" in spec and cam >= 0
            for first, last, w, h, fmt in runs:
                rects = self._rects_of(spec, w, h, fmt)
                if gated:
                    if first != base:
                        raise ValueError("camera %r: the frames of a gated camera must share one size and format" % (name,))
                    self._set_gate_layout(cam, w, h, fmt, rects, spec["gate"])
                    self._engine.bind_tiles(first, last - first, None, iou, ios, gated=True)
                else:
                    self._engine.bind_tiles(first, last - first, rects, iou, ios)
                self.bound_descriptions[first:last] = [("gated" if gated else "tiled", iou, ios, len(rects), cam)] * (last - first)

    def _bind_motion(self, table, layout, cams):
        """The motion descriptions of a freshly bound table: per camera with `motion` settings, the settings for the table's own width,
        height and format -- set anew on every bind: the camera's reference starts with the table -- then one `bind_motion` over the
        camera's frames."""
        for name, m, base, cam, runs in self._table_cameras(table, layout, cams, "motion"):
            if cam < 0:
                raise ValueError("camera %r: a motion camera needs a camera id: the reference is kept per camera (bind_cameras first)" % (name,))
            if len(runs) > 1:
                raise ValueError("camera %r: the frames of a motion camera must share one size and format" % (name,))
            first, last, w, h, fmt = runs[0]
            self._set_motion_layout(cam, w, h, fmt, m, force=True)
            iou, ios = self._bound_thresholds(m)
            self._engine.bind_motion(first, last - first, iou, ios)
            self.bound_descriptions[first:last] = [("motion", iou, ios, m["count"], cam)] * (last - first)

    def submit_host(self, lane: int, images: Sequence[np.ndarray], cameras: Optional[Sequence[int]] = None) -> None:
        """Asynchronous `detect_batch`: the frames (views of shared memory, unchanged until `collect`) are enqueued on `lane`."""
        if self.tiled:
            raise ValueError("this detector has tiles configured: the asynchronous host path (submit_host / collect) detects untiled; "
                             "use detect() / detect_batch()")
        if self.motion:
            raise ValueError("this detector has motion configured: the asynchronous host path (submit_host / collect) detects untiled; "
                             "use detect_batch()")
        self._engine.submit_host(lane, images, cameras, self._formats(images, cameras))

    def collect(self, lane: int, detections: Sequence) -> None:
        """Waits for `lane` and writes its rows into the given `Detection[100]` arrays (the frame headers)."""
        self._engine.collect(lane, detections)

    def _rects(self, spec: dict, frame: np.ndarray, fmt: int):
        """The rectangles of a frame under a `tiles` option (a grid is laid out once per frame size and format)."""
        if "rects" in spec:
            return spec["rects"]
        return self._rects_of(spec, *self._engine.frame_geometry(frame, fmt), fmt)

    def _rects_of(self, spec: dict, w: int, h: int, fmt: int):
        """... of a w x h frame of format word `fmt`"""
        if "rects" in spec:
            return spec["rects"]
        key = (id(spec), w, h, fmt & FMT_BASE_MASK)
        rects = self._tile_rects.get(key)
        if rects is None:
            cols, rows = spec["grid"]
            rects = self._tile_rects[key] = tile_grid(w, h, cols, rows, spec["overlap"], spec["full_frame"],
                                                      even=(fmt & FMT_BASE_MASK) in YUV_FORMATS)
        return rects

    def _detect_motion(self, frames, detections, cameras, passes, formats, moving):
        """The frames `moving` = [(index, settings), ...] through `detect_motion`: frames with the same thresholds share a call while their
        cameras' configured whole_frame + max_regions fit max_batch, one frame per camera and call."""
        # a frame without a camera id ends the list: the calls before the one it would have joined are made, then the error
        ok = list(itertools.takewhile(lambda im: cameras is not None and cameras[im[0]] >= 0, moving))
        calls = cut_calls([((m["iou"], m["ios"]), m["count"], cameras[i]) for i, m in ok], self.max_batch)
        ms = 0.0
        for n, call in enumerate(calls):
            for i, m in (ok[j] for j in call):
                fmt = formats[i] if formats is not None else FMT_RGB24
                self._set_motion_layout(cameras[i], *self._engine.frame_geometry(frames[i], fmt), fmt, m)
            if len(ok) < len(moving) and n == len(calls) - 1:
                break
            idx, m = [ok[j][0] for j in call], ok[call[0]][1]
            ms += self._engine.detect_motion(_pick(frames, idx), _pick(cameras, idx), _pick(detections, idx), _pick(passes, idx),
                                             _pick(formats, idx), iou=m["iou"], ios=m["ios"])
        if len(ok) < len(moving):
            raise ValueError("motion: frame %d comes without a camera id: the reference is kept per camera (detect_batch(..., cameras=...))"
                             % moving[len(ok)][0])
        return ms

    def _detect(self, frames, detections, cameras, passes):
        formats = self._formats(frames, cameras)
        if not (self.tiled or self.motion):
            return self._engine.detect_batch(frames, detections, cameras, passes, formats)
        settings = [self._default] * len(frames) if cameras is None else [self._settings(c) for c in cameras]
        # frames of a camera with motion settings go their own way; the rest as without the option: untiled ones in one call, then the tiled
        moving = [(i, s.motion) for i, s in enumerate(settings) if s.motion is not None]
        ms = self._detect_motion(frames, detections, cameras, passes, formats, moving) if moving else 0.0
        specs = {i: s.tiles for i, s in enumerate(settings) if s.motion is None}
        plain = [i for i, spec in specs.items() if spec is None]
        if plain or not frames:      # (an empty batch is the engine's to answer)
            ms += self._engine.detect_batch(_pick(frames, plain), _pick(detections, plain), _pick(cameras, plain), _pick(passes, plain),
                                            _pick(formats, plain))
        # frames with the same thresholds share a call while their tiles fit max_batch (all the tiles of a call are one batch); frames of a
        # gated description that come with a camera id go through detect_gated, one frame per camera and call
        tiled = [i for i, spec in specs.items() if spec is not None]
        fmt_of = lambda i: formats[i] if formats is not None else FMT_RGB24      # noqa: E731
        rects = {i: self._rects(specs[i], frames[i], fmt_of(i)) for i in tiled}
        gated = {i: "gate" in specs[i] and cameras is not None and cameras[i] >= 0 for i in tiled}
        items = [((specs[i]["iou"], specs[i]["ios"], gated[i]), len(rects[i]), cameras[i] if gated[i] else None) for i in tiled]
        for call in cut_calls(items, self.max_batch):
            call = [tiled[j] for j in call]
            s = specs[call[0]]
            if gated[call[0]]:
                for i in call:
                    self._set_gate_layout(cameras[i], *self._engine.frame_geometry(frames[i], fmt_of(i)), fmt_of(i), rects[i], specs[i]["gate"])
                ms += self._engine.detect_gated(_pick(frames, call), _pick(cameras, call), _pick(detections, call), _pick(passes, call),
                                                _pick(formats, call), iou=s["iou"], ios=s["ios"])
            else:
                ms += self._engine.detect_tiled(_pick(frames, call), [rects[i] for i in call], _pick(detections, call), _pick(cameras, call),
                                                _pick(passes, call), _pick(formats, call), iou=s["iou"], ios=s["ios"])
        return ms

    def _set_gate_layout(self, cam: int, w: int, h: int, fmt: int, rects, gate) -> None:
        """Camera `cam`'s tiles in the engine: set the first time a frame of it is seen, and again when its size, format or tiles change."""
        layout = (w, h, fmt & FMT_BASE_MASK, tuple(rects), gate)
        if self._layouts.get(cam) != layout:
            self._engine.set_camera_tiles(cam, w, h, rects, gate[0], gate[1], gate[2], fmt)
            self._set_ignore(cam, w, h)      # (a new layout drops the gate part of the mask: it is set behind it)
            self._layouts[cam] = layout

    def _set_motion_layout(self, cam: int, w: int, h: int, fmt: int, m: dict, force: bool = False) -> None:
        """Camera `cam`'s motion settings in the engine, the twin of `_set_gate_layout`: set the first time a frame of it is seen, again
        when its size, format or settings change, and whenever a frame table binds it (`force`).  Settings, hold, mask, in this order,
        then the layout is recorded: a bound piece the engine refuses is retried through `detect_batch()`, which must find the layout
        current and leave the camera's reference, ages and mask alone."""
        layout = (w, h, fmt & FMT_BASE_MASK, id(m))
        if force or self._layouts.get(cam) != layout:
            self._engine.set_camera_motion(cam, w, h, m["threshold"], m["min_cells"], m["dilate"], m["max_regions"], m["min_side"], m["pad"],
                                           m["whole_frame"], fmt)
            hold = self._settings(cam).hold      # (new motion settings drop the hold: it is set behind them)
            if hold is not None:
                self._engine.set_camera_motion_hold(cam, hold["hold"], hold["object_hold"])
            self._set_ignore(cam, w, h)          # (... and the motion part of the mask)
            self._layouts[cam] = layout

    def _set_ignore(self, cam: int, w: int, h: int) -> None:
        """Camera `cam`'s ignore mask in the engine, behind every (re)configuration of its motion settings or tiles."""
        named = self._settings(cam)
        if named.ignore is not None:
            self._engine.set_camera_ignore(cam, ignore_plane(named.ignore, "ignore[%r]" % (named.name,), w, h))

    def detect(self, image_shape, image_np, detections: List[Detection]):
        return self._detect([image_np.reshape(image_shape)], [detections], None, None)

    def detect_batch(self, image_shapes: Sequence, images: Sequence[np.ndarray], detections: Sequence,
                     cameras: Optional[Sequence[int]] = None, passes: Optional[Sequence[np.ndarray]] = None):
        return self._detect([im.reshape(sh) for sh, im in zip(image_shapes, images)], detections, cameras, passes)
