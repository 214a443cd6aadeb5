"""The engine calls of the detector plugin (watsor_amd/detection/hip_gpu.py), recorded on the CPU: a stand-in for `HipEngine` that logs
every call under a real `HipObjectDetector`, ctypes stand-ins for the worker's frame buffers, and the scenarios that
tests/golden/make_detector_calls_golden.py records and tests/test_detector_calls_cpu.py replays against tests/golden/detector_calls.json.
All frames are 64x48 (NV12: a 64x72 one-channel buffer) -- the smallest that still give a 2x1 grid, a 16x16 ignore rectangle and a 4x3
cell grid -- except where a scenario is about a second size (32x48)."""
import ctypes
import json
import os
import tempfile

import numpy as np

from watsor_amd.runtime import HipEngine
from watsor_amd.share import DetectionArray

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detector_calls.json")
W, H = 64, 48


# ---- frame buffers ----------------------------------------------------------------------------------------------------------------------
class _Frame:
    """What `bind_frame_table` reads of a reference Frame (watsor/stream/share.py:27-73): header, image, latch."""
    def __init__(self, w, h, channels, nbytes):
        class Header(ctypes.Structure):
            _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("channels", ctypes.c_int), ("detections", DetectionArray)]
        self.header = Header(w, h, channels)
        self.image = (ctypes.c_uint8 * nbytes)()
        self.latch = type("Latch", (), {"next": staticmethod(lambda: None)})()


def fb(*frames):
    """A FrameBuffer stand-in: `.frames`."""
    return type("FrameBuffer", (), {"frames": list(frames)})()


def rgb_buffer(n=1, w=W, h=H):
    return fb(*[_Frame(w, h, 3, w * h * 3) for _ in range(n)])


def nv12_buffer(n=1, w=W, h=H):
    return fb(*[_Frame(w, h * 3 // 2, 1, w * h * 3 // 2) for _ in range(n)])


def rgb(k, w=W, h=H):
    """An RGB24 frame whose sum tells it from the others of its call."""
    return np.full((h, w, 3), k, np.uint8)


def nv12(k, w=W, h=H):
    return np.full((h * 3 // 2, w), k, np.uint8)


def rows(n):
    return [DetectionArray() for _ in range(n)]


# ---- the stand-in engine ----------------------------------------------------------------------------------------------------------------
# positional arguments that are addresses (or lists of them): logged as their index among the addresses the engine has seen
_ADDRESSES = {"host_register_address": (0,), "host_unregister_address": (0,), "bind_frames": (0, 5)}
_RECORDED = ("close", "sync", "detect_batch", "detect_tiled", "detect_gated", "detect_motion", "set_camera_tiles", "set_camera_motion",
             "set_camera_motion_hold", "set_camera_ignore", "set_camera_filter", "set_camera_drop", "clear_camera_filter", "submit_host",
             "collect", "host_register_address", "host_unregister_address", "bind_frames", "bind_tiles", "bind_motion", "submit_bound",
             "collect_bound")


def plain_data(v, rows=None):
    """An argument as plain data: an array as (shape, dtype, sum), an output row object as its position in `rows`."""
    if isinstance(v, np.ndarray):
        total = float(np.nansum(v)) if v.dtype.kind == "f" else int(v.sum(dtype=np.int64))      # (a filter's thresholds: NaN = none)
        return ["array", list(v.shape), str(v.dtype), total]
    if isinstance(v, ctypes.Array):
        return ["rows", (rows or {}).get(id(v), -1)]
    if isinstance(v, (list, tuple)):
        return [plain_data(x, rows) for x in v]
    if isinstance(v, dict):
        return {str(k): plain_data(x, rows) for k, x in v.items()}
    if isinstance(v, (bool, str)) or v is None:
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    raise TypeError("an argument the log has no form for: %r" % (v,))


class RecordingEngine:
    """Stands where `HipEngine` stands in hip_gpu.py: the attributes the plugin reads, the real static `frame_geometry`, and every other
    method appends (name, args, kwargs) to `log` and returns 0.0."""
    nms_iou = 0.6
    num_slots = 4
    device_name = "stand-in"
    frame_geometry = staticmethod(HipEngine.frame_geometry)

    def __init__(self, engine_path, device=0, max_batch=8, max_width=1920, max_height=1080, schedule=None):
        self.max_batch = max_batch
        self.schedule = schedule or "throughput"
        self.created = [os.path.basename(engine_path), device, max_batch, max_width, max_height, schedule]
        self.log = []
        self.addresses = {}
        self.rows = {}          # id(output row object) -> its position in the plugin call under way (`Recorder.step` sets it)

    def _address(self, v):
        if isinstance(v, (list, tuple)):
            return [self._address(x) for x in v]
        return ["address", self.addresses.setdefault(int(v), len(self.addresses))]

    def _record(self, name, args, kwargs):
        where = _ADDRESSES.get(name, ())
        self.log.append([name, [self._address(a) if i in where else plain_data(a, self.rows) for i, a in enumerate(args)], plain_data(kwargs, self.rows)])
        return 0.0


def _recorded(name):
    def method(self, *args, **kwargs):
        return self._record(name, args, kwargs)
    method.__name__ = name
    return method


for _name in _RECORDED:
    setattr(RecordingEngine, _name, _recorded(_name))


# ---- recording a scenario ---------------------------------------------------------------------------------------------------------------
class Recorder:
    """Runs the steps of one scenario and keeps, per step, plain data only: the engine calls it made, what it returned, the detector's
    `bound_descriptions` behind it, and the type and text of an exception."""
    def __init__(self, hip_gpu, model_dir):
        self.hip_gpu, self.model_dir, self.steps = hip_gpu, model_dir, []

    def make(self, label, options, **kw):
        """The step that constructs a detector (None when the constructor raises)."""
        return self.step(label, None, lambda: self.hip_gpu.HipObjectDetector(self.model_dir, 0, dict(options, numa=False), **kw), keep=True)

    def step(self, label, det, call, outputs=(), keep=False):
        engine = det.engine if det is not None else None
        if engine is not None:
            engine.rows = {id(r): i for i, r in enumerate(outputs)}
        before = len(engine.log) if engine is not None else 0
        entry = {"step": label, "returned": None, "error": None}
        got = None
        try:
            got = call()
            if keep:
                det, engine = got, got.engine
                entry["returned"] = {"engine": engine.created, "tiled": det.tiled, "motion": det.motion, "schedule": det.schedule,
                                     "max_batch": det.max_batch}
            else:
                entry["returned"] = self._returned(got)
        except Exception as e:      # noqa: BLE001 -- the type and the text are what is recorded
            entry["error"] = [type(e).__name__, str(e)]
        entry["calls"] = list(engine.log[before:]) if engine is not None else []
        entry["bound_descriptions"] = plain_data(det.bound_descriptions) if det is not None else None
        self.steps.append(entry)
        return got

    @staticmethod
    def _returned(v):
        if isinstance(v, dict):      # {camera name: id}, or the frame table {camera name: (first index, latches)}
            return {str(k): [x[0], len(x[1])] if isinstance(x, tuple) else x for k, x in v.items()}
        return v


def batch(r, det, label, frames, cameras=None, passes=None):
    out = rows(len(frames))
    return r.step(label, det, lambda: det.detect_batch([f.shape for f in frames], frames, out, cameras, passes), outputs=out)


def _gate(threshold=8, **kw):
    return dict({"threshold": threshold}, **kw)


def mixed(r):
    """A: per-camera options -- motion + motion_hold + ignore + nv12 on `yard` (two frames in its buffer), a gated 2x1 grid + ignore on
    `door`, rects on `side`, nothing on `plain`; the cameras and the tiled frame table are bound, then one frame per camera is detected
    synchronously, as the worker's retry of a refused piece does: that call must set no camera again."""
    mask = np.zeros((H, W), np.uint8)
    mask[0:16, 48:64] = 1
    det = r.make("create", {
        "pixel_format": {"yard": "nv12"},
        "motion": {"yard": {"threshold": 12, "max_regions": 2, "min_side": 16}},
        "motion_hold": {"yard": {"hold": 3, "object_hold": 5}},
        "ignore": {"yard": mask, "door": [[0, 0, 16, 16]]},
        "tiles": {"door": {"grid": [2, 1], "gate": _gate(8, max_age=4)}, "side": {"rects": [[0, 0, 32, 48], [32, 0, 32, 48]], "iou": 0.5}}})
    buffers = {"yard": nv12_buffer(2), "door": rgb_buffer(), "side": rgb_buffer(), "plain": rgb_buffer()}
    ids = r.step("bind_cameras", det, lambda: det.bind_cameras(buffers))
    r.step("bind_tiled_frame_table", det, lambda: det.bind_tiled_frame_table(buffers, ids))
    names = ["door", "plain", "side", "yard"]
    frames = [rgb(1), rgb(2), rgb(3), nv12(4)]
    batch(r, det, "detect_batch after the bind", frames, [ids[n] for n in names], [np.full(100, i + 1, np.uint8) for i in range(4)])
    r.step("exit", det, lambda: det.__exit__(None, None, None))


def wide_gate(r):
    """B1: a gated `tiles` for every camera -- frames without ids are tiled, not gated; with ids they are gated."""
    det = r.make("create", {"tiles": {"grid": [2, 1], "gate": _gate(8)}})
    buffers = {"a": rgb_buffer(), "b": rgb_buffer()}
    ids = r.step("bind_cameras", det, lambda: det.bind_cameras(buffers))
    batch(r, det, "detect_batch without ids", [rgb(1), rgb(2)])
    batch(r, det, "detect_batch with ids", [rgb(1), rgb(2)], [ids["a"], ids["b"]])


def wide_motion(r):
    """B2: `motion` + `motion_hold` for every camera at max_batch 4 (a frame's whole_frame + max_regions fill a call) -- frames without
    ids are refused, a frame without an id behind two with ids ends the list where it would have joined, with ids one call per frame."""
    det = r.make("create", {"motion": {"threshold": 10, "min_side": 16}, "motion_hold": {"hold": 2}}, max_batch=4)
    buffers = {"a": rgb_buffer(), "b": rgb_buffer()}
    ids = r.step("bind_cameras", det, lambda: det.bind_cameras(buffers))
    batch(r, det, "detect_batch without ids", [rgb(1), rgb(2)])
    batch(r, det, "detect_batch with a frame without an id", [rgb(1), rgb(2), rgb(3)], [ids["a"], ids["b"], -1])
    batch(r, det, "detect_batch with ids", [rgb(1), rgb(2)], [ids["a"], ids["b"]])


def _relayout_detector(r):
    det = r.make("create", {"tiles": {"g": {"grid": [2, 1], "gate": _gate(8)}}, "motion": {"m": {"threshold": 10, "min_side": 16}},
                            "motion_hold": {"m": {"object_hold": 7}}, "ignore": {"g": [[0, 0, 16, 16]], "m": [[16, 32, 16, 16]]}})
    buffers = {"g": rgb_buffer(2), "m": rgb_buffer(2)}
    return det, buffers, r.step("bind_cameras", det, lambda: det.bind_cameras(buffers))


def relayout(r):
    """C: one gated and one motion camera seen at 64x48, again at 64x48 (no reconfiguration), then at 32x48 (settings, hold, mask)."""
    det, _, ids = _relayout_detector(r)
    cams = [ids["g"], ids["m"]]
    batch(r, det, "first 64x48", [rgb(1), rgb(2)], cams)
    batch(r, det, "second 64x48", [rgb(3), rgb(4)], cams)
    batch(r, det, "32x48", [rgb(5, w=32), rgb(6, w=32)], cams)
    batch(r, det, "64x48 again", [rgb(7), rgb(8)], cams)


def bind_twice(r):
    """C2: the tiled frame table of the same two cameras bound twice on one detector, then a synchronous batch."""
    det, buffers, ids = _relayout_detector(r)
    r.step("first bind", det, lambda: det.bind_tiled_frame_table(buffers, ids))
    r.step("second bind", det, lambda: det.bind_tiled_frame_table(buffers, ids))
    batch(r, det, "detect_batch after the binds", [rgb(1), rgb(2)], [ids["g"], ids["m"]])
    small = {"g": rgb_buffer(1, w=32), "m": rgb_buffer(1, w=32)}
    r.step("bind at 32x48", det, lambda: det.bind_tiled_frame_table(small, ids))
    batch(r, det, "detect_batch at 64x48 after the 32x48 bind", [rgb(1), rgb(2)], [ids["g"], ids["m"]])


def cutting(r):
    """D: max_batch 4, cameras with 3, 1, 3 and 2 tiles, two different `iou` among them, the gated one twice in the batch."""
    det = r.make("create", {"tiles": {"c3": {"grid": [2, 1]}, "c1": {"rects": [[0, 0, 64, 48]]},
                                      "c3b": {"rects": [[0, 0, 32, 48], [16, 0, 32, 48], [32, 0, 32, 48]], "iou": 0.5},
                                      "c2": {"grid": [2, 1], "full_frame": False, "gate": _gate(8)}}}, max_batch=4)
    buffers = {n: rgb_buffer() for n in ("c3", "c1", "c3b", "c2")}
    ids = r.step("bind_cameras", det, lambda: det.bind_cameras(buffers))
    names = ["c3", "c1", "c3b", "c2", "c2", "c1", "c3"]
    batch(r, det, "detect_batch", [rgb(i + 1) for i in range(len(names))], [ids[n] for n in names])
    r.step("bind_tiled_frame_table", det, lambda: det.bind_tiled_frame_table(buffers, ids))
    r.step("plan_bound", det, lambda: det.plan_bound([1, 0, 3, 2, 2, 1]))      # (table order: c1, c2, c3, c3b)


def plain(r):
    """E: no options -- detect() is one detect_batch with formats=None, bind_frame_table one bind_frames, and `submit_bound` /
    `collect_bound` are the engine's own bound methods."""
    det = r.make("create", {})
    out = rows(1)
    frame = rgb(9)
    r.step("detect", det, lambda: det.detect(frame.shape, frame.reshape(-1), out[0]), outputs=out)
    buffers = {"a": rgb_buffer(2), "b": rgb_buffer()}
    ids = r.step("bind_cameras", det, lambda: det.bind_cameras(buffers))
    r.step("bind_frame_table", det, lambda: det.bind_frame_table(buffers, ids))
    r.step("the engine's bound methods", det, lambda: [m.__self__ is det.engine and m.__func__ is getattr(RecordingEngine, n)
                                                       for n, m in (("submit_bound", det.submit_bound), ("collect_bound", det.collect_bound))])
    r.step("submit_host", det, lambda: det.submit_host(1, [rgb(1), rgb(2)], [-1, -1]))
    r.step("collect", det, lambda: det.collect(1, out), outputs=out)
    r.step("plan_bound", det, lambda: det.plan_bound(list(range(3)) * 4))
    r.step("exit", det, lambda: det.__exit__(None, None, None))


def wide_formats(r):
    """H: a detector-wide pixel format and an ungated detector-wide grid; one camera with GPU filters (drop=True), one with a colour
    range of its own, one with neither."""
    det = r.make("create", {"pixel_format": "nv12", "color_matrix": "bt709", "color_range": {"b": "full"},
                            "tiles": {"grid": [2, 1], "overlap": 0.25, "ios": 0.6}})
    buffers = {"a": nv12_buffer(), "b": nv12_buffer(), "c": nv12_buffer()}
    config = {"width": W, "height": H, "detect": [{"person": {"confidence": 50, "area": 10, "zones": []}}]}
    ids = r.step("bind_cameras", det, lambda: det.bind_cameras(buffers, {"c": config}, drop=True))
    out = rows(1)
    frame = nv12(5)
    r.step("detect", det, lambda: det.detect(frame.shape, frame.reshape(-1), out[0]), outputs=out)
    batch(r, det, "detect_batch with ids", [nv12(1), nv12(2), nv12(3)], [ids[n] for n in "abc"])
    r.step("bind_tiled_frame_table", det, lambda: det.bind_tiled_frame_table(buffers, ids))


def refusals(r):
    """F: what the plugin refuses, in its own words."""
    both = r.make("tiles and motion", {"tiles": {"t": {"rects": [[0, 0, 32, 32]]}, "g": {"grid": [2, 1], "gate": _gate(8)}},
                                       "motion": {"m": {"threshold": 10, "min_side": 16}}})
    ids = r.step("bind_cameras", both, lambda: both.bind_cameras({"t": rgb_buffer(), "g": rgb_buffer(), "m": rgb_buffer(), "p": rgb_buffer()}))
    r.step("bind_frame_table for a camera with tiles", both, lambda: both.bind_frame_table({"p": rgb_buffer(), "t": rgb_buffer()}, ids))
    r.step("bind_frame_table for a camera with motion", both, lambda: both.bind_frame_table({"p": rgb_buffer(), "m": rgb_buffer()}, ids))
    r.step("submit_host with tiles", both, lambda: both.submit_host(0, [rgb(1)], [-1]))
    two_sizes = fb(_Frame(W, H, 3, W * H * 3), _Frame(32, H, 3, 32 * H * 3))
    r.step("a gated camera with two sizes", both, lambda: both.bind_tiled_frame_table({"g": two_sizes, "p": rgb_buffer()}, ids))
    r.step("a motion camera with two sizes", both, lambda: both.bind_tiled_frame_table({"m": two_sizes, "p": rgb_buffer()}, ids))
    r.step("a motion camera without an id", both, lambda: both.bind_tiled_frame_table({"m": rgb_buffer(), "p": rgb_buffer()}, dict(ids, m=-1)))
    moving = r.make("motion for every camera", {"motion": {"threshold": 10}})
    r.step("submit_host with motion", moving, lambda: moving.submit_host(0, [rgb(1)], [0]))
    r.step("bind_frame_table with motion for every camera", moving, lambda: moving.bind_frame_table({"p": rgb_buffer()}, {"p": 0}))
    tiled = r.make("tiles for every camera", {"tiles": {"grid": [2, 2]}})
    r.step("bind_frame_table with tiles for every camera", tiled, lambda: tiled.bind_frame_table({"p": rgb_buffer()}, {"p": -1}))
    masked = r.make("ignore", {"motion": {"threshold": 10}, "ignore": {"garden": [[0, 0, 16, 16]], "attic": [[0, 0, 16, 16]]}})
    r.step("ignore naming unknown cameras", masked, lambda: masked.bind_cameras({"yard": rgb_buffer(), "door": rgb_buffer()}))
    outside = r.make("ignore outside", {"motion": {"threshold": 10}, "ignore": {"m": [[56, 40, 16, 16]]}})
    ids = r.step("bind_cameras", outside, lambda: outside.bind_cameras({"m": rgb_buffer()}))
    batch(r, outside, "an ignore rectangle outside the frame, detect_batch", [rgb(1)], [ids["m"]])
    r.step("an ignore rectangle outside the frame, bind", outside, lambda: outside.bind_tiled_frame_table({"m": rgb_buffer()}, ids))


_MOTION = {"threshold": 10}
CONSTRUCTOR_FAULTS = [        # two faults from different options each: which one the constructor reports
    ("schedule before pixel_format", {"schedule": "fast", "pixel_format": "p010"}, {}),
    ("pixel_format before tiles", {"pixel_format": "yuv422p", "tiles": {"grid": [0, 2]}}, {}),
    ("color_range before tiles", {"color_range": {"a": "pc"}, "tiles": 7}, {}),
    ("tiles before motion", {"tiles": {"a": {"grid": [2]}}, "motion": {"threshold": 256}}, {}),
    ("motion before motion_hold", {"motion": {"a": {"threshold": 10, "dilate": 3}}, "motion_hold": {"hold": 300}}, {}),
    ("motion_hold before ignore", {"motion": _MOTION, "motion_hold": {"b": {"hold": 0}}, "ignore": {"a": []}}, {}),
    ("motion_hold without motion before ignore", {"motion_hold": {"hold": 1}, "ignore": []}, {}),
    ("ignore before tiles over max_batch", {"tiles": {"grid": [3, 3]}, "ignore": {"a": [[0, 0, 16, 16]]}}, {"max_batch": 8}),
    ("tiles over max_batch before motion and tiles on one camera",
     {"tiles": {"a": {"grid": [3, 3]}}, "motion": {"a": _MOTION}}, {"max_batch": 8}),
    ("motion over max_batch before motion and tiles together", {"tiles": {"grid": [1, 1]}, "motion": dict(_MOTION, max_regions=4)},
     {"max_batch": 4}),
    ("motion for every camera with tiles per camera", {"tiles": {"a": {"grid": [1, 1]}}, "motion": _MOTION}, {}),
    ("tiles for every camera with motion per camera", {"tiles": {"grid": [1, 1]}, "motion": {"b": _MOTION, "a": _MOTION}}, {}),
]


def constructor_order(r):
    """G: the order the constructor checks its options in -- schedule, pixel format / colour matrix / range, tiles, motion, motion_hold,
    ignore, tiles against max_batch, the motion cross-checks."""
    for label, options, kw in CONSTRUCTOR_FAULTS:
        r.make(label, options, **kw)


SCENARIOS = {"A mixed": mixed, "B1 wide gate": wide_gate, "B2 wide motion": wide_motion, "C relayout": relayout, "C2 bind twice": bind_twice,
             "D cutting": cutting, "E plain": plain, "F refusals": refusals, "G constructor order": constructor_order,
             "H wide formats": wide_formats}


def record(name, hip_gpu):
    """The steps of scenario `name` under `hip_gpu.HipEngine` = `RecordingEngine` (the caller's patch), as plain data."""
    assert hip_gpu.HipEngine is RecordingEngine
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, hip_gpu.ENGINE_FILE), "wb").close()
        r = Recorder(hip_gpu, tmp)
        SCENARIOS[name](r)
    return json.loads(json.dumps(r.steps))      # (tuples become lists, as in the file)
