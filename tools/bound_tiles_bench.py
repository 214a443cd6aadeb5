"""What the worker's frame table buys tiled and gated detection: 1920x1080 frames in ONE page-locked arena, the robust
`-p 16` engine that bench.py times, max_batch 8, four lanes; a step is one frame -- `submit_bound(lane, [entry])`, the lane's previous batch
collected first, as the worker retires the oldest batch before it reuses a lane.

  (a) tiled      `tile_grid(1920, 1080, 3, 2, 0.2)` = 7 tiles a frame through bound submits, against the synchronous path a worker takes without
                 `hip_tiled_table`: `HipObjectDetector.detect_batch()` of 8 such frames, one call at a time -- run by the SAME script in a child
                 process of the tree given with --parent (the parent commit's build; without it: this tree's)
  (b) roi        one 640 x 480 region of interest, RGB24 and NV12: read in place by the crop kernel over PCIe, against the same frames staged whole
                 by DMA (WZ_HOST_READ=0), both on the development library, which also says which leg a frame took
  (c) gated      the 7 tiles with the gate (8, 1, 0), one camera per lane: a still picture, and a 64 x 64 patch moving inside the first grid tile
  (d) motion, still     a motion camera per lane -- threshold 8, min_cells 1, dilate 1, max_regions 3, min_side 300, pad 8 --
                 with whole_frame 0 and a still picture: no tile ever runs, a step is the DMA, the activity and the region launch
  (e) motion, patch    the same cameras with whole_frame 1 and the 64 x 64 patch moving: the whole frame and the region around the patch
                 (d) and (e) as RGB24 and as NV12, through bound submits (`wz_bind_motion`) -- one frame per bound batch and, as `plan_bound`
                 cuts a dequeued batch of the four cameras, two --, against the synchronous path a worker takes without
                 `hip_tiled_table`: the plugin with the same `motion` option, `detect_batch()` of one frame of each of the four cameras, one call
                 at a time, in a child process of the --parent tree.  Beside the frames/s: the p50 of the time spent INSIDE `submit_bound` (the
                 DMA, the two launches and the call's one stream wait)

Medians of --rounds alternating rounds.  Prints one JSON line; --out appends a readable summary.  --legs tiles | motion | all: (a) - (c), (d) - (e), both.

    python tools/bound_tiles_bench.py [--steps 400] [--warmup 40] [--rounds 3] [--legs all] [--parent DIR] [--out profiles/bound_tiles.txt]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTH, HEIGHT, GRID, OVERLAP, BATCH, RING, GATE = 1920, 1080, (3, 2), 0.2, 8, 4, (8, 1, 0)
ROI = (640, 300, 640, 480)

# The synchronous path, in terms the parent commit knows: the plugin with a `tiles` option, detect_batch() of 8 page-locked frames per call.
SYNC_BASELINE = r"""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
from watsor_amd.detection.hip_gpu import HipObjectDetector
from watsor_amd.share import DetectionArray
from watsor_amd.synth import synthetic_frame
model_dir, steps, warm = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
W, H, N = %d, %d, %d
arena = np.stack([synthetic_frame(W, H, 1234 + i) for i in range(N)])
opts = {"tiles": {"grid": [%d, %d], "overlap": %r, "ios": 0.6}, "numa": False}
with HipObjectDetector(model_dir, 0, opts, max_batch=N, max_width=W, max_height=H) as det:
    det.engine.host_register(arena)
    frames, rows = [arena[i] for i in range(N)], [DetectionArray() for _ in range(N)]
    shapes = [f.shape for f in frames]
    calls = max(1, steps // N)
    for _ in range(max(1, warm // N)):
        det.detect_batch(shapes, frames, rows)
    t0 = time.perf_counter()
    for _ in range(calls):
        det.detect_batch(shapes, frames, rows)
    dt = time.perf_counter() - t0
    det.engine.sync()
    det.engine.host_unregister(arena)
print(json.dumps(dict(value=round(calls * N / dt, 1), ms_per_frame=round(dt / (calls * N) * 1e3, 4), frames=calls * N)))
""" % (WIDTH, HEIGHT, BATCH, GRID[0], GRID[1], OVERLAP)


MOTION = dict(threshold=GATE[0], min_cells=1, dilate=1, max_regions=3, min_side=300, pad=8)
MOTION_LEGS = {"motion_still": False, "motion_patch": True}       # leg -> whole_frame (and: the patch moves)

# The synchronous path of a motion camera, in terms the parent commit knows: the plugin with a `motion` option, detect_batch() of one
# page-locked frame of each camera per call (a motion call takes one frame of a camera).  The pictures are this script's (argv[6]: its folder).
MOTION_SYNC_BASELINE = r"""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
sys.path.append(sys.argv[6])
import numpy as np
import bound_tiles_bench as bt
from watsor_amd.detection.hip_gpu import HipObjectDetector
from watsor_amd.share import DetectionArray
model_dir, steps, warm, leg, kind = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
cams = 4
arena = np.stack([np.stack(bt.motion_pictures(leg, kind)) for _ in range(cams)])
opts = {"motion": dict(bt.MOTION, whole_frame=bt.MOTION_LEGS[leg], ios=0.6), "pixel_format": kind, "numa": False}
with HipObjectDetector(model_dir, 0, opts, max_batch=bt.BATCH, max_width=bt.WIDTH, max_height=bt.HEIGHT) as det:
    det.engine.host_register(arena)
    rows, ids = [DetectionArray() for _ in range(cams)], list(range(cams))
    shapes = [arena[0, 0].shape] * cams
    def call(k):
        det.detect_batch(shapes, [arena[c, k % bt.RING] for c in ids], rows, cameras=ids)
    calls = max(1, steps // cams)
    for k in range(max(1, warm // cams)):
        call(k)
    t0 = time.perf_counter()
    for k in range(calls):
        call(warm + k)
    dt = time.perf_counter() - t0
    det.engine.sync()
    det.engine.host_unregister(arena)
print(json.dumps(dict(value=round(calls * cams / dt, 1), ms_per_frame=round(dt / (calls * cams) * 1e3, 4), frames=calls * cams)))
"""


def motion_pictures(leg, kind):
    """the RING pictures a camera of leg (d) / (e) walks: one still picture, or the 64 x 64 patch moving 80 pixels a step; kind: rgb24 | nv12"""
    from watsor_amd.synth import synthetic_frame
    base = synthetic_frame(WIDTH, HEIGHT, 1234)
    pictures = []
    for i in range(RING):
        f = base.copy()
        if MOTION_LEGS[leg]:
            f[100:164, 100 + 80 * i:164 + 80 * i] = 255 - f[100:164, 100 + 80 * i:164 + 80 * i]
        pictures.append(f if kind == "rgb24" else nv12_of(f))
    return pictures


def sync_baseline(tree, model_dir, steps, warm, motion=None):
    """motion = (leg, kind): the motion baseline of that leg; None: the tiled one of (a)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WATSOR_HIP_DEV", "WZ_HOST_READ")}
    script, extra = (SYNC_BASELINE, []) if motion is None else (MOTION_SYNC_BASELINE, list(motion) + [os.path.dirname(os.path.abspath(__file__))])
    p = subprocess.run([sys.executable, "-c", script, model_dir, str(steps), str(warm)] + extra, cwd=tree, env=env, capture_output=True, text=True,
                       timeout=300)
    if p.returncode != 0:
        raise RuntimeError("synchronous baseline in %s failed (rc %d): %s" % (tree, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def bound_steps(eng, entry_of, steps, warm, submit_times=False, per=1):
    """frames/s of one-frame bound batches over the engine's lanes (collect, then submit again) + the p50 of a lone submit + collect;
    submit_times: + the p50 of the time spent inside `submit_bound` during the measured steps, every lane busy; per > 1: entry_of returns
    the `per` entries of a step's batch"""
    lanes = eng.num_slots
    inside = []
    batch = entry_of if per > 1 else (lambda lane, s: [entry_of(lane, s)])

    def run(n, first, timed=False):
        busy = []
        for s in range(first, first + n):
            lane = s % lanes
            if lane in busy:
                eng.collect_bound(lane)
                busy.remove(lane)
            if timed:
                t1 = time.perf_counter()
                eng.submit_bound(lane, batch(lane, s))
                inside.append((time.perf_counter() - t1) * 1e3)
            else:
                eng.submit_bound(lane, batch(lane, s))
            busy.append(lane)
        for lane in busy:
            eng.collect_bound(lane)

    run(warm, 0)
    t0 = time.perf_counter()
    run(steps, warm, submit_times)
    dt = time.perf_counter() - t0
    lat = []
    for s in range(60):
        t1 = time.perf_counter()
        eng.submit_bound(0, batch(0, warm + steps + s))
        eng.collect_bound(0)
        lat.append((time.perf_counter() - t1) * 1e3)
    res = dict(value=round(steps * per / dt, 1), ms_per_step=round(dt / steps * 1e3, 4), p50_ms=round(float(np.median(lat)), 4))
    if submit_times:
        res["submit_p50_ms"] = round(float(np.median(inside)), 4)
    return res


class Arena:
    """`cams` cameras of RING frames each in one page-locked arena, bound as one frame table: entry = cam * RING + frame"""

    def __init__(self, eng, pictures, fmt, cams, with_ids=False):
        from watsor_amd.runtime import ROW_DTYPE
        self.eng = eng
        self.arena = np.stack([np.stack(pictures) for _ in range(cams)])
        eng.host_register(self.arena)
        n = cams * RING
        self.rows = np.zeros((n, 100), ROW_DTYPE)
        views = [self.arena[c, i] for c in range(cams) for i in range(RING)]
        eng.bind_frames([v.ctypes.data for v in views], [WIDTH] * n, [HEIGHT] * n, [fmt] * n,
                        [(c if with_ids else -1) for c in range(cams) for _ in range(RING)], [self.rows[i].ctypes.data for i in range(n)])

    def close(self):
        self.eng.sync()
        self.eng.bind_frames([], [], [], [], [], [])
        self.eng.host_unregister(self.arena)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="tree of the parent commit, built: where the synchronous baselines of (a), (d) and (e) run")
    ap.add_argument("--legs", default="all", choices=("all", "tiles", "motion"), help="tiles: (a) - (c); motion: (d) - (e)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    tiles_legs, motion_legs = args.legs in ("all", "tiles"), args.legs in ("all", "motion")
    sys.path.insert(0, ROOT)
    from watsor_amd import engine
    from watsor_amd.runtime import FMT_NV12, FMT_RGB24, HipEngine, tile_grid
    from watsor_amd.synth import synthetic_frame, synthetic_weights
    rects = tile_grid(WIDTH, HEIGHT, GRID[0], GRID[1], OVERLAP)
    busy = [synthetic_frame(WIDTH, HEIGHT, 1234 + i) for i in range(RING)]
    patch = []
    for i in range(RING):                      # the patch stays where only the first grid tile and the full-frame tile see it
        f = busy[0].copy()
        f[100:164, 100 + 80 * i:164 + 80 * i] = 255 - f[100:164, 100 + 80 * i:164 + 80 * i]
        patch.append(f)
    baseline_tree = os.path.abspath(args.parent) if args.parent else ROOT
    seen = {}

    def walk(lane, s):                         # every lane is a camera that walks its own ring of frames
        seen[lane] = seen.get(lane, 0) + 1
        return lane * RING + seen[lane] % RING

    def pairs(lane, s):                        # (d), (e): lanes 0 and 2 take the cameras 0 and 1, lanes 1 and 3 the cameras 2 and 3
        p = lane % 2
        seen["pair", p] = k = seen.get(("pair", p), 0) + 1
        return [2 * p * RING + k % RING, (2 * p + 1) * RING + k % RING]

    out = dict(metric="bound_tiles", frame="%dx%d, one page-locked arena" % (WIDTH, HEIGHT), tiles=len(rects), roi=list(ROI), gate=list(GATE),
               steps=args.steps, rounds=args.rounds, baseline_tree="parent commit" if args.parent else "this tree")
    runs = dict(tiled_bound=[], tiled_sync=[], gated_still=[], gated_patch=[]) if tiles_legs else {}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mi355x.bin")
        engine.save_engine(engine.build_engine(synthetic_weights(1234), robust=True), path)
        if tiles_legs:
            # ---- (a) and (c): the product library
            eng = HipEngine(path, 0, BATCH, WIDTH, HEIGHT)
            try:
                lanes = out["lanes"] = eng.num_slots
                for r in range(args.rounds):
                    a = Arena(eng, busy, FMT_RGB24, lanes)
                    eng.bind_tiles(0, lanes * RING, rects, ios=0.6)
                    runs["tiled_bound"].append(bound_steps(eng, walk, args.steps, args.warmup))
                    a.close()
                    runs["tiled_sync"].append(sync_baseline(baseline_tree, d, args.steps, args.warmup))
                    for name, pictures in (("gated_still", [busy[0]] * RING), ("gated_patch", patch)):
                        a = Arena(eng, pictures, FMT_RGB24, lanes, with_ids=True)
                        for cam in range(lanes):
                            eng.set_camera_tiles(cam, WIDTH, HEIGHT, rects, *GATE)
                            eng.bind_tiles(cam * RING, RING, None, ios=0.6, gated=True)
                        res = bound_steps(eng, walk, args.steps, args.warmup)
                        res["tiles_ran_in_last_call"] = bin(eng.gate_stats(0)[0][0]).count("1")
                        runs[name].append(res)
                        a.close()
            finally:
                eng.close()
            # ---- (b): the development library, default setting against WZ_HOST_READ=0
            engines = {}
            for leg, env in (("in_place", None), ("staged", "0")):
                os.environ.pop("WZ_HOST_READ", None)
                if env is not None:
                    os.environ["WZ_HOST_READ"] = env
                engines[leg] = HipEngine(path, 0, BATCH, WIDTH, HEIGHT, dev=True)      # (the knob is read when the engine is created)
                os.environ.pop("WZ_HOST_READ", None)
            try:
                for kind, fmt in (("rgb24", FMT_RGB24), ("nv12", FMT_NV12)):
                    pictures = busy if kind == "rgb24" else [nv12_of(f) for f in busy]
                    roi_bytes = ROI[2] * ROI[3] * (3 if kind == "rgb24" else 1.5)
                    for leg in engines:
                        runs["roi_%s_%s" % (kind, leg)] = []
                    for r in range(args.rounds):
                        for leg, e in engines.items():
                            a = Arena(e, pictures, fmt, lanes)
                            e.bind_tiles(0, lanes * RING, [ROI], ios=0.6)
                            res = bound_steps(e, walk, args.steps, args.warmup)
                            res["read_in_place"] = e.bound_source(0)[0]
                            res["bytes_per_frame_over_pcie"] = int(roi_bytes) if res["read_in_place"] else int(pictures[0].size)
                            runs["roi_%s_%s" % (kind, leg)].append(res)
                            a.close()
            finally:
                for e in engines.values():
                    e.close()
        # ---- (d) and (e): the product library, a motion camera per lane
        if motion_legs:
            eng = HipEngine(path, 0, BATCH, WIDTH, HEIGHT)
            try:
                lanes = out["lanes"] = eng.num_slots
                out["motion"] = dict(MOTION)
                for leg in MOTION_LEGS:
                    for kind in ("rgb24", "nv12"):
                        runs["%s_%s_bound" % (leg, kind)], runs["%s_%s_sync" % (leg, kind)] = [], []
                        runs["%s_%s_bound_pairs" % (leg, kind)] = []
                for r in range(args.rounds):
                    for leg, whole in MOTION_LEGS.items():
                        for kind, fmt in (("rgb24", FMT_RGB24), ("nv12", FMT_NV12)):
                            a = Arena(eng, motion_pictures(leg, kind), fmt, lanes, with_ids=True)
                            for cam in range(lanes):
                                eng.set_camera_motion(cam, WIDTH, HEIGHT, whole_frame=whole, fmt=fmt, **MOTION)
                                eng.bind_motion(cam * RING, RING, ios=0.6)
                            res = bound_steps(eng, walk, args.steps, args.warmup, submit_times=True)
                            res["tiles_in_last_call"] = len(eng.motion_stats(0)[0][0])
                            runs["%s_%s_bound" % (leg, kind)].append(res)
                            # ... and in the pieces `plan_bound` cuts a dequeued batch of these four cameras into: two cameras a bound batch
                            res = bound_steps(eng, pairs, args.steps // 2, args.warmup // 2, submit_times=True, per=2)
                            runs["%s_%s_bound_pairs" % (leg, kind)].append(res)
                            a.close()
                            for cam in range(lanes):
                                eng.clear_camera_motion(cam)
                            runs["%s_%s_sync" % (leg, kind)].append(sync_baseline(baseline_tree, d, args.steps, args.warmup, motion=(leg, kind)))
            finally:
                eng.close()
    med = lambda leg, key: float(np.median([r[key] for r in runs[leg]]))      # noqa: E731
    out["frames_per_s"] = {leg: med(leg, "value") for leg in runs}
    out["lone_p50_ms"] = {leg: med(leg, "p50_ms") for leg in runs if "p50_ms" in runs[leg][0]}
    out["runs"] = runs
    print(json.dumps(out), flush=True)
    if args.out:
        fps = out["frames_per_s"]
        with open(args.out, "a") as f:
            f.write("tools/bound_tiles_bench.py --steps %d --warmup %d --rounds %d on an MI355X: %s, robust -p 16 engine, max_batch %d, %d lanes, one frame "
                    "per bound batch\n" % (args.steps, args.warmup, args.rounds, out["frame"], BATCH, lanes))
            for leg, rs in runs.items():
                for i, r in enumerate(rs):
                    f.write("  %-22s round %d  %s\n" % (leg, i + 1, json.dumps(r)))
            if tiles_legs:
                f.write("  (a) tile_grid(%d, %d, %d, %d, %s) = %d tiles: bound submits on %d lanes %.1f frames/s (lone submit + collect p50 %.4f ms); "
                        "detect_batch() of 8 frames, one call at a time, on the %s's build %.1f frames/s: %.3f x\n"
                        % (WIDTH, HEIGHT, GRID[0], GRID[1], OVERLAP, len(rects), lanes, fps["tiled_bound"], out["lone_p50_ms"]["tiled_bound"],
                           out["baseline_tree"], fps["tiled_sync"], fps["tiled_bound"] / fps["tiled_sync"]))
                for kind in ("rgb24", "nv12"):
                    a, b = "roi_%s_in_place" % kind, "roi_%s_staged" % kind
                    f.write("  (b) one %d x %d region at (%d, %d), %s: read in place %.1f frames/s (%d bytes a frame over PCIe, lone p50 %.4f ms); staged whole "
                            "(WZ_HOST_READ=0) %.1f frames/s (%d bytes, lone p50 %.4f ms): in place / staged %.3f x\n"
                            % (ROI[2], ROI[3], ROI[0], ROI[1], kind, fps[a], runs[a][0]["bytes_per_frame_over_pcie"], out["lone_p50_ms"][a], fps[b],
                               runs[b][0]["bytes_per_frame_over_pcie"], out["lone_p50_ms"][b], fps[a] / fps[b]))
                for leg in ("gated_still", "gated_patch"):
                    f.write("  (c) %s, gate %s, one camera per lane: %.1f frames/s (lone p50 %.4f ms), tiles that ran in the last call: %d; "
                            "against the ungated bound submits of (a): %.3f x\n"
                            % (leg, GATE, fps[leg], out["lone_p50_ms"][leg], runs[leg][-1]["tiles_ran_in_last_call"], fps[leg] / fps["tiled_bound"]))
            for leg, whole in MOTION_LEGS.items() if motion_legs else ():
                for kind in ("rgb24", "nv12"):
                    a, b = "%s_%s_bound" % (leg, kind), "%s_%s_sync" % (leg, kind)
                    spread, c = [r["value"] for r in runs[b]], a + "_pairs"
                    f.write("  (%s) %s, %s, whole_frame %d, motion %s, one camera per lane: bound submits on %d lanes %.1f frames/s (lone submit + collect p50 "
                            "%.4f ms, inside submit_bound p50 %.4f ms, tiles in the last call: %d); detect_batch() of one frame of each camera, one call at a "
                            "time, on the %s's build %.1f frames/s (its rounds: %.1f .. %.1f): %.3f x; two cameras a bound batch: %.1f frames/s, %.3f x (inside submit_bound p50 %.4f ms)\n"
                            % ("e" if whole else "d", leg, kind, whole, json.dumps(MOTION), lanes, fps[a], out["lone_p50_ms"][a],
                               float(np.median([r["submit_p50_ms"] for r in runs[a]])), runs[a][-1]["tiles_in_last_call"], out["baseline_tree"], fps[b],
                               min(spread), max(spread), fps[a] / fps[b], fps[c], fps[c] / fps[b], float(np.median([r["submit_p50_ms"] for r in runs[c]]))))
    return 0


def nv12_of(rgb):
    """an NV12 picture of an RGB one (BT.601, limited range; chroma averaged over 2 x 2): test input, any bytes would do"""
    r, g, b = [rgb[..., i].astype(np.float32) for i in range(3)]
    y = 16 + 0.257 * r + 0.504 * g + 0.098 * b
    u = 128 - 0.148 * r - 0.291 * g + 0.439 * b
    v = 128 + 0.439 * r - 0.368 * g - 0.071 * b
    h, w = y.shape
    sub = lambda p: p.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))      # noqa: E731
    chroma = np.stack([sub(u), sub(v)], axis=-1).reshape(h // 2, w)
    return np.clip(np.rint(np.concatenate([y, chroma])), 0, 255).astype(np.uint8)


if __name__ == "__main__":
    sys.exit(main())
