"""What tiling costs: a 1920x1080 RGB24 frame resident in HBM, `tile_grid(1920, 1080, 3, 2, 0.2)` = 7 tiles, on the
robust `-p 16` engine (max_batch 8) that bench.py times.

  tiled      `submit_tiled_device` of the frame: crop launch + a batch of 7 + merge launch
  baseline   `submit_device` of the same 7 tiles, cropped beforehand into contiguous device images (what the parent commit can do)

Both with every lane busy (steps/s) and as a lone call (p50), alternating `--rounds` times in one process; then the HIP-event time of
the crop launch alone and of the merge launch alone (development library).  Prints one JSON line; --out appends a readable summary.

    python tools/tiled_bench.py [--steps 400] [--warmup 40] [--rounds 3] [--out profiles/tiled_detection.txt]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH, HEIGHT, GRID, OVERLAP, BATCH, RING = 1920, 1080, (3, 2), 0.2, 8, 4


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import bench
    from watsor_amd import engine
    from watsor_amd.runtime import HipEngine, tile_grid
    from watsor_amd.synth import synthetic_frame, synthetic_weights
    rects = tile_grid(WIDTH, HEIGHT, GRID[0], GRID[1], OVERLAP)
    frames = [synthetic_frame(WIDTH, HEIGHT, 1234 + i) for i in range(RING)]
    crop_bytes = sum(3 * r[2] * r[3] for r in rects)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mi355x.bin")
        engine.save_engine(engine.build_engine(synthetic_weights(1234), robust=True), path)
        eng = HipEngine(path, 0, BATCH, WIDTH, HEIGHT)
        try:
            d_frames = [eng.upload(f) for f in frames]
            d_crops = [[eng.upload(np.ascontiguousarray(f[y:y + h, x:x + w])) for x, y, w, h in rects] for f in frames]
            ws, hs = [r[2] for r in rects], [r[3] for r in rects]
            legs = {"tiled": lambda lane, s: eng.submit_tiled_device(lane, [d_frames[s % RING]], [WIDTH], [HEIGHT], [rects], ios=0.6),
                    "baseline": lambda lane, s: eng.submit_device(lane, d_crops[s % RING], ws, hs)}
            runs = {k: [] for k in legs}
            for _ in range(args.rounds):
                for name, submit in legs.items():
                    runs[name].append(bench.throughput(eng, submit, 1, steps=args.steps, warm=args.warmup))
            lanes = eng.num_slots
        finally:
            eng.close()
        dev = HipEngine(path, 0, BATCH, WIDTH, HEIGHT, dev=True)
        try:
            ptr = dev.upload(frames[0])
            events = [dev.profile_tiled([ptr], [WIDTH], [HEIGHT], [rects], ios=0.6, reps=100) for _ in range(3)]
        finally:
            dev.close()
    med = lambda name, key: float(np.median([r[key] for r in runs[name]]))      # noqa: E731
    out = dict(metric="tiled_detection_overhead", frame="%dx%d RGB24, resident in HBM" % (WIDTH, HEIGHT), tiles=len(rects), lanes=lanes,
               grid=list(GRID), overlap=OVERLAP, crop_bytes_written=crop_bytes, steps=args.steps, rounds=args.rounds,
               tiled_frames_per_s=med("tiled", "value"), baseline_steps_per_s=med("baseline", "value"),
               tiled_ms_per_step=med("tiled", "ms_per_step"), baseline_ms_per_step=med("baseline", "ms_per_step"),
               tiled_p50_ms=med("tiled", "p50_ms"), baseline_p50_ms=med("baseline", "p50_ms"),
               crop_launch_us=[round(e[0] * 1e3, 2) for e in events], merge_launch_us=[round(e[1] * 1e3, 2) for e in events],
               empty_bracket_us=[round(e[2] * 1e3, 2) for e in events])
    out["busy_ratio"] = round(out["tiled_ms_per_step"] / out["baseline_ms_per_step"], 4)
    out["lone_ratio"] = round(out["tiled_p50_ms"] / out["baseline_p50_ms"], 4)
    out["runs"] = runs
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("tools/tiled_bench.py --steps %d --warmup %d --rounds %d on an MI355X: one %s frame, tile_grid(%d, %d, %d, %d, %s) = %d tiles "
                    "(%.1f MB written by the crop), robust -p 16 engine, max_batch %d, %d lanes\n"
                    % (args.steps, args.warmup, args.rounds, out["frame"], WIDTH, HEIGHT, GRID[0], GRID[1], OVERLAP, len(rects), crop_bytes / 1e6,
                       BATCH, lanes))
            for name in legs:
                for i, r in enumerate(runs[name]):
                    f.write("  round %d  %-8s  %9.1f steps/s with every lane busy (%.4f ms per step), lone call p50 %.4f ms\n"
                            % (i + 1, name, r["value"], r["ms_per_step"], r["p50_ms"]))
            f.write("  medians: tiled %.1f frames/s, %.4f ms per step, lone p50 %.4f ms; baseline (submit_device of the %d pre-cropped tiles) "
                    "%.4f ms per step, lone p50 %.4f ms\n" % (out["tiled_frames_per_s"], out["tiled_ms_per_step"], out["tiled_p50_ms"], len(rects),
                                                              out["baseline_ms_per_step"], out["baseline_p50_ms"]))
            f.write("  overhead of tiling = tiled / baseline: %.4f with every lane busy, %.4f for a lone call\n" % (out["busy_ratio"], out["lone_ratio"]))
            f.write("  HIP-event time of one launch alone, mean of 100, three measurements (us): crop %s, merge %s, the bracket around nothing %s\n"
                    % (out["crop_launch_us"], out["merge_launch_us"], out["empty_bracket_us"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
