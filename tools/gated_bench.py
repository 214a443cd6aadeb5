"""What gating costs and saves: 1920x1080 RGB24 frames resident in HBM, `tile_grid(1920, 1080, 3, 2, 0.2)` = 7
tiles, on the robust `-p 16` engine (max_batch 8) that bench.py times; one camera per lane, gate (8, 1, 0).

  gated      `submit_gated_device` of the frame: activity launch + the host's decision + crop and batch of the tiles that run + commit + merge
  baseline   `submit_tiled_device` of the same tiles: every tile runs (code the gate does not touch)

in three scenes: (a) `busy`, every tile changes every step; (b) `still`, the same picture; (c) `patch`, a 64 x 64 patch moving inside the
first grid tile, so that tile and the full-frame tile run.  Both with every lane busy (frames/s) and as a lone call (p50), alternating
`--rounds` times in one process; then the HIP-event time of the activity launch and of the commit launch alone beside the crop launch's on
the same tiles (development library).  Prints one JSON line; --out appends a readable summary.

    python tools/gated_bench.py [--steps 400] [--warmup 40] [--rounds 3] [--out profiles/gated_tiles.txt]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH, HEIGHT, GRID, OVERLAP, BATCH, RING, GATE = 1920, 1080, (3, 2), 0.2, 8, 4, (8, 1, 0)


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
    busy = [synthetic_frame(WIDTH, HEIGHT, 1234 + i) for i in range(RING)]
    patch = []
    for i in range(RING):                      # the patch stays where only the first grid tile and the full-frame tile see it
        f = busy[0].copy()
        f[100:164, 100 + 80 * i:164 + 80 * i] = 255 - f[100:164, 100 + 80 * i:164 + 80 * i]
        patch.append(f)
    scenes = {"busy": busy, "still": [busy[0]] * RING, "patch": patch}
    expect = {"busy": len(rects), "still": 0, "patch": 2}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mi355x.bin")
        engine.save_engine(engine.build_engine(synthetic_weights(1234), robust=True), path)
        eng = HipEngine(path, 0, BATCH, WIDTH, HEIGHT)
        try:
            lanes = eng.num_slots
            for cam in range(lanes):
                eng.set_camera_tiles(cam, WIDTH, HEIGHT, rects, *GATE)
            runs, ran = {}, {}
            for name, frames in scenes.items():
                ptrs = [eng.upload(f) for f in frames]
                seen = [0] * lanes             # every camera walks the ring at its own pace: its picture changes with each of ITS calls

                def gated(lane, s, ptrs=ptrs, seen=seen):
                    seen[lane] += 1
                    eng.submit_gated_device(lane, [ptrs[seen[lane] % RING]], [WIDTH], [HEIGHT], [lane], ios=0.6)

                def tiled(lane, s, ptrs=ptrs, seen=seen):
                    seen[lane] += 1
                    eng.submit_tiled_device(lane, [ptrs[seen[lane] % RING]], [WIDTH], [HEIGHT], [rects], ios=0.6)

                runs[name] = {"gated": [], "baseline": []}
                for _ in range(args.rounds):
                    runs[name]["gated"].append(bench.throughput(eng, gated, 1, steps=args.steps, warm=args.warmup))
                    ran[name] = bin(eng.gate_stats(0)[0][0]).count("1")      # the last call's running tiles
                    runs[name]["baseline"].append(bench.throughput(eng, tiled, 1, steps=args.steps, warm=args.warmup))
                eng.sync()
                for p in ptrs:
                    eng.free(p)
        finally:
            eng.close()
        dev = HipEngine(path, 0, BATCH, WIDTH, HEIGHT, dev=True)
        try:
            ptrs = [dev.upload(f) for f in busy[:2]]
            dev.set_camera_tiles(0, WIDTH, HEIGHT, rects, *GATE)
            events, crops = [], []
            for i in range(3):                 # a reference first, then another picture: every tile is compared, runs and is committed
                dev.submit_gated_device(0, [ptrs[i % 2]], [WIDTH], [HEIGHT], [0], ios=0.6)
                dev.wait(0)
                events.append(dev.profile_gated([ptrs[(i + 1) % 2]], [WIDTH], [HEIGHT], [0], ios=0.6, reps=100))
                assert dev.gate_stats(0)[0][0] == (1 << len(rects)) - 1
                crops.append(dev.profile_tiled([ptrs[0]], [WIDTH], [HEIGHT], [rects], ios=0.6, reps=100))
        finally:
            dev.close()
    med = lambda name, leg, key: float(np.median([r[key] for r in runs[name][leg]]))      # noqa: E731
    luma_bytes = sum(3 * r[2] * r[3] for r in rects)
    out = dict(metric="gated_tiles", frame="%dx%d RGB24, resident in HBM" % (WIDTH, HEIGHT), tiles=len(rects), lanes=lanes, gate=list(GATE),
               bytes_read_by_activity=luma_bytes, grid_bytes_written=sum(2 * (-(-r[2] // 16)) * (-(-r[3] // 16)) for r in rects),
               steps=args.steps, rounds=args.rounds, tiles_ran_in_last_call=ran, tiles_expected=expect, scenes={},
               activity_launch_us=[round(e[0] * 1e3, 2) for e in events], commit_launch_us=[round(e[1] * 1e3, 2) for e in events],
               crop_launch_us=[round(c[0] * 1e3, 2) for c in crops], empty_bracket_us=[round(e[2] * 1e3, 2) for e in events])
    for name in scenes:
        out["scenes"][name] = dict(gated_frames_per_s=med(name, "gated", "value"), baseline_frames_per_s=med(name, "baseline", "value"),
                                   gated_p50_ms=med(name, "gated", "p50_ms"), baseline_p50_ms=med(name, "baseline", "p50_ms"))
    out["runs"] = runs
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("tools/gated_bench.py --steps %d --warmup %d --rounds %d on an MI355X: %s frames, tile_grid(%d, %d, %d, %d, %s) = %d tiles, gate %s, "
                    "one camera per lane, robust -p 16 engine, max_batch %d, %d lanes\n"
                    % (args.steps, args.warmup, args.rounds, out["frame"], WIDTH, HEIGHT, GRID[0], GRID[1], OVERLAP, len(rects), GATE, BATCH, lanes))
            for name in scenes:
                for leg in ("gated", "baseline"):
                    for i, r in enumerate(runs[name][leg]):
                        f.write("  %-5s round %d  %-8s  %9.1f frames/s with every lane busy (%.4f ms per step), lone call p50 %.4f ms\n"
                                % (name, i + 1, leg, r["value"], r["ms_per_step"], r["p50_ms"]))
                sc = out["scenes"][name]
                f.write("  %-5s medians: gated %.1f frames/s, lone p50 %.4f ms; ungated submit_tiled_device %.1f frames/s, lone p50 %.4f ms; "
                        "gated / ungated: %.3f x the frames/s, %.3f x the lone p50; tiles that ran in the last gated call: %d (expected %d)\n"
                        % (name, sc["gated_frames_per_s"], sc["gated_p50_ms"], sc["baseline_frames_per_s"], sc["baseline_p50_ms"],
                           sc["gated_frames_per_s"] / sc["baseline_frames_per_s"], sc["gated_p50_ms"] / sc["baseline_p50_ms"], ran[name], expect[name]))
            f.write("  HIP-event time of one launch alone, mean of 100, three measurements (us): activity %s (reads %.1f MB, writes %d bytes of grids), "
                    "commit of all %d tiles %s, crop of the same tiles %s, the bracket around nothing %s\n"
                    % (out["activity_launch_us"], luma_bytes / 1e6, out["grid_bytes_written"], len(rects), out["commit_launch_us"], out["crop_launch_us"],
                       out["empty_bracket_us"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
