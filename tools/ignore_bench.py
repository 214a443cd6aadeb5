"""What an ignore mask costs, and that a camera without one pays nothing: HIP-event times of the two launches a
mask touches, for one 1920 x 1080 RGB24 camera, on the robust `-p 16` engine (development library).

  region launch     wz_k_motion_regions alone on a 120 x 68 grid with one changed blob and a burnt-in clock (`wz_profile_motion`): without a
                    mask -- and, where the tree has masks, with the clock's cells ignored (`wz_profile_motion_ignore`)
  activity launch   wz_k_tile_activity alone as one gated call of a camera with one whole-frame tile issues it (`wz_profile_gated`):
                    without a mask -- and, where the tree has masks, with the clock ignored (`set_camera_ignore`)

The mean of `--reps` brackets each, the empty bracket beside it.  The script runs on a tree WITHOUT masks too (it then prints the two
mask-free figures only): run it alternately on the parent tree and on this one, `--tree` names the tree whose package and library to load.
The two mask-free legs come first, so that up to them both trees make the same calls and allocations in the same order.
Prints one JSON line.

    python tools/ignore_bench.py [--tree DIR] [--reps 200] [--label NAME]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

WIDTH, HEIGHT, THR = 1920, 1080, 12
SETTINGS = dict(min_cells=1, dilate=1, max_regions=3, min_side=300, pad=8)
CLOCK = (1500, 40, 320, 32)      # x, y, w, h of the burnt-in timestamp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import motion_oracle as mo
    from watsor_amd import engine
    from watsor_amd.runtime import HipEngine
    from watsor_amd.synth import synthetic_weights

    gh, gw = mo.grid_shape(WIDTH, HEIGHT)
    x, y, w, h = CLOCK
    clock = np.zeros((gh, gw), bool)
    clock[y // 16:(y + h - 1) // 16 + 1, x // 16:(x + w - 1) // 16 + 1] = True
    blob = np.zeros((gh, gw), bool)
    blob[20:26, 50:58] = True
    now, ref = mo.grids_for(blob | clock, WIDTH, HEIGHT, THR)
    out = {"label": args.label, "tree": tree, "reps": args.reps, "cells": [gh, gw], "changed": int((blob | clock).sum()), "clock_cells": int(clock.sum())}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mi355x.bin")
        engine.save_engine(engine.build_engine(synthetic_weights(1234), robust=True), path)
        eng = HipEngine(path, 0, 8, WIDTH, HEIGHT, dev=True)
        try:
            masks = hasattr(eng, "set_camera_ignore")
            out["masks"] = masks
            us = lambda ms: round(1e3 * ms, 2)      # noqa: E731
            reg, act, empty, rounds = eng.profile_motion(now, ref, WIDTH, HEIGHT, THR, reps=args.reps, **SETTINGS)
            out["region_us"], out["region_empty_us"], out["rounds"] = us(reg), us(empty), rounds
            # the activity launch: frame A is the reference, frame B (the blob and the clock changed) is what the profiled launch reads
            rng = np.random.default_rng(19)
            a = rng.integers(0, 200, (HEIGHT, WIDTH, 3), dtype=np.uint8)
            b = a.copy()
            b[320:416, 800:928] = 255
            b[y:y + h, x:x + w] = 255
            d_a, d_b = eng.upload(a), eng.upload(b)
            cam, whole = 3, [(0, 0, WIDTH, HEIGHT)]
            plane = np.zeros((HEIGHT, WIDTH), np.uint8)
            plane[y:y + h, x:x + w] = 1
            for leg in ("activity", "activity_masked") if masks else ("activity",):
                eng.set_camera_tiles(cam, WIDTH, HEIGHT, whole, THR, 1, 0)
                if leg == "activity_masked":
                    eng.set_camera_ignore(cam, plane)
                eng.submit_gated_device(0, [d_a], [WIDTH], [HEIGHT], [cam])
                eng.wait(0)
                act, commit, empty = eng.profile_gated([d_b], [WIDTH], [HEIGHT], [cam], reps=args.reps)
                out[leg + "_us"], out[leg + "_empty_us"] = us(act), us(empty)
                out[leg + "_cells"] = int(eng.gate_stats(0)[1][0][0])
                eng.clear_camera_tiles(cam)
            if masks:
                reg, empty = eng.profile_motion_ignore(now, ref, clock.astype(np.uint8), WIDTH, HEIGHT, THR, reps=args.reps, **SETTINGS)
                out["region_masked_us"], out["region_masked_empty_us"] = us(reg), us(empty)
        finally:
            eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
