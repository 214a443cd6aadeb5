"""What motion regions cost, on the robust `-p 16` engine (max_batch 8) that bench.py times.

  launches   HIP-event time of the region launch alone on a 1080p grid (120 x 68 cells), mean of 100 with the empty bracket beside it, for a
             still picture, one blob, 2 % noise (dilate 1) and the one-cell serpentine (dilate 0) -- and of the whole-frame activity launch of
             a 1920 x 1080 RGB24 frame beside it (development library), three measurements each
             and, as a yardstick for the same step on a host thread, scipy's dilation + labelling + boxes + counts on the same grids
  lone call  p50 of a lone `submit_motion_device` + wait with whole_frame 1 whose picture changes in one place (the whole frame and one
             region: a batch of two), against `submit_tiled_device` + wait of the same frames on the same two rectangles -- code this
             feature does not touch; the difference is what finding the rectangle costs.  Alternating `--rounds` times in one process.

  --hold     instead of the two above: what a camera with a hold pays on top -- the region launch with ages, with
             ages that are all zero and without, on still / blob / noise, and the stamp launch alone with 0 / 1 / 100 passing rows

Prints one JSON line; --out appends a readable summary.

    python tools/motion_bench.py [--steps 200] [--rounds 3] [--out profiles/motion_regions.txt]
    python tools/motion_bench.py --hold [--out profiles/motion_hold.txt]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WIDTH, HEIGHT, BATCH, THR = 1920, 1080, 8, 12
SETTINGS = dict(min_cells=1, dilate=1, max_regions=3, min_side=300, pad=8)


def lone_p50(eng, submit, steps, warm=20):
    lat = []
    for s in range(steps + warm):
        t1 = time.perf_counter()
        submit(s)
        eng.wait(0)
        if s >= warm:
            lat.append((time.perf_counter() - t1) * 1e3)
    return round(float(np.median(lat)), 4)


def host_labelling_us(C, dilate, reps=200):
    """A yardstick for the same step on a host thread: scipy's C code for dilation, 8-connected labelling, the components' boxes and their
    counts of changed cells on the grid C (no grid travels, no ranking, no walk): median of `reps`, in microseconds; None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    eight = np.ones((3, 3), bool)
    lat = []
    for _ in range(reps):
        t1 = time.perf_counter()
        D = ndimage.binary_dilation(C, structure=np.ones((2 * dilate + 1,) * 2, bool)) if dilate else C
        lab, count = ndimage.label(D, structure=eight)
        ndimage.find_objects(lab)
        np.bincount(lab[C], minlength=count + 1)
        lat.append((time.perf_counter() - t1) * 1e6)
    return round(float(np.median(lat)), 1)


def hold_leg(args):
    """--hold: what a camera with a hold pays on top, on the same 120 x 68 grid.  The region launch with ages -- 2 %
    of the cells hold a seeded age of 1 .. 255 -- against the same launch without, on still / blob / noise; the stamp launch alone with 0, 1
    and 100 passing rows (100 seeded boxes of up to 600 x 400 pixels).  HIP-event brackets, mean of 100, the empty bracket beside it, three
    measurements each."""
    import motion_hold_oracle as ho
    import motion_oracle as mo
    from watsor_amd import engine
    from watsor_amd.runtime import ROW_DTYPE, HipEngine
    from watsor_amd.synth import synthetic_weights
    gh, gw = mo.grid_shape(WIDTH, HEIGHT)
    rng = np.random.default_rng(19)
    blob = np.zeros((gh, gw), bool)
    blob[20:26, 50:58] = True
    grids = {"still": np.zeros((gh, gw), bool), "blob": blob, "noise": rng.random((gh, gw)) < 0.02}
    age = np.where(rng.random((gh, gw)) < 0.02, rng.integers(1, 256, (gh, gw)), 0).astype(np.uint8)
    rows = np.zeros(100, ROW_DTYPE)
    rows["label"] = 1
    rows["x_min"], rows["y_min"] = rng.integers(0, WIDTH - 600, 100), rng.integers(0, HEIGHT - 400, 100)
    rows["x_max"], rows["y_max"] = rows["x_min"] + rng.integers(16, 600, 100), rows["y_min"] + rng.integers(16, 400, 100)
    med = lambda v: float(np.median(v))      # noqa: E731
    us = lambda v: round(v * 1e3, 2)         # noqa: E731
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mi355x.bin")
        engine.save_engine(engine.build_engine(synthetic_weights(1234), robust=True), path)
        dev = HipEngine(path, 0, BATCH, WIDTH, HEIGHT, dev=True)
        launches, stamps = {}, {}
        try:
            for name, C in grids.items():
                now, ref = mo.grids_for(C, WIDTH, HEIGHT, THR)
                found = dev.stage_motion_hold(now, ref, age, WIDTH, HEIGHT, THR, 5, **SETTINGS)
                want = ho.step(now, ref, age, WIDTH, HEIGHT, 0, THR, 5, **SETTINGS)
                assert found[:5] == want[:5] and (found[5] == want[5]).all(), name
                aged = [dev.profile_motion_hold(now, ref, age, rows, np.zeros(100, np.uint8), WIDTH, HEIGHT, THR, 5, 3, reps=100, **SETTINGS) for _ in range(3)]
                zero = [dev.profile_motion_hold(now, ref, np.zeros_like(age), rows, np.zeros(100, np.uint8), WIDTH, HEIGHT, THR, 5, 3, reps=100, **SETTINGS)
                        for _ in range(3)]      # ages that are all zero: the same regions as without, plus the age byte's load and store
                plain = [dev.profile_motion(now, ref, WIDTH, HEIGHT, THR, reps=100, **SETTINGS) for _ in range(3)]
                launches[name] = dict(changed_cells=int(C.sum()), active=found[3], held=found[4], components=found[2],
                                      with_ages_us=[us(r[0]) for r in aged], with_ages_empty_us=[us(r[2]) for r in aged],
                                      zero_ages_us=[us(r[0]) for r in zero], zero_ages_empty_us=[us(r[2]) for r in zero],
                                      without_us=[us(r[0]) for r in plain], without_empty_us=[us(r[2]) for r in plain],
                                      plain_changed_components=dev.stage_motion_regions(now, ref, WIDTH, HEIGHT, THR, **SETTINGS)[2])
            now, ref = mo.grids_for(grids["blob"], WIDTH, HEIGHT, THR)
            for passing in (0, 1, 100):
                ok = np.zeros(100, np.uint8)
                ok[:passing] = 1
                got = dev.stage_motion_stamp(age, rows, ok, WIDTH, HEIGHT, 3)
                assert (got == ho.stamp(age, rows, ok, WIDTH, HEIGHT, 3)).all(), passing
                runs = [dev.profile_motion_hold(now, ref, age, rows, ok, WIDTH, HEIGHT, THR, 5, 3, reps=100, **SETTINGS) for _ in range(3)]
                stamps[str(passing)] = dict(cells_raised=int((got != age).sum()), stamp_us=[us(r[1]) for r in runs], empty_us=[us(r[2]) for r in runs])
        finally:
            dev.close()
    out = dict(metric="motion_hold", grid="%d x %d cells (%dx%d)" % (gw, gh, WIDTH, HEIGHT), threshold=THR, settings=SETTINGS, hold=5, object_hold=3,
               aged_cells=int((age > 0).sum()), launches=launches, stamp=stamps)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("tools/motion_bench.py --hold on an MI355X: %s, threshold %d, %s, hold 5, object_hold 3, %d cells with a seeded age\n"
                    % (out["grid"], THR, SETTINGS, out["aged_cells"]))
            f.write("  HIP-event time of one launch alone, mean of 100, three measurements (us); the bracket around nothing beside it\n")
            for name, r in launches.items():
                f.write("  %-6s %4d changed + %3d held cells, %3d components (%d without ages): region launch with ages %s (empty %s), with ages all zero %s (empty %s), "
                        "without %s (empty %s) -> %.2f / %.2f / %.2f us above the bracket\n"
                        % (name, r["changed_cells"], r["held"], r["components"], r["plain_changed_components"], r["with_ages_us"], r["with_ages_empty_us"],
                           r["zero_ages_us"], r["zero_ages_empty_us"], r["without_us"], r["without_empty_us"],
                           med(r["with_ages_us"]) - med(r["with_ages_empty_us"]), med(r["zero_ages_us"]) - med(r["zero_ages_empty_us"]),
                           med(r["without_us"]) - med(r["without_empty_us"])))
            for passing, r in stamps.items():
                f.write("  stamp launch, %3s passing rows (%4d cells raised the first time): %s (empty %s) -> %.2f us above the bracket\n"
                        % (passing, r["cells_raised"], r["stamp_us"], r["empty_us"], med(r["stamp_us"]) - med(r["empty_us"])))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hold", action="store_true", help="only the motion-hold leg: the region launch with ages, the stamp launch (DESIGN.md section 19b)")
    args = ap.parse_args(argv)
    if args.hold:
        return hold_leg(args)
    import motion_oracle as mo
    from watsor_amd import engine
    from watsor_amd.runtime import HipEngine
    from watsor_amd.synth import synthetic_frame, synthetic_weights
    gh, gw = mo.grid_shape(WIDTH, HEIGHT)
    rng = np.random.default_rng(19)
    blob = np.zeros((gh, gw), bool)
    blob[20:26, 50:58] = True
    grids = {"still": (np.zeros((gh, gw), bool), 1), "blob": (blob, 1), "noise": (rng.random((gh, gw)) < 0.02, 1),
             "serpentine": (mo.serpentine(gh, gw), 0)}
    a = synthetic_frame(WIDTH, HEIGHT, 1234)
    a[500:548, 900:948] = 16                   # a patch that turns bright and dark again: every call sees the same one region
    b = a.copy()
    b[500:548, 900:948] = 240
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mi355x.bin")
        engine.save_engine(engine.build_engine(synthetic_weights(1234), robust=True), path)
        dev = HipEngine(path, 0, BATCH, WIDTH, HEIGHT, dev=True)
        launches = {}
        try:
            for name, (C, dilate) in grids.items():
                now, ref = mo.grids_for(C, WIDTH, HEIGHT, THR)
                p = dict(SETTINGS, dilate=dilate)
                found = dev.stage_motion_regions(now, ref, WIDTH, HEIGHT, THR, **p)
                assert found == mo.regions_of(C, WIDTH, HEIGHT, 0, **p), name
                runs = [dev.profile_motion(now, ref, WIDTH, HEIGHT, THR, reps=100, **p) for _ in range(3)]
                launches[name] = dict(changed_cells=int(C.sum()), components=found[2], regions=len(found[0]), rounds=runs[0][3],
                                      regions_us=[round(r[0] * 1e3, 2) for r in runs], activity_us=[round(r[1] * 1e3, 2) for r in runs],
                                      empty_us=[round(r[2] * 1e3, 2) for r in runs], host_scipy_us=host_labelling_us(C, dilate))
        finally:
            dev.close()
        eng = HipEngine(path, 0, BATCH, WIDTH, HEIGHT)
        try:
            ptrs = [eng.upload(a), eng.upload(b)]
            eng.set_camera_motion(0, WIDTH, HEIGHT, THR, whole_frame=True, **SETTINGS)
            for s in range(2):
                eng.submit_motion_device(0, [ptrs[s % 2]], [WIDTH], [HEIGHT], [0], ios=0.6)
                eng.wait(0)
            rects = eng.motion_stats(0)[0][0]
            assert len(rects) == 2, rects

            def motion(s):
                eng.submit_motion_device(0, [ptrs[s % 2]], [WIDTH], [HEIGHT], [0], ios=0.6)

            def tiled(s):
                eng.submit_tiled_device(0, [ptrs[s % 2]], [WIDTH], [HEIGHT], [rects], ios=0.6)

            lone = {"motion": [], "tiled": []}
            for _ in range(args.rounds):
                lone["motion"].append(lone_p50(eng, motion, args.steps))
                assert eng.motion_stats(0)[0][0] == rects
                lone["tiled"].append(lone_p50(eng, tiled, args.steps))
            eng.sync()
        finally:
            eng.close()
    out = dict(metric="motion_regions", grid="%d x %d cells (%dx%d)" % (gw, gh, WIDTH, HEIGHT), threshold=THR, settings=SETTINGS, launches=launches,
               lone_call=dict(rectangles=[list(r) for r in rects], steps=args.steps, motion_p50_ms=lone["motion"], tiled_p50_ms=lone["tiled"],
                              motion_median_ms=float(np.median(lone["motion"])), tiled_median_ms=float(np.median(lone["tiled"]))))
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("tools/motion_bench.py --steps %d --rounds %d on an MI355X: %s, threshold %d, %s, robust -p 16 engine, max_batch %d\n"
                    % (args.steps, args.rounds, out["grid"], THR, SETTINGS, BATCH))
            f.write("  HIP-event time of one launch alone, mean of 100, three measurements (us); the bracket around nothing beside it\n")
            for name, r in launches.items():
                net = float(np.median(r["regions_us"])) - float(np.median(r["empty_us"]))
                f.write("  %-10s (dilate %d) %5d changed cells, %4d components, %d regions, %d labelling rounds: region launch %s, empty bracket %s -> %.2f us above it; "
                        "scipy on a host thread (dilate, label, boxes, counts) %s us\n"
                        % (name, grids[name][1], r["changed_cells"], r["components"], r["regions"], r["rounds"], r["regions_us"], r["empty_us"], net, r["host_scipy_us"]))
            act = [v for r in launches.values() for v in r["activity_us"]]
            f.write("  whole-frame activity launch of a %dx%d RGB24 frame (reads %.1f MB, writes %d bytes): median %.2f us, min %.2f, max %.2f over %d measurements\n"
                    % (WIDTH, HEIGHT, WIDTH * HEIGHT * 3 / 1e6, gw * gh * 2, float(np.median(act)), min(act), max(act), len(act)))
            lc = out["lone_call"]
            f.write("  lone call, frames resident in HBM, the whole frame + one region %s (a batch of two), p50 of %d calls, %d rounds alternating (ms):\n"
                    "    submit_motion_device + wait %s, submit_tiled_device + wait on the same two rectangles %s\n"
                    "    medians %.4f against %.4f ms: finding the rectangle costs %.1f us of a lone call\n"
                    % (list(rects[1]), args.steps, args.rounds, lc["motion_p50_ms"], lc["tiled_p50_ms"], lc["motion_median_ms"], lc["tiled_median_ms"],
                       (lc["motion_median_ms"] - lc["tiled_median_ms"]) * 1e3))
    return 0


if __name__ == "__main__":
    sys.exit(main())
