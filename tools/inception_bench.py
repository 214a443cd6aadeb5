"""Throughput of an SSD-Inception-v2 engine (watsor_amd/inception.py) -- or, with --network mobilenet_v1, of an SSD-MobileNet-v1 one
(watsor_amd/mobilenet_v1.py): 640x480 frames resident in HBM, batch 8, four lanes, the `-p 16` and `-p 32` engines on seeded synthetic
weights -- bench.py's headline workload on the other networks.  Prints one JSON line per precision (and writes them to --out), with
the MACs per frame computed from the program's shapes.  --unfused: the `-p 16` engine with one op per layer (fuse=False; the A/B of
MobileNet-v1's fused separable layers).

    python tools/inception_bench.py [--network inception_v2|mobilenet_v1] [--unfused] [--steps 300] [--warmup 30] [--precision 16 32]
                                    [--out profiles/inception_bench.json]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH, HEIGHT, BATCH, RING = 640, 480, 8, 4


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--precision", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--out", default=None)
    ap.add_argument("--network", choices=["inception_v2", "mobilenet_v1"], default="inception_v2")
    ap.add_argument("--unfused", action="store_true", help="one op per layer (engine.build_engine(fuse=False))")
    args = ap.parse_args(argv)
    import bench
    from watsor_amd import engine, inception, mobilenet_v1
    from watsor_amd.runtime import HipEngine
    from watsor_amd.synth import synthetic_frame, synthetic_inception_v2, synthetic_mobilenet_v1
    if args.network == "mobilenet_v1":
        W, macs, metric = synthetic_mobilenet_v1(1234), mobilenet_v1.macs_per_frame(), "ssd_mobilenet_v1_throughput"
    else:
        W, macs, metric = synthetic_inception_v2(1234), inception.macs_per_frame(), "ssd_inception_v2_throughput"
    lines = []
    for p in args.precision:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "mi355x.bin")
            engine.save_engine(engine.build_engine(W, p, fuse=not args.unfused), path)
            eng = HipEngine(path, 0, BATCH, WIDTH, HEIGHT)
            try:
                dfr = [eng.upload(synthetic_frame(WIDTH, HEIGHT, 1234 + i)) for i in range(RING * BATCH)]
                r = bench.throughput(eng, lambda lane, s: eng.submit_device(lane, dfr[(s % RING) * BATCH:(s % RING + 1) * BATCH],
                                                                            [WIDTH] * BATCH, [HEIGHT] * BATCH),
                                     BATCH, steps=args.steps, warm=args.warmup)
                lanes = eng.num_slots
            finally:
                eng.close()
        if args.unfused:
            r["program"] = "unfused"
        r.update(metric=metric, precision=p, batch=BATCH, lanes=lanes, frame="%dx%d" % (WIDTH, HEIGHT),
                 frames="resident in HBM", macs_per_frame=macs,
                 useful_tflops=round(r["value"] * macs * 2 / 1e12, 2))
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
