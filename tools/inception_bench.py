"""Throughput of an SSD-Inception-v2 engine (watsor_amd/inception.py): 640x480 frames resident in HBM, batch 8, four lanes, the
`-p 16` and `-p 32` engines on seeded synthetic weights -- bench.py's headline workload on the second network.  Prints one JSON
line per precision (and writes them to --out), with the MACs per frame computed from the program's shapes.

    python tools/inception_bench.py [--steps 300] [--warmup 30] [--precision 16 32] [--out profiles/inception_bench.json]"""
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
    args = ap.parse_args(argv)
    import bench
    from watsor_amd import engine, inception
    from watsor_amd.runtime import HipEngine
    from watsor_amd.synth import synthetic_frame, synthetic_inception_v2
    W = synthetic_inception_v2(1234)
    macs = inception.macs_per_frame()
    lines = []
    for p in args.precision:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "mi355x.bin")
            engine.save_engine(engine.build_engine(W, p), path)
            eng = HipEngine(path, 0, BATCH, WIDTH, HEIGHT)
            try:
                dfr = [eng.upload(synthetic_frame(WIDTH, HEIGHT, 1234 + i)) for i in range(RING * BATCH)]
                r = bench.throughput(eng, lambda lane, s: eng.submit_device(lane, dfr[(s % RING) * BATCH:(s % RING + 1) * BATCH],
                                                                            [WIDTH] * BATCH, [HEIGHT] * BATCH),
                                     BATCH, steps=args.steps, warm=args.warmup)
                lanes = eng.num_slots
            finally:
                eng.close()
        r.update(metric="ssd_inception_v2_throughput", precision=p, batch=BATCH, lanes=lanes, frame="%dx%d" % (WIDTH, HEIGHT),
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
