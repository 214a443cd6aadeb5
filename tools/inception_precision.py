"""The `-p 16` SSD-Inception-v2 engine emulated on the CPU against the fp32 oracle (tests/inception_v2_oracle.py): fp16 folded
weights, fp16 storage of every tensor the engine stores, fp32 sums, the fp16 input.  Decides which `-p 16` program ships:
max score deviation <= 7e-4 -> the plain fp16 program.  Writes profiles/inception_fp16_emulation.json.

    python tools/inception_precision.py [--frames 4] [--seed 1234]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from inception_v2_oracle import InceptionOracleNet  # noqa: E402
from oracle import preprocess as pre  # noqa: E402
from oracle.postprocess import sigmoid  # noqa: E402
from watsor_amd.synth import synthetic_frame, synthetic_inception_v2  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "inception_fp16_emulation.json"))
    args = ap.parse_args(argv)
    W = synthetic_inception_v2(args.seed)
    frames = [synthetic_frame(640, 480, s) for s in range(1, args.frames + 1)]
    x = np.stack([pre.preprocess(f, 300) for f in frames])
    be, lg, T = InceptionOracleNet(W).forward(x, keep=True)
    be16, lg16, T16 = InceptionOracleNet(W, emulate16=True).forward(x, keep=True)
    dev = float(np.abs(sigmoid(lg) - sigmoid(lg16)).max())
    rec = {
        "what": "-p 16 SSD-Inception-v2 engine emulated on the CPU vs the fp32 oracle",
        "weights": "synthetic_inception_v2:%d" % args.seed, "frames": "synthetic_frame(640, 480, 1 .. %d)" % args.frames,
        "max_score_dev": dev,
        "max_logit_dev": float(np.abs(lg - lg16).max()), "max_box_encoding_dev": float(np.abs(be - be16).max()),
        "tensor_rel_dev": {k: float(np.abs(T[k] - T16[k]).max() / max(np.abs(T[k]).max(), 1e-12))
                           for k in ("Conv2d_1a_7x7", "Mixed_3c", "Mixed_4c", "Mixed_5c")},
        "decision": "plain fp16" if dev <= 7e-4 else ("split weights needed" if dev <= 1e-3 else "not parity-qualified"),
    }
    with open(args.output, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
