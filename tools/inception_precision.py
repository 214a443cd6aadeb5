"""The `-p 16` SSD-Inception-v2 (or SSD-MobileNet-v1) engine emulated on the CPU against the fp32 oracle (tests/inception_v2_oracle.py,
tests/mobilenet_v1_oracle.py): fp16 folded weights, fp16 storage of every tensor the engine stores, fp32 sums, the fp16 input.  Decides
which `-p 16` program ships: max score deviation <= 7e-4 -> the plain fp16 program.  Writes profiles/inception_fp16_emulation.json
(--network mobilenet_v1: profiles/mobilenet_v1_fp16_emulation.json).

    python tools/inception_precision.py [--network inception_v2|mobilenet_v1] [--frames 4] [--seed 1234]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from inception_v2_oracle import InceptionOracleNet  # noqa: E402
from mobilenet_v1_oracle import MobilenetV1OracleNet  # noqa: E402
from oracle import preprocess as pre  # noqa: E402
from oracle.postprocess import sigmoid  # noqa: E402
from watsor_amd.synth import synthetic_frame, synthetic_inception_v2, synthetic_mobilenet_v1  # noqa: E402

# network -> (weights, oracle, tensors reported, engine name, default output)
NETWORKS = {
    "inception_v2": (synthetic_inception_v2, InceptionOracleNet, ("Conv2d_1a_7x7", "Mixed_3c", "Mixed_4c", "Mixed_5c"),
                     "SSD-Inception-v2", "inception_fp16_emulation.json"),
    "mobilenet_v1": (synthetic_mobilenet_v1, MobilenetV1OracleNet,
                     ("Conv2d_0", "Conv2d_1_depthwise", "Conv2d_5_pointwise", "Conv2d_11_pointwise", "Conv2d_13_pointwise"),
                     "SSD-MobileNet-v1", "mobilenet_v1_fp16_emulation.json"),
}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--network", choices=sorted(NETWORKS), default="inception_v2")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("-o", "--output", default=None)
    args = ap.parse_args(argv)
    synth, net, names, title, out_name = NETWORKS[args.network]
    W = synth(args.seed)
    frames = [synthetic_frame(640, 480, s) for s in range(1, args.frames + 1)]
    x = np.stack([pre.preprocess(f, 300) for f in frames])
    be, lg, T = net(W).forward(x, keep=True)
    be16, lg16, T16 = net(W, emulate16=True).forward(x, keep=True)
    dev = float(np.abs(sigmoid(lg) - sigmoid(lg16)).max())
    rec = {
        "what": "-p 16 %s engine emulated on the CPU vs the fp32 oracle" % title,
        "weights": "%s:%d" % (synth.__name__, args.seed), "frames": "synthetic_frame(640, 480, 1 .. %d)" % args.frames,
        "max_score_dev": dev,
        "max_logit_dev": float(np.abs(lg - lg16).max()), "max_box_encoding_dev": float(np.abs(be - be16).max()),
        "tensor_rel_dev": {k: float(np.abs(T[k] - T16[k]).max() / max(np.abs(T[k]).max(), 1e-12)) for k in names},
        "decision": "plain fp16" if dev <= 7e-4 else ("split weights needed" if dev <= 1e-3 else "not parity-qualified"),
    }
    with open(args.output or os.path.join(ROOT, "profiles", out_name), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
