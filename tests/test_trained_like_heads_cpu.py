"""The trained-like class heads (trained_like_heads.py) give the populations the production-tail tests on the GPU rely on, measured on
the fp32 oracle network's head outputs (no GPU): per frame kind the candidates above 0.3, the scores that are exactly 1.0, the range of
the scores, the crowded bin of the dead columns -- and, which decides whether a frame's walk reaches that bin, the NMS survivors above it."""
import numpy as np
import pytest

import parity_utils as pu
import trained_like_heads as H
from oracle import postprocess as post
from watsor_amd import arch
from watsor_amd.synth import synthetic_weights

SEEDS = (0, 1, 2)


@pytest.fixture(scope="module")
def heads():
    """kind -> (box encodings, logits) of the oracle network on the three seeds' frames."""
    from oracle.ssd_mobilenet_v2 import OracleNet
    prog = arch.build(fuse=False)
    net = OracleNet(H.trained_heads(synthetic_weights(1234), prog, 5))
    kinds = {}
    for seed in SEEDS:
        for kind, f in H.frame_kinds(seed).items():
            kinds.setdefault(kind, []).append(f)
    out = {}
    for kind, frames in kinds.items():
        be, lg, _ = pu.oracle_forward_from_half(net, pu.oracle_input_half(frames))
        out[kind] = (be, lg)
    return out


def test_only_the_class_predictors_change():
    prog = arch.build(fuse=False)
    W0 = synthetic_weights(1234)
    W = H.trained_heads(W0, prog, 5)
    changed = sorted(k for k in W0 if not np.array_equal(W0[k], W[k]))
    assert changed == sorted("%s/ClassPredictor/%s" % (op.scope, v) for op in H.head_ops(prog) for v in ("weights", "biases"))
    assert len(H.hot_columns(prog, 5)) == H.HOT and len(set(H.hot_columns(prog, 5))) == H.HOT
    for op in H.head_ops(prog):
        w, b = W[op.scope + "/ClassPredictor/weights"], W[op.scope + "/ClassPredictor/biases"]
        cls = np.arange(w.shape[3]) % H.NUM_COLS
        dead = np.isin(cls, H.DEAD)
        assert not w[..., dead].any() and (b[dead] == np.float32(H.DEAD_BIAS)).all() and w[..., ~dead].any(axis=(0, 1, 2)).all()
        assert (b[cls == 0] > 0).all() and (b[(cls != 0) & ~dead] < 0).all()


@pytest.mark.parametrize("kind", ["noise", "synthetic"])
def test_busy_frames_look_trained(heads, kind):
    for lg in heads[kind][1]:
        p = H.populations(lg)
        print(kind, {k: v for k, v in p.items() if k != "hist"})
        # the band holds for the busy kinds.  The constant frame is the quiet scene BY CONSTRUCTION -- fewer than 100 NMS survivors above
        # the dead columns' bin is what makes its walk reach that bin -- and so lies below it (test_which_frames_walk_down_to_the_dead_bin)
        assert 100 < p["above_03"] < 2000
        assert p["ones"] >= 20
        assert p["smin"] < 1e-6 and p["smax"] > 0.9


def test_dead_columns_crowd_one_bin_in_every_frame(heads):
    for kind, (_, lgs) in heads.items():
        for lg in lgs:
            p = H.populations(lg)
            assert p["top_bin"] == H.dead_bin() and p["top_bin_count"] > H.WZ_CAND_CAP
            assert p["top_bin_count"] >= len(H.DEAD) * lg.shape[0] > 2 * H.WZ_CAND_CAP      # ... and the bit map lists more than twice the list


def test_which_frames_walk_down_to_the_dead_bin(heads):
    """NMS survivors above the dead bin: a noise frame has its 100 rows without it (with a margin the fp16 programs' logit error does
    not eat), a constant frame does not -- it is the dead-column scene: its rows end inside the crowded bin."""
    edge = np.uint32((H.dead_bin() + 1) << 20).view(np.float32)
    for kind, (bes, lgs) in heads.items():
        for be, lg in zip(bes, lgs):
            _, s, _, nd = post.postprocess(be, lg, pu.anchors_cs(), fast=True, max_total=300)
            above = int((s[:nd] >= edge).sum())
            print(kind, "survivors above the dead bin:", above, "candidates above 0.3:", H.populations(lg)["above_03"])
            if kind == "noise":
                assert above >= 125
            elif kind == "constant":
                assert 20 <= above <= 80 and H.populations(lg)["ones"] >= 20 and 20 < H.populations(lg)["above_03"] < 100
                _, s100, _, n100 = post.postprocess(be, lg, pu.anchors_cs(), fast=True)
                assert n100 == 100 and H.score_bins(s100[99:100])[0] == H.dead_bin()
