"""SSD-MobileNet-v1 300x300 as an op program for the MI355X engine (the third network family beside arch.py's MobileNet-v2 and
inception.py's Inception-v2).

The reference's README names `ssd_mobilenet_v1_coco` as the fastest model of its table, and its CPU image ships it.  The topology
below is restated from TF-slim's `mobilenet_v1.py`, the Object Detection API's `ssd_mobilenet_v1_feature_extractor.py` and
`ssd_mobilenet_v1_coco.config` AS RECALLED: none of these files was at hand when this module was written, and no trained checkpoint
was either.  What pins it down is the shape check of the importer (every variable of a frozen graph is compared against
`Program.variable_shapes()`, a mismatch refuses the model by name) and the anchor check of `engine.apply_graph_settings`.

  * `Conv2d_0` is a 3x3 stride-2 conv to 32 channels (the MobileNet-v2 stem, OP_STEM); then thirteen separable layers
    `Conv2d_<i>_depthwise` (depthwise 3x3, [3,3,C,1]) -> `Conv2d_<i>_pointwise` (1x1).  Every conv is followed by BatchNorm
    (eps 1e-3) and ReLU6; padding is TF `SAME`.
  * fuse=True: each separable layer is ONE op (OP_DWSEP, csrc/k_dwsep.hip) carrying its two unfused ops as `parts`; fuse=False keeps
    one op per layer (OP_DW, OP_CONV: the per-tensor tests, the A/B and the `-p 32` engine).
  * The SSD taps are Conv2d_11_pointwise (19x19x512) and Conv2d_13_pointwise (10x10x1024), followed by the extras
    `Conv2d_13_pointwise_1_Conv2d_{2..5}_1x1_{256,128,128,64}` / `Conv2d_13_pointwise_2_Conv2d_{2..5}_3x3_s2_{512,256,256,128}` (5, 3, 2, 1)
    and the same six box predictors as the other two networks (anchors per location 3, 6, 6, 6, 6, 6; 1917 anchors).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

from . import arch
from .arch import ACT_RELU6, NUM_CLASSES, OP_CONV, OP_DW, OP_DWSEP, OP_STEM, OUT_HEAD, Op, Program, Tensor, tf_same

FE = "FeatureExtractor/MobilenetV1/"
FAMILY = "MobilenetV1"

# (stride, output channels) of the separable layers Conv2d_1 .. Conv2d_13, depth multiplier 1.0
SEPARABLE = [(1, 64), (2, 128), (1, 128), (2, 256), (1, 256), (2, 512),
             (1, 512), (1, 512), (1, 512), (1, 512), (1, 512), (2, 1024), (1, 1024)]
EXTRA_DEPTHS = [(256, 512), (128, 256), (128, 256), (64, 128)]
ANCHORS_PER_LOCATION = [3, 6, 6, 6, 6, 6]
TAPS = ("Conv2d_11_pointwise", "Conv2d_13_pointwise")


def _conv(scope: str, src: str, dst: str, cin: int, cout: int, k: int, stride: int) -> Op:
    return Op(OP_CONV, FE + scope, src, dst, cin, cout, k, stride, ACT_RELU6, True)


def build(size: int = arch.INPUT_SIZE, input_pair: bool = False, head_ks: Sequence[int] = (3,) * 6, fuse: bool = True) -> Program:
    """The SSD-MobileNet-v1 program.  fuse=True: every separable layer is one OP_DWSEP (the `-p 16` program); fuse=False: one op per
    layer.  input_pair: the network input is stored as a hi + lo pair of halves (the `-p 32` program, as in arch.build).
    head_ks: kernel size of each box predictor (1 or 3; a frozen graph's own weights say which, engine.head_kernel_sizes)."""
    if len(head_ks) != 6 or any(k not in (1, 3) for k in head_ks):
        raise ValueError("box predictor kernel sizes %r: six of 1 or 3 expected" % (tuple(head_ks),))
    p = Program(size=size)
    ops: List[Op] = [Op(OP_STEM, FE + "Conv2d_0", "input", "Conv2d_0", 3, 32, 3, 2, ACT_RELU6, True)]
    cur, cin = "Conv2d_0", 32
    for i, (s, c) in enumerate(SEPARABLE, start=1):
        dn, pn = "Conv2d_%d_depthwise" % i, "Conv2d_%d_pointwise" % i
        dw = Op(OP_DW, FE + dn, cur, dn, cin, cin, 3, s, ACT_RELU6, True)
        pw = _conv(pn, dn, pn, cin, c, 1, 1)
        if fuse:   # cin = depthwise channels = pointwise K; k / stride / padding are the depthwise conv's
            ops.append(Op(OP_DWSEP, FE + "Conv2d_%d" % i, cur, pn, cin, c, 3, s, ACT_RELU6, True, parts=[dw, pw]))
        else:
            ops += [dw, pw]
        cur, cin = pn, c
    taps = list(TAPS)
    for i, (d1, d2) in enumerate(EXTRA_DEPTHS):
        n1 = "Conv2d_13_pointwise_1_Conv2d_%d_1x1_%d" % (i + 2, d1)
        n2 = "Conv2d_13_pointwise_2_Conv2d_%d_3x3_s2_%d" % (i + 2, d2)
        ops.append(_conv(n1, cur, n1, cin, d1, 1, 1))
        ops.append(_conv(n2, n1, n2, d1, d2, 3, 2))
        cur, cin = n2, d2
        taps.append(n2)

    p.tensors["input"] = Tensor("input", size, size, 3, hp=input_pair)
    for op in ops:
        src = p.tensors[op.src]
        if src.c != op.cin:
            raise AssertionError("%s reads %d channels of %s, which has %d" % (op.scope, op.cin, op.src, src.c))
        op.hin, op.win = src.h, src.w
        op.hout, op.pad_t = tf_same(op.hin, op.k, op.stride)
        op.wout, op.pad_l = tf_same(op.win, op.k, op.stride)
        for part in op.parts or []:                       # the unfused ops of a separable layer: depthwise map, then 1x1
            part.hin, part.win = (op.hin, op.win) if part.kind == OP_DW else (op.hout, op.wout)
            part.hout, part.wout = op.hout, op.wout
            part.pad_t, part.pad_l = (op.pad_t, op.pad_l) if part.kind == OP_DW else (0, 0)
        p.tensors[op.dst] = Tensor(op.dst, op.hout, op.wout, op.cout)

    off = 0
    for i, (tname, a, hk) in enumerate(zip(taps, ANCHORS_PER_LOCATION, head_ks)):
        tt = p.tensors[tname]
        op = Op(OP_CONV, "BoxPredictor_%d" % i, tname, "head_%d" % i, tt.c, a * 4 + a * NUM_CLASSES,
                hk, 1, arch.ACT_NONE, False, out_mode=OUT_HEAD, head_index=i, anchors_per_loc=a)
        op.n_box = a * 4
        op.hin, op.win = tt.h, tt.w
        op.hout, op.pad_t = tf_same(tt.h, hk, 1)
        op.wout, op.pad_l = tf_same(tt.w, hk, 1)
        op.anchor_offset = off
        ops.append(op)
        p.feature_maps.append((tname, tt.h, a))
        off += tt.h * tt.w * a
    p.num_anchors = off
    p.ops = ops
    return p


def macs_per_frame(prog: Optional[Program] = None) -> int:
    """Multiply-accumulates of one frame, from the program's shapes (a separable layer as its depthwise plus its pointwise part)."""
    prog = prog or build()
    total = 0
    for op in prog.ops:
        for part in (op.parts if op.kind == OP_DWSEP else [op]):
            k_in = 1 if part.kind == OP_DW else part.cin
            total += part.hout * part.wout * part.cout * part.k * part.k * k_in
    return total
