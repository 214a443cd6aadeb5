"""SSD-Inception-v2 300x300 as an op program for the MI355X engine (the second network family beside arch.py's MobileNet-v2).

The reference's README names `ssd_inception_v2_coco_2018_01_28` as the model of its CPU and GPU plugins next to the two
MobileNets (README.md:446-451).  The topology below is restated from TF-slim's `inception_v2.py`, the Object Detection API's
`ssd_inception_v2_feature_extractor.py` and `ssd_inception_v2_coco.config` AS RECALLED: none of these files was at hand when this
module was written, and no trained checkpoint was either.  What pins it down is the shape check of the importer (every variable
of a frozen graph is compared against `Program.variable_shapes()`, a mismatch refuses the model by name) and the anchor check of
`engine.apply_graph_settings`.

  * Every conv is followed by BatchNorm (eps 1e-3) and ReLU6 (`override_base_feature_extractor_hyperparams`); padding is TF `SAME`.
  * The stem `Conv2d_1a_7x7` is a separable conv: depthwise [7,7,3,8] stride 2, pointwise [1,1,24,64], then BatchNorm and ReLU6.
    The builder folds it into ONE dense 7x7x3x64 kernel (engine.fold_stem7) and runs it as OP_STEM7.
  * Mixed modules have up to four branches joined by a channel concat, in the order B0, B1, B2, B3.  There is no concat op: the
    last op of every branch writes its slice of the module's tensor (Op.coff / Op.cdst).
  * The SSD taps are Mixed_4c (19x19x576) and Mixed_5c (10x10x1024), followed by the extras
    `Mixed_5c_1_Conv2d_{2..5}_1x1_{256,128,128,64}` / `Mixed_5c_2_Conv2d_{2..5}_3x3_s2_{512,256,256,128}` (5, 3, 2, 1) and the same
    six box predictors as MobileNet-v2 (anchors per location 3, 6, 6, 6, 6, 6; 1917 anchors).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

from . import arch
from .arch import (ACT_RELU6, ACT_NONE, NUM_CLASSES, OP_CONV, OP_POOL, OP_STEM7, OUT_ACT, OUT_HEAD, Op, Program, Tensor,
                   tf_same)

FE = "FeatureExtractor/InceptionV2/"
FAMILY = "InceptionV2"

# module -> (B0 depths, B1 depths, B2 depths, B3 depth or None); a tuple of two for B0 means 1x1 -> 3x3 stride 2 (Mixed_4a / 5a)
MODULES: List[Tuple[str, tuple, tuple, tuple, Optional[int], str]] = [
    # name,     B0,          B1,              B2,               B3,   B3 pool
    ("Mixed_3b", (64,),      (64, 64),        (64, 96, 96),     32,   "avg"),
    ("Mixed_3c", (64,),      (64, 96),        (64, 96, 96),     64,   "avg"),
    ("Mixed_4a", (128, 160), (64, 96, 96),    (),               None, "max"),
    ("Mixed_4b", (224,),     (64, 96),        (96, 128, 128),   128,  "avg"),
    ("Mixed_4c", (192,),     (96, 128),       (96, 128, 128),   128,  "avg"),
    ("Mixed_4d", (160,),     (128, 160),      (128, 160, 160),  96,   "avg"),
    ("Mixed_4e", (96,),      (128, 192),      (160, 192, 192),  96,   "avg"),
    ("Mixed_5a", (128, 192), (192, 256, 256), (),               None, "max"),
    ("Mixed_5b", (352,),     (192, 320),      (160, 224, 224),  128,  "avg"),
    ("Mixed_5c", (352,),     (192, 320),      (192, 224, 224),  128,  "max"),
]
EXTRA_DEPTHS = [(256, 512), (128, 256), (128, 256), (64, 128)]
ANCHORS_PER_LOCATION = [3, 6, 6, 6, 6, 6]
TAPS = ("Mixed_4c", "Mixed_5c")


def _conv(scope: str, src: str, dst: str, cin: int, cout: int, k: int, stride: int) -> Op:
    return Op(OP_CONV, FE + scope, src, dst, cin, cout, k, stride, ACT_RELU6, True)


def _module(name: str, b0, b1, b2, b3, pool: str, src: str, cin: int) -> Tuple[List[Op], int]:
    """The ops of one Mixed module in branch order; every branch's last op writes its slice of the tensor `name`."""
    ops: List[Op] = []
    reduction = b3 is None                    # Mixed_4a / Mixed_5a: stride-2 branches and a max pool over the input
    branches: List[List[Op]] = []
    if reduction:
        d0, d1 = b0
        branches.append([_conv(name + "/Branch_0/Conv2d_0a_1x1", src, name + "/Branch_0/Conv2d_0a_1x1", cin, d0, 1, 1),
                         _conv(name + "/Branch_0/Conv2d_1a_3x3", name + "/Branch_0/Conv2d_0a_1x1", name, d0, d1, 3, 2)])
        e0, e1, e2 = b1
        branches.append([_conv(name + "/Branch_1/Conv2d_0a_1x1", src, name + "/Branch_1/Conv2d_0a_1x1", cin, e0, 1, 1),
                         _conv(name + "/Branch_1/Conv2d_0b_3x3", name + "/Branch_1/Conv2d_0a_1x1", name + "/Branch_1/Conv2d_0b_3x3",
                               e0, e1, 3, 1),
                         _conv(name + "/Branch_1/Conv2d_1a_3x3", name + "/Branch_1/Conv2d_0b_3x3", name, e1, e2, 3, 2)])
        mp = Op(OP_POOL, FE + name + "/Branch_2/MaxPool_1a_3x3", src, name, cin, cin, 3, 2, ACT_NONE, False, pool_max=True)
        branches.append([mp])
    else:
        branches.append([_conv(name + "/Branch_0/Conv2d_0a_1x1", src, name, cin, b0[0], 1, 1)])
        d0, d1 = b1
        branches.append([_conv(name + "/Branch_1/Conv2d_0a_1x1", src, name + "/Branch_1/Conv2d_0a_1x1", cin, d0, 1, 1),
                         _conv(name + "/Branch_1/Conv2d_0b_3x3", name + "/Branch_1/Conv2d_0a_1x1", name, d0, d1, 3, 1)])
        e0, e1, e2 = b2
        branches.append([_conv(name + "/Branch_2/Conv2d_0a_1x1", src, name + "/Branch_2/Conv2d_0a_1x1", cin, e0, 1, 1),
                         _conv(name + "/Branch_2/Conv2d_0b_3x3", name + "/Branch_2/Conv2d_0a_1x1", name + "/Branch_2/Conv2d_0b_3x3",
                               e0, e1, 3, 1),
                         _conv(name + "/Branch_2/Conv2d_0c_3x3", name + "/Branch_2/Conv2d_0b_3x3", name, e1, e2, 3, 1)])
        pname = "MaxPool_0a_3x3" if pool == "max" else "AvgPool_0a_3x3"
        pl = Op(OP_POOL, FE + name + "/Branch_3/" + pname, src, name + "/Branch_3/" + pname, cin, cin, 3, 1, ACT_NONE, False,
                pool_max=pool == "max")
        branches.append([pl, _conv(name + "/Branch_3/Conv2d_0b_1x1", pl.dst, name, cin, b3, 1, 1)])
    coff = 0
    for br in branches:
        last = br[-1]
        last.coff = coff
        coff += last.cout
        ops.extend(br)
    for br in branches:
        br[-1].cdst = coff
    return ops, coff


def build(size: int = arch.INPUT_SIZE, input_pair: bool = False, head_ks: Sequence[int] = (3,) * 6) -> Program:
    """The SSD-Inception-v2 program: one op per layer (conv, pool, the folded 7x7 stem), branches written by slice into the module
    tensors, the six SSD heads as one [box | class] conv each (arch.build's OUT_HEAD form).
    input_pair: the network input is stored as a hi + lo pair of halves (the `-p 32` program, as in arch.build).
    head_ks: kernel size of each box predictor (1 or 3; a frozen graph's own weights say which, engine.head_kernel_sizes)."""
    if len(head_ks) != 6 or any(k not in (1, 3) for k in head_ks):
        raise ValueError("box predictor kernel sizes %r: six of 1 or 3 expected" % (tuple(head_ks),))
    p = Program(size=size)
    ops: List[Op] = []
    ops.append(Op(OP_STEM7, FE + "Conv2d_1a_7x7", "input", "Conv2d_1a_7x7", 3, 64, 7, 2, ACT_RELU6, True))
    ops.append(Op(OP_POOL, FE + "MaxPool_2a_3x3", "Conv2d_1a_7x7", "MaxPool_2a_3x3", 64, 64, 3, 2, ACT_NONE, False, pool_max=True))
    ops.append(_conv("Conv2d_2b_1x1", "MaxPool_2a_3x3", "Conv2d_2b_1x1", 64, 64, 1, 1))
    ops.append(_conv("Conv2d_2c_3x3", "Conv2d_2b_1x1", "Conv2d_2c_3x3", 64, 192, 3, 1))
    ops.append(Op(OP_POOL, FE + "MaxPool_3a_3x3", "Conv2d_2c_3x3", "MaxPool_3a_3x3", 192, 192, 3, 2, ACT_NONE, False, pool_max=True))
    cur, cin = "MaxPool_3a_3x3", 192
    for name, b0, b1, b2, b3, pool in MODULES:
        mops, cout = _module(name, b0, b1, b2, b3, pool, cur, cin)
        ops.extend(mops)
        cur, cin = name, cout
    taps = list(TAPS)
    for i, (d1, d2) in enumerate(EXTRA_DEPTHS):
        n1 = "Mixed_5c_1_Conv2d_%d_1x1_%d" % (i + 2, d1)
        n2 = "Mixed_5c_2_Conv2d_%d_3x3_s2_%d" % (i + 2, d2)
        ops.append(_conv(n1, cur, n1, cin, d1, 1, 1))
        ops.append(_conv(n2, n1, n2, d1, d2, 3, 2))
        cur, cin = n2, d2
        taps.append(n2)

    # shape inference; a tensor written by several ops (a module's concat) is declared by the first, checked against the others
    p.tensors["input"] = Tensor("input", size, size, 3, hp=input_pair)
    for op in ops:
        src = p.tensors[op.src]
        if src.c != op.cin and not op.kind == OP_STEM7:
            raise AssertionError("%s reads %d channels of %s, which has %d" % (op.scope, op.cin, op.src, src.c))
        op.hin, op.win = src.h, src.w
        op.hout, op.pad_t = tf_same(op.hin, op.k, op.stride)
        op.wout, op.pad_l = tf_same(op.win, op.k, op.stride)
        c = op.cdst or op.cout
        t = p.tensors.get(op.dst)
        if t is None:
            p.tensors[op.dst] = Tensor(op.dst, op.hout, op.wout, c)
        elif (t.h, t.w, t.c) != (op.hout, op.wout, c):
            raise AssertionError("%s writes a %dx%dx%d slice map into %s (%dx%dx%d)" % (op.scope, op.hout, op.wout, c, op.dst, t.h, t.w, t.c))

    off = 0
    for i, (tname, a, hk) in enumerate(zip(taps, ANCHORS_PER_LOCATION, head_ks)):
        tt = p.tensors[tname]
        op = Op(OP_CONV, "BoxPredictor_%d" % i, tname, "head_%d" % i, tt.c, a * 4 + a * NUM_CLASSES,
                hk, 1, ACT_NONE, False, out_mode=OUT_HEAD, head_index=i, anchors_per_loc=a)
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
    """Multiply-accumulates of one frame, from the program's shapes (the stem as the folded dense 7x7x3x64 conv, pools as none)."""
    prog = prog or build()
    total = 0
    for op in prog.ops:
        if op.kind == OP_POOL:
            continue
        total += op.hout * op.wout * op.cout * op.k * op.k * op.cin
    return total


def tensor_writers(prog: Program) -> Dict[str, List[int]]:
    """tensor -> indices of the ops that write it (a module's concat tensor has one writer per branch)."""
    out: Dict[str, List[int]] = {}
    for i, op in enumerate(prog.ops):
        if op.out_mode == OUT_ACT:
            out.setdefault(op.dst, []).append(i)
    return out
