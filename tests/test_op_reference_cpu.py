"""tests/op_reference.py proves itself without a GPU: the chained float64 references against the three fp32 oracles, the walker on a
fake engine with one seeded defect at a time, the fused blocks on an emulator that rounds where the kernels round (three storage
forms, four summation orders, eight structural and three precision defects), and the bound function on fp32 sums in four orders.
The last section does it again on weights spread like a trained checkpoint's (tests/trained_like.py): the generator's properties on
the small program and the three networks, both emulators inside the unchanged bound at up to two decades, every seeded defect named
again, and the defects that need fp16-subnormal operands to show."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import op_reference as R
import parity_utils as pu
import trained_like as TL
from inception_v2_oracle import InceptionOracleNet
from mobilenet_v1_oracle import MobilenetV1OracleNet
from oracle.ssd_mobilenet_v2 import OracleNet
from watsor_amd import arch, inception, mobilenet_v1
from watsor_amd.arch import ACT_NONE, ACT_RELU6, OP_CONV, OP_DW, OP_DWSEP, OP_POOL, OP_STEM, OP_STEM7, OUT_HEAD, Op, Program, Tensor, tf_same
from watsor_amd.synth import synthetic_frame, synthetic_inception_v2, synthetic_mobilenet_v1, synthetic_weights

SEED = 1234


# ---------------------------------------------------------------------------------------------------------------------------------
# against the oracles
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["mobilenet_v2", "inception_v2", "mobilenet_v1"])
def test_float64_network_agrees_with_the_fp32_oracle(family):
    """The references chained with exact=True are a float64 network; tensor by tensor (every tensor the oracle keeps) and on the two
    head outputs it agrees with the independently written fp32 oracle within 1e-4 max|ref| + 1e-5: pads, slices, branch order, head
    column order and the stem fold of the reference are right."""
    prog, W, net = {"mobilenet_v2": (arch.build(fuse=False), synthetic_weights(SEED), OracleNet),
                    "inception_v2": (inception.build(), synthetic_inception_v2(SEED), InceptionOracleNet),
                    "mobilenet_v1": (mobilenet_v1.build(fuse=False), synthetic_mobilenet_v1(SEED), MobilenetV1OracleNet)}[family]
    x = pu.oracle_input_half([synthetic_frame(640, 480, 5000)])
    T, be, lg = R.run_program(prog, W, x.astype(np.float64))
    rbe, rlg, RT = pu.oracle_forward_from_half(net(W), x, keep=True)
    seen = 0
    for name, ref in RT.items():
        if name == "input" or name.startswith(("box_", "cls_")):     # (the MobileNet-v2 oracle keeps its twelve head maps: below)
            continue
        assert name in T, name
        assert T[name].shape == ref.shape, name
        assert np.abs(T[name] - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-5, name
        seen += 1
    # every tensor the oracle keeps: all of the MobileNets' (60, 35), module outputs and trunk of Inception (23 of its 61)
    assert seen == {"mobilenet_v2": 60, "inception_v2": 23, "mobilenet_v1": 35}[family]
    assert family == "inception_v2" or seen == len({op.dst for op in prog.ops if op.out_mode != OUT_HEAD})
    assert np.abs(be - rbe).max() <= 1e-4 * np.abs(rbe).max() + 1e-5
    assert np.abs(lg - rlg).max() <= 1e-4 * np.abs(rlg).max() + 1e-5


def test_fused_programs_chain_to_the_same_network():
    """OP_DWSEP's reference (exact) is the depthwise op then the pointwise op; the robust program's split-weight Conv_1 reads a doubled tensor."""
    W = synthetic_mobilenet_v1(SEED)
    x = pu.oracle_input_half([synthetic_frame(640, 480, 5001)]).astype(np.float64)
    _, be0, lg0 = R.run_program(mobilenet_v1.build(fuse=False), W, x)
    _, be1, lg1 = R.run_program(mobilenet_v1.build(fuse=True), W, x)
    assert np.abs(be0 - be1).max() <= 1e-12 and np.abs(lg0 - lg1).max() <= 1e-12
    op = [o for o in arch.build(hp_upto=arch.HP_ALL_BLOCKS, conv1_split=True).ops if o.split_w][0]
    plain = [o for o in arch.build().ops if o.scope == op.scope][0]
    W2 = synthetic_weights(SEED)
    src = np.random.default_rng(1).uniform(-2, 2, (1, 10, 10, 320)).astype(np.float16).astype(np.float64)
    a = R.reference(op, W2, np.concatenate([src, src], -1), precision=16)
    b = R.reference(plain, W2, src, precision=16)
    scale = np.abs(b.ref).max()
    assert np.abs(a.ref - b.ref).max() < 2e-3 * scale          # the two differ by the fp16 rounding of the weights (2^-11 each) ...
    w64 = R.engine_weights(plain, W2, 16, exact=True)
    c = R.reference(plain, W2, src, precision=16, exact=True)
    assert np.abs(a.ref - c.ref).max() < np.abs(b.ref - c.ref).max() / 100 and w64[0].shape[2] == 320   # ... which the hi + lo halves do not have


# ---------------------------------------------------------------------------------------------------------------------------------
# a small program with every op kind, and a fake engine that computes it with fp32 sums and fp16 stores
# ---------------------------------------------------------------------------------------------------------------------------------
def small_program() -> Program:
    """A few ops of each kind, maps 38 -> 19 -> 10 -> 5 as in the networks: 3x3 and 7x7 stems, depthwise, a linear 1x1 (negative values),
    max pool stride 2, a 1x1 with residual and ReLU6, a module of three branches written by slice (one with an average pool), 3x3
    stride-2 convs over an odd (19) and an even (10) map, a fused separable layer, two heads (3 and 6 anchors)."""
    S = 76
    p = Program(size=S)

    def conv(scope, src, dst, cin, cout, k, s, act=ACT_RELU6, **kw):
        return Op(OP_CONV, scope, src, dst, cin, cout, k, s, act, True, **kw)

    ops = [
        Op(OP_STEM, "stem", "input", "stem", 3, 32, 3, 2, ACT_RELU6, True),
        Op(OP_STEM7, "stem7", "input", "stem7", 3, 64, 7, 2, ACT_RELU6, True),
        Op(OP_DW, "dw", "stem", "dw", 32, 32, 3, 1, ACT_RELU6, True),
        conv("proj", "dw", "proj", 32, 64, 1, 1, ACT_NONE),
        Op(OP_POOL, "maxpool", "proj", "maxpool", 64, 64, 3, 2, ACT_NONE, False, pool_max=True),
        conv("expand", "maxpool", "expand", 64, 96, 1, 1),
        conv("resconv", "expand", "resconv", 96, 64, 1, 1, ACT_RELU6, res="maxpool"),
        conv("mix/b0", "resconv", "mix", 64, 32, 1, 1, coff=0, cdst=160),
        conv("mix/b1a", "resconv", "mix/b1a", 64, 64, 1, 1),
        conv("mix/b1b", "mix/b1a", "mix", 64, 96, 3, 1, coff=32, cdst=160),
        Op(OP_POOL, "mix/avgpool", "resconv", "mix/avgpool", 64, 64, 3, 1, ACT_NONE, False, pool_max=False),
        conv("mix/b3", "mix/avgpool", "mix", 64, 32, 1, 1, coff=128, cdst=160),
        conv("down", "mix", "down", 160, 128, 3, 2),
        conv("e1", "down", "e1", 128, 64, 1, 1),
        conv("e2", "e1", "e2", 64, 128, 3, 2),
    ]
    dw = Op(OP_DW, "sep_depthwise", "down", "sep_depthwise", 128, 128, 3, 1, ACT_RELU6, True)
    pw = conv("sep_pointwise", "sep_depthwise", "sep", 128, 128, 1, 1)
    ops.append(Op(OP_DWSEP, "sep", "down", "sep", 128, 128, 3, 1, ACT_RELU6, True, parts=[dw, pw]))
    p.tensors["input"] = Tensor("input", S, S, 3)
    for op in ops:
        src = p.tensors[op.src]
        op.hin, op.win = src.h, src.w
        op.hout, op.pad_t = tf_same(op.hin, op.k, op.stride)
        op.wout, op.pad_l = tf_same(op.win, op.k, op.stride)
        for part in op.parts or []:
            part.hin, part.win = (op.hin, op.win) if part.kind == OP_DW else (op.hout, op.wout)
            part.hout, part.wout = op.hout, op.wout
            part.pad_t, part.pad_l = (op.pad_t, op.pad_l) if part.kind == OP_DW else (0, 0)
        p.tensors.setdefault(op.dst, Tensor(op.dst, op.hout, op.wout, op.cdst or op.cout))
    off = 0
    for i, (tname, a) in enumerate((("mix", 3), ("e2", 6))):
        tt = p.tensors[tname]
        op = Op(OP_CONV, "BoxPredictor_%d" % i, tname, "head_%d" % i, tt.c, a * 4 + a * arch.NUM_CLASSES, 3, 1, ACT_NONE, False,
                out_mode=OUT_HEAD, head_index=i, anchors_per_loc=a)
        op.n_box = a * 4
        op.hin, op.win = tt.h, tt.w
        op.hout, op.pad_t = tf_same(tt.h, 3, 1)
        op.wout, op.pad_l = tf_same(tt.w, 3, 1)
        op.anchor_offset = off
        ops.append(op)
        off += tt.h * tt.w * a
    p.num_anchors = off
    p.ops = ops
    return p


def small_weights(prog: Program, seed: int = 7):
    rng = np.random.Generator(np.random.PCG64(seed))
    W = {}
    for name, shape in prog.variable_shapes().items():
        leaf = name.rsplit("/", 1)[1]
        if leaf.endswith("weights"):
            fan_in = shape[0] * shape[1] * (1 if leaf == "depthwise_weights" and shape[3] == 1 else shape[2])
            W[name] = (rng.standard_normal(shape) * (1.0 / 7 if name == "stem7/depthwise_weights" else math.sqrt(2.0 / fan_in))).astype(np.float32)
        elif leaf == "gamma":
            W[name] = (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif leaf == "moving_variance":
            W[name] = (0.75 + 0.5 * rng.random(shape)).astype(np.float32)
        elif leaf == "biases":
            W[name] = (0.05 * rng.standard_normal(shape) - (4.6 if "ClassPredictor" in name else 0.0)).astype(np.float32)
        else:                                                    # beta, moving_mean
            W[name] = (0.1 * rng.standard_normal(shape) + (0.2 if leaf == "beta" else 0.0)).astype(np.float32)
    return W


class FakeEngine:
    """The `-p 16` program in torch: fp16 weights, float32 sums (torch's own order), bias, activation, residual, one fp16 rounding per
    stored tensor -- and, on request, ONE defect in the op whose scope is `where`."""

    def __init__(self, prog, weights, defect=None, where=None):
        self.prog, self.W, self.defect, self.where = prog, weights, defect, where
        self.names = ["input"] + list(dict.fromkeys(op.dst for op in prog.ops if op.out_mode != OUT_HEAD))
        self.T = {}

    def tensors(self):
        return [(n, self.prog.tensors[n].h, self.prog.tensors[n].w, 4 if n == "input" else self.prog.tensors[n].c) for n in self.names]

    def stage_read_tensor(self, idx, frame=0):
        return self.T[self.names[idx]][frame]

    def _conv(self, x, w, stride, pad_t, pad_l, groups=1):
        k = w.shape[0]
        _, pb = R._pads(x.shape[1], k, stride, pad_t)
        _, pr = R._pads(x.shape[2], k, stride, pad_l)
        xt = F.pad(torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2), (pad_l, pr, pad_t, pb))
        wt = torch.from_numpy(np.ascontiguousarray(w.astype(np.float32).transpose((2, 3, 0, 1) if groups > 1 else (3, 2, 0, 1))))
        return F.conv2d(xt, wt, None, stride=stride, groups=groups).permute(0, 2, 3, 1).numpy()

    def _dense(self, op, x, res, d, stride=None, pad_t=None, pad_l=None):
        w, b = R.engine_weights(op, self.W, 16)
        b = b.astype(np.float32)
        stride, pad_t, pad_l = (op.stride, op.pad_t, op.pad_l) if stride is None else (stride, pad_t, pad_l)
        hi = np.float32(6.0)
        if d == "k_chunk_dropped":
            w = w.copy()
            w[:, :, -32:, :] = 0
        elif d == "taps_mirrored_x":
            w = w[:, ::-1]
        elif d == "pad_l_off_by_one":
            pad_l += 1
        elif d == "bias_last_column_zero":
            b = b.copy()
            b[-1] = 0
        elif d == "relu6_clamps_at_6.5":
            hi = np.float32(6.5)
        elif d == "subnormal_weights_read_as_zero":
            w = np.where(np.abs(w) < 2.0 ** -14, 0.0, w)
        y = self._conv(x, w, stride, pad_t, pad_l)[:, :op.hout, :op.wout] + b
        if d == "residual_before_activation" and res is not None:
            y, res = y + res.astype(np.float32), None
        if op.act == ACT_RELU6:
            y = np.clip(y, np.float32(0), hi)
        if res is not None:
            y = y + res.astype(np.float32)
        return y

    def stage_forward(self, x_half):
        n = x_half.shape[0]
        T = self.T = {"input": np.asarray(x_half, np.float16)}
        be = np.zeros((n, self.prog.num_anchors, 4), np.float32)
        lg = np.zeros((n, self.prog.num_anchors, arch.NUM_CLASSES), np.float32)
        for op in self.prog.ops:
            d = self.defect if op.scope == self.where else None
            x = T[op.src]
            if op.kind in (OP_STEM, OP_STEM7):
                x = x[..., :3]
            if op.kind == OP_POOL:
                x32 = x.astype(np.float32)
                if op.pool_max:
                    xp = R._padded(x32, 3, op.stride, op.pad_t, op.pad_l, 0.0 if d == "max_pool_pads_with_zero" else -np.inf)
                    y = np.max(np.stack([w for _, _, w in R._windows(xp, 3, op.stride, op.hout, op.wout)]), 0)
                else:
                    xp = R._padded(x32, 3, op.stride, op.pad_t, op.pad_l)
                    s = np.sum(np.stack([w for _, _, w in R._windows(xp, 3, op.stride, op.hout, op.wout)]), 0, dtype=np.float32)
                    taps = R.in_image_taps(op.hin, op.win, 3, op.stride, op.pad_t, op.pad_l)[None, :, :, None]
                    y = s * (np.float32(1.0) / (np.float32(9.0) if d == "avg_pool_divides_by_9" else taps.astype(np.float32)))
            elif op.kind == OP_DW:
                w, b = R.engine_weights(op, self.W, 16)
                y = R.depthwise_fp32_emulated(x, w, b, op.stride, op.pad_t, op.pad_l, op.act)
            elif op.kind == OP_DWSEP:
                dw, pw = op.parts
                w, b = R.engine_weights(dw, self.W, 16)
                mid = R.depthwise_fp32_emulated(x, w, b, op.stride, op.pad_t, op.pad_l, dw.act).astype(np.float16)
                y = self._dense(pw, mid, None, d, 1, 0, 0)
            else:
                y = self._dense(op, x, T[op.res] if op.res else None, d)
            if d == "frames_swapped":
                y = y[::-1]
            if op.out_mode == OUT_HEAD:
                b, c = R.head_rows(op, y)
                if d == "head_class_columns_shifted_one_anchor":
                    c = np.roll(c.reshape(n, -1, op.anchors_per_loc, arch.NUM_CLASSES), 1, axis=2).reshape(c.shape)
                be[:, op.anchor_offset:op.anchor_offset + b.shape[1]] = b
                lg[:, op.anchor_offset:op.anchor_offset + c.shape[1]] = c
            else:
                y16 = y.astype(np.float16)
                if d == "store_flushes_subnormals":
                    y16 = np.where(np.abs(y16) < np.float16(2.0 ** -14), np.float16(0), y16)
                if op.cdst:
                    t = T.setdefault(op.dst, np.zeros(y.shape[:3] + (op.cdst,), np.float16))
                    coff = op.coff + (8 if d == "slice_written_8_channels_late" else 0)
                    t[..., coff:coff + op.cout] = y16
                else:
                    T[op.dst] = y16
        self.be, self.lg = be, lg
        return be, lg


@pytest.fixture(scope="module")
def small():
    prog = small_program()
    W = small_weights(prog)
    x = np.stack([R.noise_input(prog.size, 11, 3.0), R.impulse_input(prog.size, 12), R.noise_input(prog.size, 13, 1.0)])
    return prog, W, x


def test_walker_passes_a_correct_fp32_sum_engine(small):
    prog, W, x = small
    rep = R.walk(FakeEngine(prog, W), prog, W, x)
    print("\n" + rep.summary())
    assert rep.ops_checked == len(prog.ops) and rep.ops_mbconv == 0 and rep.ops_unchecked == 0
    assert set(rep.worst) >= {"stem3x3", "stem7x7", "depthwise", "pool_max", "pool_avg", "dwsep", "head3x3", "conv1x1_res", "conv3x3_s2", "conv3x3_slice"}
    assert max(v[0] for v in rep.worst.values()) <= 1.0
    assert rep.elements == sum(op.hout * op.wout * op.cout for op in prog.ops) * x.shape[0]
    # the subset of frames the GPU test uses at batch 16 and 21 still covers everything
    rep = R.walk(FakeEngine(prog, W), prog, W, x, frames=[0, 2])
    assert rep.ops_checked == len(prog.ops)


# defect -> (op it is put into, does the end-to-end tests' bound 0.04 * scale + 0.02 on the defective tensor let it through?)
DEFECTS = {
    "avg_pool_divides_by_9":                 ("mix/avgpool", False),
    "max_pool_pads_with_zero":               ("maxpool", False),
    "k_chunk_dropped":                       ("mix/b1b", False),
    "taps_mirrored_x":                       ("down", False),
    "pad_l_off_by_one":                      ("e2", False),
    "slice_written_8_channels_late":         ("mix/b0", False),
    "residual_before_activation":            ("resconv", False),
    "relu6_clamps_at_6.5":                   ("expand", False),
    "bias_last_column_zero":                 ("e1", True),
    "frames_swapped":                        ("mix/b1a", False),
    "head_class_columns_shifted_one_anchor": ("BoxPredictor_1", False),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_walker_names_the_op_of_every_seeded_defect(small, defect):
    """One defect at a time in the fake engine: the walker fails and names the op.  Beside it, the bound of the end-to-end tests
    (max|got - ref| <= 0.04 max|ref| + 0.02, `ref` = the defect-free tensor; 0.05 on the class logits) on the same defective tensor:

defect                                   op               walker    0.04 * scale + 0.02
        avg pool divides by 9 everywhere         mix/avgpool      fails     fails
        max pool pads with 0 (negative values)   maxpool          fails     fails
        last 32-channel K chunk dropped          mix/b1b          fails     fails
        3x3 taps mirrored in x                   down             fails     fails
        pad_l off by one, stride 2, even map     e2               fails     fails
        slice written at coff + 8                mix/b0           fails     fails
        residual added before the activation     resconv          fails     fails
        ReLU6 clamps at 6.5                      expand           fails     fails
        bias of column cout - 1 zeroed           e1               fails     PASSES
        frames 0 and 1 swapped in one op         mix/b1a          fails     fails
        class columns shifted by one anchor      BoxPredictor_1   fails     fails

    Applied to the very tensor the defect corrupts, with the defect-free tensor as reference and inputs that fill the ReLU6 range, the old
    bound sees ten of the eleven (it misses the zeroed bias: one column off by 0.04 where 0.26 is allowed).  That is not how it is used:
    the end-to-end tests apply it to tensors that carry the rounding of every layer in front, compare with an fp32 oracle, and never look
    at 38 of Inception's 61 tensors.  What the walker adds is the margin and the address: every defect above is outside the op's own bound by a factor of more than 200
    (ReLU6 at 6.5: 249, the zeroed bias: 337, the others 2e3 .. 9e4 or an exact comparison), in the op that has it and in no other."""
    prog, W, x = small
    where, old_bound_lets_through = DEFECTS[defect]
    bad = FakeEngine(prog, W, defect, where)
    with pytest.raises(AssertionError) as ei:
        R.walk(bad, prog, W, x)
    msg = str(ei.value)
    assert "(%s," % where in msg, msg
    first = [ln for ln in msg.splitlines()[1:] if "coverage" not in ln][0]
    assert "(%s," % where in first, msg                          # the first failing op is the defective one, not a consumer
    good = FakeEngine(prog, W)
    good.stage_forward(x)
    op = [o for o in prog.ops if o.scope == where][0]
    if op.out_mode == OUT_HEAD:
        passes = bool(np.abs(bad.lg - good.lg).max() <= 0.05 and np.abs(bad.be - good.be).max() <= 0.04)
    else:
        passes = R.old_bound_passes(bad.T[op.dst], good.T[op.dst])
    print("\n%s in %s: walker fails; 0.04 * scale + 0.02 %s" % (defect, where, "PASSES" if passes else "fails"))
    assert passes == old_bound_lets_through


def test_only_the_defective_op_fails(small):
    """Op-local: downstream ops read what the defective op stored, so they stay inside their bounds."""
    prog, W, x = small
    with pytest.raises(AssertionError) as ei:
        R.walk(FakeEngine(prog, W, "taps_mirrored_x", "mix/b1b"), prog, W, x)
    assert str(ei.value).startswith("1 failure(s)") and "(mix/b1b," in str(ei.value)


def test_walker_counts_what_is_left_out(small):
    """An op missing from the program the walker is given leaves channels uncovered: the coverage count fails."""
    prog, W, x = small
    short = small_program()
    short.ops = [o for o in short.ops if o.scope != "mix/b3"]
    with pytest.raises(AssertionError, match="coverage: tensor mix"):
        R.walk(FakeEngine(prog, W), short, W, x)
    short = small_program()
    short.ops = [o for o in short.ops if o.scope != "BoxPredictor_0"]
    with pytest.raises(AssertionError, match="coverage: head rows"):
        R.walk(FakeEngine(prog, W), short, W, x)


# ---------------------------------------------------------------------------------------------------------------------------------
# fused blocks: a four-block program in the three storage forms, and an emulator that rounds where the kernels round
# ---------------------------------------------------------------------------------------------------------------------------------
ORDERS = ("sequential", "reversed", "pairwise", "chunks32")
F32 = np.float32


def block_program(hp: bool, dup: bool = False) -> Program:
    """Four fused blocks on maps 38 -> 19 -> 10 -> 5: the stem block (3 -> 32 -> 16, 19x19, odd), a stride-2 block with an expand stage
    (16 -> 96 -> 24, onto the even 10x10 map: the padding is bottom / right only), a residual block (24 -> 144 -> 24) and a stride-2
    block that also stores its expanded tensor (24 -> 144 -> 32, `dst2`, as block 13 does).  hp: split-operand blocks between pair
    tensors, the last output one fp16 -- or, dup, [hi | hi]; else plain fp16 blocks."""
    S = 38
    p = Program(size=S)
    p.tensors["input"] = Tensor("input", S, S, 3, hp=hp)
    ops = []

    def block(i, src, cin, mid, cout, stride, stem=False, res=None, dst2=None):
        name = "b%d" % i
        parts = [Op(OP_STEM, name + "/stem", src, name + "/stem", 3, mid, 3, 2, ACT_RELU6, True) if stem else
                 Op(OP_CONV, name + "/expand", src, name + "/expand", cin, mid, 1, 1, ACT_RELU6, True),
                 Op(OP_DW, name + "/depthwise", name + "/expand", name + "/depthwise", mid, mid, 3, stride, ACT_RELU6, True),
                 Op(OP_CONV, name + "/project", name + "/depthwise", name + "/output", mid, cout, 1, 1, ACT_NONE, True, res=res)]
        ops.append(Op(arch.OP_MBCONV, name, src, name + "/output", mid, cout, 3, stride, ACT_NONE, True, res=res, cmid=mid,
                      cin0=mid if stem else cin, parts=parts, stem=stem, block=i, hp=hp, dst2=dst2))
        return name + "/output"

    t = block(0, "input", 3, 32, 16, 1, stem=True)
    t = block(1, t, 16, 96, 24, 2)
    t = block(2, t, 24, 144, 24, 1, res=t)
    block(3, t, 24, 144, 32, 2, dst2="b3/expand")
    ops[-1].dup_out = dup
    for op in ops:
        src = p.tensors[op.src]
        op.hin, op.win = src.h, src.w
        if op.stem:
            op.hin, st = tf_same(src.h, 3, 2)
            op.win, sl = tf_same(src.w, 3, 2)
            op.stem_pad = (st, sl)
        op.hout, op.pad_t = tf_same(op.hin, 3, op.stride)
        op.wout, op.pad_l = tf_same(op.win, 3, op.stride)
        p.tensors[op.dst] = Tensor(op.dst, op.hout, op.wout, 2 * op.cout if op.dup_out else op.cout, hp=hp and op is not ops[-1])
        if op.dst2:
            p.tensors[op.dst2] = Tensor(op.dst2, op.hin, op.win, op.cmid)
    p.ops = ops
    return p


def _enc_unorm16(d):
    """The unorm16 pack: clamp to [0, 1], times 65535 in fp32, to the nearest integer."""
    return np.rint(np.clip(d, F32(0), F32(1)) * F32(65535.0)).astype(np.uint16)


def _enc_float(d):
    """wz_hp_fenc4: t = clamp(d, 0, 1) * T in fp32 (fp32 subnormals kept), half of the kept ulp added to the pattern, bits 10 .. 25."""
    t = (np.clip(d, F32(0), F32(1)) * F32(R.engine.FLOAT_FORM_T)).astype(F32)
    return ((t.view(np.uint32) + np.uint32(512)) >> np.uint32(10)).astype(np.uint16)


def _dec_float(code):
    return (code.astype(np.uint32) << np.uint32(10)).view(F32)


def _split16(v):
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(F32)).astype(F32).astype(np.float16)


def _gemm_f32(first, groups, order):
    """fp32 sum, in `order`, of `first` [..., cout] (or None) and, channel by channel, the products a [..., K] x w [K, cout] of every
    (a, w) in `groups` (all fp16 values: the products are exact in fp32) -- term order: the groups one after the other, as the kernels
    issue their three MFMA terms."""
    cout = groups[0][1].shape[1]
    lead = groups[0][0].shape[:-1]
    cols = [] if first is None else [np.broadcast_to(first.astype(np.float64), lead + (cout,))[..., None]]
    for a, w in groups:
        cols.append(np.einsum("...k,ko->...ok", a.astype(np.float64), w))
    terms = np.concatenate(cols, axis=-1)
    t32 = terms.astype(F32)
    assert (t32.astype(np.float64) == terms).all()
    return _sum_f32(t32.reshape(-1, t32.shape[-1]), order).reshape(lead + (cout,))


class BlockEngine(FakeEngine):
    """The fake engine for programs of fused blocks: every stage of a block in float32 sums of the given order, every stored value
    rounded where the kernels round it (the chunk buffer's codes as wz_hp_fenc4 and the unorm16 pack produce them, hi + lo halves, fp16),
    pair tensors kept as their two fp16 planes.  `defect` in the block whose scope is `where`."""

    def __init__(self, prog, weights, float_form_upto=-1, order="sequential", defect=None, where=None):
        super().__init__(prog, weights, defect, where)
        self.ffu, self.order = float_form_upto, order
        self.names = ["input"] + [t for op in prog.ops for t in (op.dst, op.dst2) if t]

    def tensors(self):
        return [(n, self.prog.tensors[n].h, self.prog.tensors[n].w, 4 if n == "input" else self.prog.tensors[n].c) for n in self.names]

    def stage_read_tensor(self, idx, frame=0, halves=False):
        t = self.T[self.names[idx]]
        if isinstance(t, tuple):
            hi, lo = t[0][frame], t[1][frame]
            return (hi, lo) if halves else hi.astype(F32) + lo.astype(F32)
        return (t[frame], None) if halves else t[frame]

    def stage_forward(self, x_half):
        x = np.asarray(x_half, np.float16)
        self.T = {"input": (x, np.zeros_like(x)) if self.prog.tensors["input"].hp else x}
        for op in self.prog.ops:
            assert op.kind == arch.OP_MBCONV
            self._block(op, self.defect if op.scope == self.where else None)
        n = x.shape[0]
        return np.zeros((n, 0, 4), F32), np.zeros((n, 0, arch.NUM_CLASSES), F32)

    def _halves(self, name):
        t = self.T[name]
        return t if isinstance(t, tuple) else (t, np.zeros_like(t))

    def _block(self, op, d):
        form = R.chunk_form(op, self.ffu)
        bw = R.block_weights(op, self.W, form)
        hp, order = op.hp, self.order
        xh, xl = self._halves(op.src)
        n = xh.shape[0]
        # ---- expand (the stem block: the 27 taps x channels of the stem conv gathered per pixel), fp32, the bias first
        if op.stem:
            st, sl = op.stem_pad
            gather = lambda a: np.concatenate([w for _, _, w in R._windows(R._padded(a[..., :3].astype(np.float64), 3, 2, st, sl), 3, 2, op.hin, op.win)], -1)
            xh, xl = gather(xh), gather(xl)
            whi, wlo = bw["e_hi"].reshape(27, -1), bw["e_lo"].reshape(27, -1)
        else:
            whi, wlo = bw["e_hi"][0, 0], bw["e_lo"][0, 0]
        if d == "wlo_subnormals_read_as_zero":                                      # ... in both GEMMs of the block
            wlo = np.where(np.abs(wlo) < 2.0 ** -14, 0.0, wlo)
        terms = [(xh, wlo), (xl, whi), (xh, whi)] if hp else [(xh, whi)]
        dpre = _gemm_f32(bw["e_b"], terms, order)                                   # [n, hin, win, cmid] float32
        top = F32(1) if hp else F32(6)
        zc = np.clip(dpre, F32(0), top)
        # ---- the chunk buffer: codes (or fp16 values), zero outside the frame
        enc = {R.FORM_FP16: lambda v: v.astype(np.float16), R.FORM_UNORM16: _enc_unorm16, R.FORM_FLOAT: _enc_float}[form]
        code = enc(zc if form == R.FORM_FP16 else dpre)
        dst2 = None
        if op.dst2:
            dst2 = (zc if d == "dst2_stores_the_clamped_value" or not hp else F32(6) * zc).astype(np.float16)
        wd = np.asarray(self._tap_weights(op, form), np.float64)                   # [3,3,cmid]: what the kernel multiplies the decoded code by
        if d == "float_code_decoded_linearly":
            x = code.astype(np.float64) * (R.engine.FLOAT_FORM_T / 65535.0)        # (the linear scale, brought to the float form's units)
        else:
            x = (_dec_float(code) if form == R.FORM_FLOAT else code).astype(np.float64)
        s, pt, pl = op.stride, op.pad_t, op.pad_l

        def padded(pad_t, fill=None):
            xp = R._padded(x, 3, s, pad_t, pl)
            if fill is not None:                                                     # the out-of-frame pixels hold `fill` [cmid]
                m = R._padded(np.ones(x.shape[:3] + (1,)), 3, s, pad_t, pl)
                xp = np.where(m > 0, xp, fill)
            return xp

        def depthwise(xp):
            taps = list(R._windows(xp, 3, s, op.hout, op.wout))
            if order in ("reversed", "pairwise"):
                taps = taps[::-1]
            acc = np.zeros((n, op.hout, op.wout, op.cmid), F32) if form == R.FORM_FLOAT else \
                np.broadcast_to(bw["d_b"].astype(F32), (n, op.hout, op.wout, op.cmid)).copy()
            for ky, kx, win in taps:
                acc = (acc.astype(np.float64) + win[:, :op.hout, :op.wout] * wd[ky, kx]).astype(F32)      # one fused multiply-add
            if form == R.FORM_FLOAT:
                acc = (acc.astype(np.float64) * 2.0 ** 60 + bw["d_b"]).astype(F32)
            return np.clip(acc, F32(0), F32(6))

        if d == "halo_column_off_by_one_right_edge":                                # the in-frame test reads ix < win - 1
            x = x.copy()
            x[:, :, -1, :] = 0
        y = depthwise(padded(pt + 1 if d == "pad_t_off_by_one" else pt))
        if d == "halo_holds_relu6_bias":                                            # ... in the top-left corner tile
            b_code = enc(np.clip(bw["e_b"].astype(F32), F32(0), top) if form == R.FORM_FP16 else bw["e_b"].astype(F32))
            fill = (_dec_float(b_code) if form == R.FORM_FLOAT else b_code).astype(np.float64)
            y[:, :4, :4] = depthwise(padded(pt, fill))[:, :4, :4]
        # ---- what feeds the project GEMM, the sum over the expanded channels, bias, residual, store
        if hp:
            yh, yl = _split16(y)
            whi, wlo = bw["p_hi"], bw["p_lo"]
            if d == "wlo_subnormals_read_as_zero":
                wlo = np.where(np.abs(wlo) < 2.0 ** -14, 0.0, wlo)
            terms = [(yh, wlo), (yl, whi), (yh, whi)]
            if d == "wlo_xhi_dropped":
                terms = terms[1:]
        else:
            yh = y.astype(np.float16)
            terms = [(yh, bw["p_hi"])]
        acc = _gemm_f32(None, terms, order)
        if d == "chunk_missing_at_one_pixel":                                       # channels 32 .. 63 of pixel (1, 2) of frame 0
            keep = [(a[0, 1, 2][None, None, None, np.r_[0:32, 64:op.cmid]], w[np.r_[0:32, 64:op.cmid]]) for a, w in terms]
            acc[0, 1, 2] = _gemm_f32(None, keep, order)[0, 0, 0]
        acc = acc + bw["p_b"].astype(F32)
        if op.res:
            rh, rl = self._halves(op.res)
            if d == "residual_of_the_neighbouring_pixel":
                rh, rl = np.roll(rh, 1, axis=2), np.roll(rl, 1, axis=2)
            if d == "residual_lo_ignored":
                rl = np.zeros_like(rl)
            acc = acc + (rh.astype(F32) + rl.astype(F32))
        if d == "tiles_of_two_frames_swapped":
            acc[[0, 1], :4, :4] = acc[[1, 0], :4, :4]
        oh, ol = _split16(acc)
        if d == "output_lo_zeroed_in_one_tile":
            ol[0, 4:8, 4:8] = 0
        if d == "pair_store_flushes_subnormals":
            oh = np.where(np.abs(oh) < np.float16(2.0 ** -14), np.float16(0), oh)
            ol = np.where(np.abs(ol) < np.float16(2.0 ** -14), np.float16(0), ol)
        if self.prog.tensors[op.dst].hp:
            self.T[op.dst] = (oh, ol)
        else:
            self.T[op.dst] = np.concatenate([oh, oh], -1) if op.dup_out else oh
        if op.dst2:
            self.T[op.dst2] = dst2

    def _tap_weights(self, op, form):
        """fp16 taps (plain), fp32(w * 6 / 65535) (the code is 0 .. 65535), fp32(w * 6 * 2^60 / (2 - 2^-13)) (the code's float)."""
        wd, _ = R.engine.fold_batch_norm(self.W, op.parts[1])
        wd = wd[..., 0]
        if form == R.FORM_FP16:
            return R._f16(wd)
        return R._f32(wd / R.engine.UNORM16_PER_6) if form == R.FORM_UNORM16 else R._f32(wd * R.engine.FLOAT_FORM_TAP_SCALE)


FORMS = {"float_form": dict(hp=True, ffu=99), "unorm16": dict(hp=True, ffu=-1, dup=True), "plain_fp16": dict(hp=False, ffu=-1)}


@pytest.fixture(scope="module")
def blocks():
    """form -> (program, weights, float_form_upto); inputs as the GPU conformance batches mix them: noise of amplitude 4, impulses,
    zeros, noise of amplitude 1."""
    out = {}
    for form, kw in FORMS.items():
        prog = block_program(kw["hp"], kw.get("dup", False))
        out[form] = (prog, small_weights(prog, 21), kw["ffu"])
    S = out["unorm16"][0].size
    x = np.stack([R.noise_input(S, 31), R.impulse_input(S, 32), np.zeros((S, S, 4), np.float16), R.noise_input(S, 33, 1.0)])
    return out, x


@pytest.mark.parametrize("form", sorted(FORMS))
def test_walker_passes_the_block_emulator_in_every_order(blocks, form):
    """The emulator rounds at every point the derivation lists and sums in fp32 in four orders: inside the tolerance in all of them,
    with the exact properties of the stored pairs (and the lo-half-alive rule) holding on these inputs.  Prints the worst share."""
    progs, x = blocks
    prog, W, ffu = progs[form]
    worst = {}
    for order in ORDERS:
        rep = R.walk(BlockEngine(prog, W, ffu, order), prog, W, x, float_form_upto=ffu, check=False)
        assert not rep.failures, (order, rep.failures[:5])
        assert rep.ops_checked == rep.blocks_checked == len(prog.ops) == 4 and rep.ops_unchecked == 0
        assert "block13_expand" in rep.worst
        for k, v in rep.worst.items():
            worst[k] = max(worst.get(k, 0.0), v[0])
    print("\n%s: worst err / tol over four orders: %s" % (form, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) < 1.0
    assert set(worst) >= ({"block_plain"} if form == "plain_fp16" else {"block_hp_q"} if form == "float_form" else {"block_hp", "block_hp2"})


class RanBefore(BlockEngine):
    """An engine whose batch was run before the walk (tests/test_gpu_production_walk.py): the input pair holds the lo half it was
    given.  ignore_lo: the first block computes from the hi half alone, the stored input keeps its lo."""

    def run(self, hi, lo, ignore_lo=False):
        self.T = {"input": (hi, np.zeros_like(lo) if ignore_lo else lo)}
        for op in self.prog.ops:
            self._block(op, None)
            self.T["input"] = (hi, lo)
        n = hi.shape[0]
        return np.zeros((n, 0, 4), F32), np.zeros((n, 0, arch.NUM_CLASSES), F32)

    def stage_forward(self, x_half):
        raise AssertionError("the walker ran a batch of its own")


@pytest.mark.parametrize("form", ["float_form", "unorm16"])
def test_walker_takes_a_batch_that_ran_before_it_and_its_lo_half(blocks, form):
    """heads=(box_enc, logits): no stage_forward, the first block's reference from the stored halves.  With a lo half of order one
    an engine that ignores it is named; with the lo half a resize stores (2^-12 of the input) ignoring it stays inside the first
    block's bound on this program -- what tests/test_gpu_input_lo.py exists for."""
    progs, x = blocks
    prog, W, ffu = progs[form]
    assert prog.tensors["input"].hp
    rng = np.random.Generator(np.random.PCG64(41))
    v = np.zeros(x.shape, F32)
    v[..., :3] = rng.uniform(-1, 1, x.shape[:3] + (3,)).astype(F32)
    hi = v.astype(np.float16)
    small = (v - hi.astype(F32)).astype(np.float16)
    assert (small[..., :3] != 0).mean() > 0.9
    for lo, flagged in ((R.noise_input(prog.size, 43, 1.0)[None].repeat(x.shape[0], 0), True), (small, None)):
        for ignore in (False, True):
            e = RanBefore(prog, W, ffu, "chunks32")
            heads = e.run(hi, lo, ignore)
            rep = R.walk(e, prog, W, None, float_form_upto=ffu, check=False, heads=heads)
            assert rep.ops_checked == len(prog.ops) and rep.ops_unchecked == 0
            if not ignore:
                assert not rep.failures, rep.failures[:3]
            elif flagged:
                assert rep.failures and all("(b0," in f for f in rep.failures), rep.failures[:3]
            else:
                print("\n%s: the lo half of a resize ignored by block 0: %d failure(s), worst err / tol %.3g"
                      % (form, len(rep.failures), max(v_[0] for v_ in rep.worst.values())))
    with pytest.raises(AssertionError):
        R.walk(e, prog, W, None, float_form_upto=ffu, heads=(heads[0], heads[1][:1]))


# defect -> (block it is put into, the forms it exists in)
STRUCTURAL = {
    "halo_holds_relu6_bias":              ("b2", sorted(FORMS)),
    "halo_column_off_by_one_right_edge":  ("b2", sorted(FORMS)),
    "pad_t_off_by_one":                   ("b1", sorted(FORMS)),
    "chunk_missing_at_one_pixel":         ("b2", sorted(FORMS)),
    "float_code_decoded_linearly":        ("b1", ["float_form"]),
    "residual_of_the_neighbouring_pixel": ("b2", sorted(FORMS)),
    "tiles_of_two_frames_swapped":        ("b0", sorted(FORMS)),
    "dst2_stores_the_clamped_value":      ("b3", ["float_form", "unorm16"]),
}
STRUCTURAL_CASES = [(d, f) for d, (_, forms) in sorted(STRUCTURAL.items()) for f in forms]


def _factor(msg):
    """The largest err / tol a walker message names."""
    import re
    return max(float(v) for v in re.findall(r"err / tol ([0-9.e+\-inf]+)", msg))


@pytest.mark.parametrize("defect,form", STRUCTURAL_CASES, ids=["%s-%s" % c for c in STRUCTURAL_CASES])
def test_walker_names_the_block_of_every_structural_defect(blocks, defect, form):
    """One structural defect at a time in the block emulator: the walker fails, in that block and in no other.  The defects: an
    out-of-frame halo pixel holding relu6(bias) in one corner tile; the halo's last in-frame column taken for padding; pad_t off by one
    on a stride-2 block; one 32-channel chunk of one pixel missing from the project sum; the float-form code decoded with the linear
    scale; the residual of the neighbouring pixel; one 4 x 4 tile swapped between two frames; block 13's second output stored as the
    clamped z in [0, 1] without its factor 6."""
    progs, x = blocks
    prog, W, ffu = progs[form]
    where = STRUCTURAL[defect][0]
    with pytest.raises(AssertionError) as ei:
        R.walk(BlockEngine(prog, W, ffu, "chunks32", defect, where), prog, W, x, float_form_upto=ffu)
    lines = str(ei.value).splitlines()[1:]
    assert lines and all("(%s," % where in ln for ln in lines), lines
    print("\n%s in %s (%s): outside by a factor of %.3g" % (defect, where, form, _factor(str(ei.value))))


PRECISION = {"wlo_xhi_dropped": "b2", "residual_lo_ignored": "b2", "output_lo_zeroed_in_one_tile": "b1"}


@pytest.mark.parametrize("defect", sorted(PRECISION))
def test_precision_defects_are_reported(blocks, defect):
    """Defects of 2^-12 relative size, in the split-operand program with the linear buffer.  Their factors are printed, not asserted:
    the tolerance is derived from the formats, and what of a lost lo half it can see is a measurement.  The exception is the output
    whose lo half is zero in one tile: the lo-half-alive rule must name it."""
    progs, x = blocks
    prog, W, ffu = progs["unorm16"]
    where = PRECISION[defect]
    good = R.walk(BlockEngine(prog, W, ffu, "chunks32"), prog, W, x, float_form_upto=ffu, check=False)
    rep = R.walk(BlockEngine(prog, W, ffu, "chunks32", defect, where), prog, W, x, float_form_upto=ffu, check=False)
    kind = R.op_kind_name([o for o in prog.ops if o.scope == where][0], ffu)
    tol_fail = [f for f in rep.failures if "err / tol" in f]
    print("\n%s in %s: worst err / tol %.3g (without the defect %.3g); bound %s, exact checks %s"
          % (defect, where, rep.worst[kind][0], good.worst[kind][0], "FAILS" if tol_fail else "passes",
             "FAIL" if len(rep.failures) > len(tol_fail) else "pass"))
    if defect == "output_lo_zeroed_in_one_tile":
        assert any("lo half dead" in f and "(%s," % where in f for f in rep.failures), rep.failures
    assert all("(%s," % where in f for f in rep.failures), rep.failures


def test_pair_checks():
    rng = np.random.Generator(np.random.PCG64(5))
    v = rng.uniform(-6, 6, (2, 8, 8, 32)).astype(F32)
    hi, lo = _split16(v)
    assert R.pair_checks(hi, lo) == []
    bad = lo.copy()
    bad[0, 0, 0, 0] = np.float16(0.25)
    assert any("|lo| >" in m for m in R.pair_checks(hi, bad))
    dead = lo.copy()
    dead[1, 4:8, 0:4, 16:32] = 0
    assert any("lo half dead" in m for m in R.pair_checks(hi, dead))
    hi2 = hi.copy()
    hi2[0, 1, 1, 1] = np.inf
    assert any("finite" in m for m in R.pair_checks(hi2, lo))
    assert R.pair_store_radius(1.0) == 2.0 ** -22 and R.float_form_step(0.0) < 2.0 ** -19.9


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound function
# ---------------------------------------------------------------------------------------------------------------------------------
def _sum_f32(terms, order):
    """terms [sums, K] float32 -> fp32 sums in the given order."""
    n, K = terms.shape
    if order == "reversed":
        return _sum_f32(terms[:, ::-1], "sequential")
    if order == "sequential":
        acc = np.zeros(n, np.float32)
        for k in range(K):
            acc = acc + terms[:, k]
        return acc
    if order == "chunks32":                      # 32 terms at a time into one accumulator (the MFMA's shape), chunk sums exact
        acc = np.zeros(n, np.float32)
        for k in range(0, K, 32):
            acc = (acc.astype(np.float64) + terms[:, k:k + 32].astype(np.float64).sum(1)).astype(np.float32)
        return acc
    t = terms
    while t.shape[1] > 1:                        # pairwise
        if t.shape[1] % 2:
            t = np.concatenate([t, np.zeros((n, 1), np.float32)], 1)
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]


@pytest.mark.parametrize("K", [9, 27, 288, 1152, 2880, 11520])
def test_fp32_sums_in_any_order_stay_inside_the_bound(K):
    """ReLU6-like activations x He-scaled fp16 weights (exact products), summed in fp32 in sequential, reversed, pairwise and 32-chunk
    order: inside tol, fp32 and fp16 store; a sum that drops one 32-term chunk is outside e_acc in most cases."""
    rng = np.random.Generator(np.random.PCG64(K))
    n = 400
    x = np.clip(rng.standard_normal((n, K)) * 1.5 + 0.5, 0, 6).astype(np.float16).astype(np.float64)
    w = (rng.standard_normal((n, K)) * math.sqrt(2.0 / K)).astype(np.float16).astype(np.float64)
    prod = x * w
    terms = prod.astype(np.float32)
    assert (terms.astype(np.float64) == prod).all()             # fp16 x fp16 is exact in fp32
    ref, T, r = prod.sum(1), np.abs(prod).sum(1), K + 2
    worst = 0.0
    for order in ("sequential", "reversed", "pairwise", "chunks32"):
        got = _sum_f32(terms, order)
        assert (np.abs(got.astype(np.float64) - ref) <= R.tolerance(ref, T, r, False)).all(), order
        assert (np.abs(got.astype(np.float16).astype(np.float64) - ref) <= R.tolerance(ref, T, r, True)).all(), order
        worst = max(worst, float((np.abs(got.astype(np.float64) - ref) / R.e_acc(T, r)).max()))
    print("\nK = %d: worst err / e_acc over four orders: %.3f" % (K, worst))
    assert worst < 0.5
    if K >= 64:
        dropped = _sum_f32(terms[:, :-32], "chunks32")
        outside = np.abs(dropped.astype(np.float64) - ref) > R.e_acc(T, r)
        assert outside.mean() >= 0.9, outside.mean()


def test_bound_pieces():
    assert R.ulp16(1.0) == 2.0 ** -10 and R.ulp16(5.9) == 2.0 ** -8 and R.ulp16(0.0) == 2.0 ** -24 and R.ulp16(-0.3) == 2.0 ** -12
    assert R.e_acc(1.0, 9) == 9 * R.U and R.e_acc(1.0, 10000) == 800 * R.U     # worst case below r = 64, the sqrt form above
    assert R.tolerance(1.0, 0.0, 5, True) == 2.0 ** -11 and R.tolerance(1.0, 0.0, 5, False) == 0.0
    t = R.in_image_taps(19, 19, 3, 1, 1, 1)
    assert t[0, 0] == 4 and t[0, 5] == 6 and t[9, 9] == 9 and t[18, 18] == 4
    t = R.in_image_taps(10, 10, 3, 2, 0, 0)                     # even map, stride 2: the padding is bottom / right only
    assert t.shape == (5, 5) and t[0, 0] == 9 and t[4, 4] == 4 and t[0, 4] == 6


# ---------------------------------------------------------------------------------------------------------------------------------
# weights spread like a trained checkpoint's (tests/trained_like.py): the generator's properties, the emulators inside the bound,
# the seeded defects named again, and the defects that only such weights can show
# ---------------------------------------------------------------------------------------------------------------------------------
TL_SEED = 77


def _real_program(family):
    return {"mobilenet_v2": (arch.build(fuse=False), synthetic_weights, 2.0),
            "inception_v2": (inception.build(), synthetic_inception_v2, 1.5),
            "mobilenet_v1": (mobilenet_v1.build(fuse=False), synthetic_mobilenet_v1, 1.5)}[family]


@pytest.fixture(scope="module")
def small_spread(small):
    """decades -> (program, trained-like weights, inputs) of the small program, built once."""
    prog, W, x = small
    cache = {}

    def get(decades):
        if decades not in cache:
            cache[decades] = (prog, TL.trained_like(W, prog, decades, TL_SEED), x)
        return cache[decades]
    return get


@pytest.fixture(scope="module")
def blocks_spread(blocks):
    """decades -> ({form -> (program, trained-like weights, float_form_upto)}, inputs) of the four-block programs."""
    progs, x = blocks
    cache = {}

    def get(decades):
        if decades not in cache:
            cache[decades] = {form: (prog, TL.trained_like(W, prog, decades, TL_SEED), ffu) for form, (prog, W, ffu) in progs.items()}
        return cache[decades], x
    return get


@pytest.mark.parametrize("family", ["small", "mobilenet_v2", "inception_v2", "mobilenet_v1"])
def test_trained_like_weights_have_the_properties_the_gpu_tests_rely_on(small, family):
    """In the float64 network on these weights: the per-channel max|activation| of every BatchNorm-produced tensor spans at least
    0.7 * decades decades between its 5th and 95th percentile; dead channels are exactly constant; saturated channels are 6 at more
    than 90 % of the pixels; fp16 subnormals exist among the packed `-p 16` weights (the lo halves of the robust program included) and
    among the activations rounded to fp16; the MobileNet-v2 result is what `--robust auto` packs the robust program for."""
    if family == "small":
        prog, W0, x = small
        decades = 2.0
    else:
        prog, make, decades = _real_program(family)
        W0 = make(SEED)
        x = pu.oracle_input_half([synthetic_frame(640, 480, 5000)])
    W = TL.trained_like(W0, prog, decades, TL_SEED)
    again = TL.trained_like(W0, prog, decades, TL_SEED)
    assert set(W) == set(W0) and all((W[k] == again[k]).all() and W[k].dtype == np.float32 and W[k].shape == W0[k].shape for k in W)
    assert any((W[k] != v).any() for k, v in TL.trained_like(W0, prog, decades, TL_SEED + 1).items())
    T, _, _ = R.run_program(prog, W, x.astype(np.float64))
    marks = TL.marks(prog, W)
    spans, n_dead, n_sat = {}, 0, 0
    for op in prog.ops:
        if not op.has_bn or op.out_mode == OUT_HEAD or op.kind == OP_POOL:
            continue
        c0 = op.coff if op.cdst else 0
        t = T[op.dst][..., c0:c0 + op.cout]
        lo, hi = np.percentile(np.abs(t).max(axis=(0, 1, 2)), [5, 95])
        spans[op.scope] = math.log10(hi / max(lo, 1e-300))
        m = marks.get(op.dst)
        if m is None:
            continue
        dead, sat = m["dead"][c0:c0 + op.cout], m["saturated"][c0:c0 + op.cout]
        n_dead, n_sat = n_dead + int(dead.sum()), n_sat + int(sat.sum())
        td = t[..., dead].reshape(-1, int(dead.sum()))
        assert (td == td[0]).all(), op.scope                                         # exactly constant: relu6(beta)
        assert ((td[0] >= 0) & (td[0] <= 6)).all()
        assert ((t[..., sat] == 6.0).mean(axis=(0, 1, 2)) > 0.9).all(), op.scope
    worst = min(spans, key=spans.get)
    assert spans[worst] >= 0.7 * decades, (worst, spans[worst])
    assert n_dead > 0 and n_sat > 0
    flat = [p for op in prog.ops for p in (op.parts if op.kind == OP_DWSEP else [op]) if p.kind != OP_POOL]
    sub_w = sum(TL.count_fp16_subnormal(R.engine_weights(p, W, 16)[0]) for p in flat if p.kind != OP_STEM)
    if family == "mobilenet_v2":
        for op in arch.build(hp_upto=arch.HP_ALL_BLOCKS, conv1_split=True).ops:
            if op.kind == arch.OP_MBCONV:
                bw = R.block_weights(op, W, R.chunk_form(op, R.FLOAT_FORM_UPTO))
                sub_w += sum(TL.count_fp16_subnormal(bw[k]) for k in ("e_lo", "p_lo") if bw[k] is not None)
        spread = R.engine.channel_spread_decades(W)
        print("\nengine.channel_spread_decades: %.2f" % spread)
        assert spread > R.engine.SPREAD_VALIDATED_DECADES
    sub_a = sum(TL.count_fp16_subnormal(t.astype(np.float16)) for name, t in T.items() if name != "input")
    print("\n%s at %.1f decades: narrowest tensor %s (%.2f decades p5 .. p95); %d dead and %d saturated channels; fp16 subnormals: %d "
          "packed weights, %d activations" % (family, decades, worst, spans[worst], n_dead, n_sat, sub_w, sub_a))
    assert sub_w > 0 and sub_a > 0


def test_trained_like_is_the_same_function_where_relu6_does_not_clip(small):
    """Without degenerate channels and on an input small enough that no activation reaches 6, the spread network's head outputs are
    those of the network it was made from: every consumer divides by what its producer multiplied by."""
    prog, W0, _ = small
    W0 = {k: v * np.float32(0.25) if k.endswith(("/gamma", "/beta")) else v for k, v in W0.items()}      # (a network that stays below 6)
    x = np.stack([R.noise_input(prog.size, 41, 1.0)]).astype(np.float64)
    T0, be0, lg0 = R.run_program(prog, W0, x)
    assert max(np.abs(t).max() for n, t in T0.items() if n != "input") < 6.0
    W = TL.trained_like(W0, prog, 2.0, TL_SEED, dead=0.0, saturated=0.0)
    _, be, lg = R.run_program(prog, W, x)
    assert np.abs(be - be0).max() <= 1e-5 * np.abs(be0).max() and np.abs(lg - lg0).max() <= 1e-5 * np.abs(lg0).max()   # (float32 variables)


@pytest.mark.parametrize("decades", [1.5, 2.0])
def test_walker_passes_the_fp32_sum_engine_on_trained_like_weights(small_spread, decades):
    prog, W, x = small_spread(decades)
    rep = R.walk(FakeEngine(prog, W), prog, W, x, check=False, marks=TL.marks(prog, W))
    print("\n%.1f decades: %s\n%s" % (decades, rep.summary(), rep.populations()))
    assert not rep.failures, rep.failures[:5]
    assert rep.ops_checked == len(prog.ops) and rep.ops_unchecked == 0
    assert max(v[0] for v in rep.worst.values()) <= 1.0
    assert rep.subnormal_refs > 0 and rep.dead_elements > 0 and rep.saturated_elements > 0


@pytest.mark.parametrize("decades", [1.0, 2.0])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_walker_passes_the_block_emulator_on_trained_like_weights(blocks_spread, form, decades):
    progs, x = blocks_spread(decades)
    prog, W, ffu = progs[form]
    worst, by_order = {}, {}
    for order in ORDERS:
        rep = R.walk(BlockEngine(prog, W, ffu, order), prog, W, x, float_form_upto=ffu, check=False, marks=TL.marks(prog, W))
        assert not rep.failures, (order, rep.failures[:5])
        assert rep.ops_checked == rep.blocks_checked == len(prog.ops) == 4 and rep.ops_unchecked == 0
        for k, v in rep.worst.items():
            worst[k] = max(worst.get(k, 0.0), v[0])
        by_order[order] = max(v[0] for k, v in rep.worst.items() if k != "block13_expand")
    print("\n%s at %.0f decade(s): worst err / tol over four orders: %s (the blocks by order: %s); %s"
          % (form, decades, "  ".join("%s %.3f" % kv for kv in sorted(worst.items())), "  ".join("%s %.3f" % (o, by_order[o]) for o in ORDERS),
             rep.populations()))
    assert max(worst.values()) < 1.0
    assert rep.dead_elements > 0 and rep.saturated_elements > 0                       # (block 3's expanded tensor)


def _only(where, msg):
    lines = [ln for ln in msg.splitlines()[1:] if "coverage" not in ln]
    assert lines and all("(%s," % where in ln for ln in lines), msg


# the two defects that need subnormal operands to show: defect -> op it is put into
SUBNORMAL_DEFECTS = {"store_flushes_subnormals": "expand", "subnormal_weights_read_as_zero": "mix/b1b"}


@pytest.mark.parametrize("defect", sorted(DEFECTS) + sorted(SUBNORMAL_DEFECTS))
def test_walker_names_the_op_of_every_defect_on_trained_like_weights(small_spread, defect):
    """The eleven seeded defects at two decades of spread, and two more: an fp16 store that flushes subnormal results to zero, a GEMM
    that reads subnormal fp16 weights as zero.  Each fails in the op that has it and in no other; the factor is printed."""
    prog, W, x = small_spread(2.0)
    where = DEFECTS[defect][0] if defect in DEFECTS else SUBNORMAL_DEFECTS[defect]
    with pytest.raises(AssertionError) as ei:
        R.walk(FakeEngine(prog, W, defect, where), prog, W, x)
    _only(where, str(ei.value))
    print("\n%s in %s at 2 decades: outside by a factor of %.3g" % (defect, where, _factor(str(ei.value))))


@pytest.mark.parametrize("defect,form", STRUCTURAL_CASES, ids=["%s-%s" % c for c in STRUCTURAL_CASES])
def test_walker_names_the_block_of_every_structural_defect_on_trained_like_weights(blocks_spread, defect, form):
    progs, x = blocks_spread(2.0)
    prog, W, ffu = progs[form]
    where = STRUCTURAL[defect][0]
    with pytest.raises(AssertionError) as ei:
        R.walk(BlockEngine(prog, W, ffu, "chunks32", defect, where), prog, W, x, float_form_upto=ffu)
    _only(where, str(ei.value))
    print("\n%s in %s (%s) at 2 decades: outside by a factor of %.3g" % (defect, where, form, _factor(str(ei.value))))


def test_walker_names_the_block_whose_pair_store_flushes_subnormals(blocks_spread):
    """hi = RN16(v), lo = RN16(v - hi): below |v| = 2^-3 the lo half is an fp16 subnormal.  A store that flushes it loses up to 2^-15:
    outside the float-form blocks' bound, in that block and in no other.  The linear unorm16 buffer's bound allows a whole code step
    (1 / 65535 of full scale) per tap and cannot see it; that figure is printed beside it."""
    progs, x = blocks_spread(2.0)
    prog, W, ffu = progs["float_form"]
    with pytest.raises(AssertionError) as ei:
        R.walk(BlockEngine(prog, W, ffu, "chunks32", "pair_store_flushes_subnormals", "b1"), prog, W, x, float_form_upto=ffu)
    _only("b1", str(ei.value))
    prog, W, ffu = progs["unorm16"]
    rep = R.walk(BlockEngine(prog, W, ffu, "chunks32", "pair_store_flushes_subnormals", "b1"), prog, W, x, float_form_upto=ffu, check=False)
    print("\npair_store_flushes_subnormals in b1 at 2 decades: float form outside by a factor of %.3g; unorm16 worst err / tol %.3g"
          % (_factor(str(ei.value)), rep.worst["block_hp"][0]))
    assert all("(b1," in f for f in rep.failures), rep.failures


@pytest.mark.parametrize("form", ["float_form", "unorm16"])
@pytest.mark.parametrize("defect", sorted(PRECISION) + ["wlo_subnormals_read_as_zero"])
def test_precision_defects_are_reported_on_trained_like_weights(blocks_spread, defect, form):
    """The 2^-12 defects again at two decades, in both 16-bit forms of the chunk buffer, and one more: a split-operand block that reads
    the subnormal values of its Wlo operands as zero.  Factors printed, not asserted -- except that the lo-half-alive rule must still
    name the zeroed tile."""
    progs, x = blocks_spread(2.0)
    prog, W, ffu = progs[form]
    where = PRECISION.get(defect, "b2")
    good = R.walk(BlockEngine(prog, W, ffu, "chunks32"), prog, W, x, float_form_upto=ffu, check=False)
    rep = R.walk(BlockEngine(prog, W, ffu, "chunks32", defect, where), prog, W, x, float_form_upto=ffu, check=False)
    kind = R.op_kind_name([o for o in prog.ops if o.scope == where][0], ffu)
    tol_fail = [f for f in rep.failures if "err / tol" in f]
    print("\n%s in %s (%s) at 2 decades: worst err / tol %.3g (without the defect %.3g); bound %s, exact checks %s"
          % (defect, where, form, rep.worst[kind][0], good.worst[kind][0], "FAILS" if tol_fail else "passes",
             "FAIL" if len(rep.failures) > len(tol_fail) else "pass"))
    assert not good.failures
    if defect == "output_lo_zeroed_in_one_tile":
        assert any("lo half dead" in f and "(%s," % where in f for f in rep.failures), rep.failures
    assert all("(%s," % where in f for f in rep.failures), rep.failures


def test_walker_names_a_dead_channel_that_holds_the_wrong_constant(small_spread):
    """A dead channel is compared bit for bit: the neighbouring channel's bias (a layout bug) fails in that op, under `dead channel`."""
    prog, W, x = small_spread(2.0)
    marks = TL.marks(prog, W)
    eng = FakeEngine(prog, W)
    ch = int(np.flatnonzero(marks["e1"]["dead"])[0])
    forward = eng.stage_forward

    def corrupted(x_half):
        out = forward(x_half)
        eng.T["e1"][..., ch] = eng.T["e1"][..., ch] + np.float16(2.0 ** -10)
        return out
    eng.stage_forward = corrupted
    rep = R.walk(eng, prog, W, x, check=False, marks=marks)
    assert any("dead channel" in f and "(e1," in f for f in rep.failures), rep.failures


@pytest.mark.parametrize("decades", [1.0, 2.0])
def test_the_builder_packs_the_robust_program_for_trained_like_weights(decades):
    """`--robust auto` decides by engine.channel_spread_decades: above SPREAD_VALIDATED_DECADES at one and two decades, and both
    `-p 16` programs build (the float-form tap scaling fits)."""
    W = TL.trained_like(synthetic_weights(SEED), arch.build(fuse=False), decades, TL_SEED)
    spread = R.engine.channel_spread_decades(W)
    print("\n%.1f decades: engine.channel_spread_decades %.2f" % (decades, spread))
    assert spread > R.engine.SPREAD_VALIDATED_DECADES
    assert len(R.engine.build_engine(W, robust=True)) > 0 and len(R.engine.build_engine(W)) > 0
