"""tests/op_reference.py proves itself without a GPU: the chained float64 references against the three fp32 oracles, the walker on a
fake engine with one seeded defect at a time, and the bound function on fp32 sums in four orders."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import op_reference as R
import parity_utils as pu
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
            elif op.cdst:
                t = T.setdefault(op.dst, np.zeros(y.shape[:3] + (op.cdst,), np.float16))
                coff = op.coff + (8 if d == "slice_written_8_channels_late" else 0)
                t[..., coff:coff + op.cout] = y.astype(np.float16)
            else:
                T[op.dst] = y.astype(np.float16)
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
