"""Engine builder: model weights -> `mi355x.bin`, the file `HipObjectDetector` loads.

MI355X analogue of `watsor/engine.py:17-107` (TensorRT engine builder CLI, run once before the
application starts, auto-invoked by `watsor/main_for_gpu.py:17-26` when `gpu.uff`/`gpu.onnx` exists
without `gpu.trt`).  Same command line shape (`-i/--input`, `-p/--precision {32,16}`, `-w`, `-mw`,
`-mh`, `-o/--output`); the input is an `.npz` of TF variables (names as in the frozen graph of
`ssd_mobilenet_v2_coco`, `ssd_inception_v2_coco` or `ssd_mobilenet_v1_coco`, TF layouts, BatchNorm unfolded), a frozen graph, or the
literal `synthetic[:seed]` (MobileNet-v2) / `synthetic_inception_v2[:seed]` / `synthetic_mobilenet_v1[:seed]`.  The network family is
read from the variable names.

What building does: fold every FusedBatchNorm into its convolution (fp64), round to fp16, lay the
weights out in the MFMA fragment order the HIP kernels read (csrc/wz_program.h), generate the anchor
table, assign activation tensors to HBM buffer slots by liveness, and write one flat image.
"""
from __future__ import annotations

import argparse
import os
import struct
import sys
from typing import Dict, List, Optional

import numpy as np

from . import arch, inception, mobilenet_v1
from .anchors import ssd_anchor_table

MAGIC = 0x35335A57
FORMAT_VERSION = 12
FAMILIES = {"MobilenetV2": "SSD-MobileNet-v2", "InceptionV2": "SSD-Inception-v2",
            "MobilenetV1": "SSD-MobileNet-v1"}   # feature extractor scope -> network
POOL_AVG = 16              # WzOpFlags::WZ_OPF_POOL_AVG (csrc/wz_program.h)
BN_EPSILON = 1e-3          # watsor/test/model/prepare.py:48

DEFAULT_POST = dict(max_total=100, max_per_class=100, score_threshold=1e-8, iou_threshold=0.6,
                    scales=(10.0, 10.0, 5.0, 5.0))   # prepare.py:54-61,120-128; SURVEY.md App. B.5
# The two steps whose form differs between exporter generations: how ResizeBilinear maps output to
# input coordinates, and whether boxes are clipped to the image before or after the per-class NMS.  Defaults = the 2018 graph
# the reference's README names; a frozen graph's own ResizeBilinear attributes override the first (frozen_graph.graph_settings).
RESIZE_MODES = {"legacy": 0, "half_pixel": 1}
DEFAULT_OPTIONS = dict(resize="legacy", clip_after_nms=False)


def apply_graph_settings(settings: dict, model_width: int, model_height: int, post: Optional[dict], options: Optional[dict]):
    """What a frozen graph says about itself (`frozen_graph.graph_settings`) -> (post, options) for `build_engine`; raises
    ValueError for a graph this engine cannot reproduce.  Explicit `post` / `options` entries must agree with the graph."""
    post, options = dict(post or {}), dict(options or {})

    def adopt(target, key, value, what):
        if key in target and target[key] != value:
            raise ValueError("%s: the graph says %r, the command line says %r" % (what, value, target[key]))
        target[key] = value

    if "input_size" in settings and tuple(settings["input_size"]) != (model_height, model_width):
        raise ValueError("the graph resizes its input to %dx%d, the engine is being built for %dx%d (-mw / -mh)"
                         % (settings["input_size"][1], settings["input_size"][0], model_width, model_height))
    if settings.get("resize_align_corners"):
        raise ValueError("the graph's ResizeBilinear has align_corners=True: not a resize mode of this engine")
    if "resize_half_pixel_centers" in settings:
        adopt(options, "resize", "half_pixel" if settings["resize_half_pixel_centers"] else "legacy", "resize mode")
    for key, what in (("iou_threshold", "NMS IoU threshold"), ("score_threshold", "score threshold"),
                      ("max_per_class", "detections per class"), ("max_total", "total detections")):
        if key in settings:
            v = settings[key]
            if key.endswith("threshold"):
                v = float(np.float32(v))
                if key in post:
                    post[key] = float(np.float32(post[key]))
            adopt(post, key, v, what)
    if "box_scales_ambiguous" in settings and "box_scales" not in settings:
        import warnings
        warnings.warn("the graph's box-coder scale factors could not be read unambiguously (%r): keeping %r"
                      % (settings["box_scales_ambiguous"], tuple(post.get("scales", (10.0, 10.0, 5.0, 5.0)))))
    if "box_scales" in settings:
        sc = tuple(float(x) for x in settings["box_scales"])
        if len(sc) != 4 or min(sc) <= 0:
            raise ValueError("the graph's box decoder has %d scale factors %r, expected (ty, tx, th, tw)" % (len(sc), sc))
        adopt(post, "scales", sc, "box coder scale factors")
    if settings.get("anchor_vectors"):
        from .anchors import ssd_box_specs
        specs = ssd_box_specs()
        expected = []
        for layer in specs:
            expected.append(np.array([s for s, _ in layer], np.float32))
            expected.append(np.array([r for _, r in layer], np.float32))
        lengths = {len(layer) for layer in specs}
        for v in settings["anchor_vectors"]:
            if v.size in lengths and not any(e.size == v.size and np.allclose(e, v, rtol=0, atol=2e-4) for e in expected):
                raise ValueError("the graph's anchor generator holds %s, which is neither a scale nor an aspect-ratio list of this "
                                 "engine's anchors (scales 0.2 .. 0.95, ratios 1, 2, 1/2, 3, 1/3; watsor_amd/anchors.py)"
                                 % np.array2string(v, precision=4))
    if post.get("max_total", 100) > 100 or post.get("max_total", 100) < 1:
        raise ValueError("max_total %r: the Detection array of a frame holds 100 rows (watsor/stream/share.py:31)" % post["max_total"])
    return post, options


def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


def _families_built() -> str:
    return " and ".join("%s (FeatureExtractor/%s/)" % (v, k) for k, v in FAMILIES.items())


def detect_family(weights: Dict[str, np.ndarray]) -> str:
    """The feature extractor the variables belong to ("MobilenetV2", "InceptionV2" or "MobilenetV1"), from their
    `FeatureExtractor/<name>/` scope; ValueError for any other (or for a mixture).  The MobilenetV1 scope is also that of other
    MobileNet-v1 detectors: a model under it that lacks any of the SSD-MobileNet-v1 feature extractor's variables is refused here,
    before anything reads them.  Other float constants under the scope are ignored, as for the other two networks."""
    found = sorted({k.split("/")[1] for k in weights if k.startswith("FeatureExtractor/") and k.count("/") >= 2})
    if found == ["MobilenetV1"]:
        missing = sorted(k for k in mobilenet_v1.build(fuse=False).variable_shapes() if k.startswith(mobilenet_v1.FE) and k not in weights)
        if missing:
            raise ValueError("the model's FeatureExtractor/MobilenetV1/ variables are not SSD-MobileNet-v1's (%d of its variables missing, "
                             "e.g. %s); this engine builds %s" % (len(missing), missing[0], _families_built()))
    if len(found) == 1 and found[0] in FAMILIES:
        return found[0]
    raise ValueError("the model's feature extractor is %s; this engine builds %s" % (
        " + ".join(found) if found else "unknown (no FeatureExtractor/ variables)", _families_built()))


def fold_stem7(W: Dict[str, np.ndarray], op: "arch.Op") -> np.ndarray:
    """The separable stem (depthwise [k,k,c,m], pointwise [1,1,c*m,cout]) as one dense [k,k,c,cout] kernel, float64:
    W[ky,kx,c,o] = sum_m dw[ky,kx,c,m] * pw[0,0,c*m_count+m,o] (TF orders the depthwise outputs channel-major)."""
    dw = W[op.scope + "/depthwise_weights"].astype(np.float64)
    pw = W[op.scope + "/pointwise_weights"].astype(np.float64)
    k, _, c, m = dw.shape
    return np.einsum("yxcm,cmo->yxco", dw, pw[0, 0].reshape(c, m, pw.shape[3]))


def fold_batch_norm(W: Dict[str, np.ndarray], op: "arch.Op"):
    """(weights float64 in TF layout, bias float64[cout]) with BatchNorm folded in."""
    if op.out_mode == arch.OUT_HEAD:                                     # [k,k,cin, a*4 | a*91], biases only
        w = np.concatenate([W[op.scope + "/BoxEncodingPredictor/weights"], W[op.scope + "/ClassPredictor/weights"]],
                           axis=3).astype(np.float64)
        b = np.concatenate([W[op.scope + "/BoxEncodingPredictor/biases"], W[op.scope + "/ClassPredictor/biases"]])
        return w, b.astype(np.float64)
    if op.kind == arch.OP_DW:
        w = W[op.scope + "/depthwise_weights"].astype(np.float64)        # [k,k,C,1]
    elif op.kind == arch.OP_STEM7:
        w = fold_stem7(W, op)                                            # [7,7,3,64], before the BatchNorm
    else:
        w = W[op.scope + "/weights"].astype(np.float64)                  # [k,k,cin,cout]
    if not op.has_bn:
        return w, W[op.scope + "/biases"].astype(np.float64)
    g = W[op.scope + "/BatchNorm/gamma"].astype(np.float64)
    b = W[op.scope + "/BatchNorm/beta"].astype(np.float64)
    m = W[op.scope + "/BatchNorm/moving_mean"].astype(np.float64)
    v = W[op.scope + "/BatchNorm/moving_variance"].astype(np.float64)
    s = g / np.sqrt(v + BN_EPSILON)
    w = w * (s[None, None, :, None] if op.kind == arch.OP_DW else s[None, None, None, :])
    return w, b - m * s


def pack_conv_weights(w: np.ndarray, n_pad: int, kc: int) -> np.ndarray:
    """[k,k,cin,cout] -> fp16 [n_pad/16][taps][kc][64][8] (A-operand fragments of mfma_f32_16x16x32_f16)."""
    k, _, cin, cout = w.shape
    taps = k * k
    wp = np.zeros((taps, kc * 32, n_pad), np.float32)
    wp[:, :cin, :cout] = w.reshape(taps, cin, cout)
    # k index = c*32 + g*8 + j ; n index = t*16 + r ; lane = g*16 + r
    wp = wp.reshape(taps, kc, 4, 8, n_pad // 16, 16)            # [tap][c][g][j][t][r]
    wp = wp.transpose(4, 0, 1, 2, 5, 3)                         # [t][tap][c][g][r][j]
    return np.ascontiguousarray(wp).astype(np.float16).reshape(-1)


def split_halves(w: np.ndarray):
    """float64 array -> (hi, lo) float64 arrays holding fp16 values with hi + lo ~ w to about 2^-22 relative
    (hi = RN16(w), lo = RN16(w - hi)): the two A operands of the split-operand kernels (csrc/k_mbconv_hp.hip)."""
    hi = w.astype(np.float16).astype(np.float64)
    lo = (w - hi).astype(np.float16).astype(np.float64)
    return hi, lo


UNORM16_PER_6 = 65535.0 / 6.0    # the split-operand blocks keep relu6 outputs in LDS as unorm16 of x / 6
FLOAT_FORM_T = 2.0 ** -120 * (2.0 - 2.0 ** -13)   # ... the robust program as a 16-bit float: bits 10 .. 25 of the fp32 pattern of t = (x / 6) T -- exponent field
                                                  # 0 .. 7, 13 mantissa bits, subnormal below code 8192 (csrc/k_hp_ops.h: one instruction decodes a value)
FLOAT_FORM_TAP_SCALE = 6.0 * 2.0 ** 60 / (2.0 - 2.0 ** -13)   # what the depthwise taps of such a block carry; the kernel scales the tap sum back by 2^60
FLOAT_FORM_LAST_BLOCK = 12       # the last block whose kernel has a float-form build (csrc/k_mbconv_hp.hip: wz_launch_mbconv_hp_q; the 10x10 maps do not)


def stem_k_rows(w: np.ndarray) -> np.ndarray:
    """Stem weights [3,3,3,cout] -> [32, cout] in the K order the split-operand stem block gathers its B fragments in
    (csrc/k_mbconv_hp.hip): k = tap*4 + c for taps 0 .. 7 (a lane group's 8 values = the 4-channel pixels of two taps,
    loaded as they lie in the input tensor, no element shuffling), and the ninth tap's three channels in the zero-channel
    slots of taps 0, 1, 2 (k = 3, 7, 11).  The plain program keeps k = tap*3 + c (csrc/k_mbconv_wave.hip)."""
    cout = w.shape[3]
    out = np.zeros((32, cout), w.dtype)
    for t in range(8):
        for c in range(3):
            out[t * 4 + c] = w[t // 3, t % 3, c]
    for c in range(3):
        out[c * 4 + 3] = w[2, 2, c]
    return out


def stem7_k_rows(w: np.ndarray) -> np.ndarray:
    """Dense stem weights [7,7,3,cout] -> [224, cout] with k = tap * 4 + c (tap = ky * 7 + kx): a lane group's 8 K values are the
    4-channel pixels of two taps as they lie in the input tensor (csrc/k_inception.hip); channel 3 and taps 49 .. 55 are zero.
    49 taps x 4 = 196 rows, seven 32-row MFMA chunks."""
    k, _, c, cout = w.shape
    out = np.zeros((STEM7_KC * 32, cout), w.dtype)
    for t in range(k * k):
        out[t * 4:t * 4 + c] = w[t // k, t % k]
    return out


STEM7_KC = 7


def pack_conv_weights_f32(w: np.ndarray, n_pad: int, kc: int) -> np.ndarray:
    """[k,k,cin,cout] -> fp32 [n_pad/16][taps][kc][64][4]: lane (r16, g) of N-tile t holds W[k = c*16 + 4g + j][n = t*16 + r16]
    (the A operands of four v_mfma_f32_16x16x4_f32, one float4 load per lane; csrc/k_f32.hip)."""
    k, _, cin, cout = w.shape
    taps = k * k
    wp = np.zeros((taps, kc * 16, n_pad), np.float32)
    wp[:, :cin, :cout] = w.reshape(taps, cin, cout)
    wp = wp.reshape(taps, kc, 4, 4, n_pad // 16, 16)            # [tap][c][g][j][t][r]
    wp = wp.transpose(4, 0, 1, 2, 5, 3)                         # [t][tap][c][g][r][j]
    return np.ascontiguousarray(wp).reshape(-1)


OP_RECORD_BYTES = 256


def _op_record(op, tindex, n_pad, kc, w_off, b_off, mb) -> bytes:
    """struct WzOpDesc of csrc/wz_program.h.  An op that writes a channel slice of its output (Op.cdst) carries the slice in the
    fields the fused blocks use for cmid / cin0 (dst_coff / dst_c); every op of the MobileNet programs leaves them as they were."""
    if getattr(op, "cdst", 0):
        assert op.kind in (arch.OP_CONV, arch.OP_POOL, arch.OP_STEM7) and not mb["cmid"] and not mb["cin0"]
        mb = dict(mb, cmid=op.coff, cin0=op.cdst)
    return struct.pack(
        "<20i2q8i8q64s",
        op.kind, tindex[op.src], tindex.get(op.dst, -1) if op.out_mode == arch.OUT_ACT else -1,
        tindex[op.res] if op.res else -1,
        op.cin, op.cout, op.k, op.stride,
        op.hin, op.win, op.hout, op.wout,
        op.pad_t, op.pad_l, op.act, op.out_mode,
        op.anchor_offset, op.anchors_per_loc, n_pad, kc,
        w_off, b_off,
        op.n_box, mb["cmid"], mb["cin0"], mb["kc0"], mb["cmid_pad"], mb["nmid_pad"], mb["stem"], mb["stem_pad"],
        mb["we_off"], mb["be_off"], mb["wd_off"], mb["bd_off"], mb.get("we_lo_off", 0), mb.get("w_lo_off", 0),
        mb.get("flags", 0), (tindex[op.dst2] + 1) if getattr(op, "dst2", None) else 0,
        op.scope.encode()[:63])


def assign_slots(prog: "arch.Program", tensor_names: List[str]) -> List[int]:
    """Liveness-based buffer sharing: tensors whose lifetimes do not overlap reuse one HBM buffer.  A tensor written by several ops
    (the concat of an Inception module, one slice per branch) lives from its first writer on; the slot is taken before that op's
    inputs are released, so no writer's input can share it.  A head's convolution may be launched after the last op (the grouped
    launches of HeadPark::flush, csrc/wz_network.hip): what a head reads lives to the end of the program and its slot is never
    released.  (Every builder appends the heads last, where nothing is allocated any more: the rule costs today's programs no slot.)"""
    index = {n: i for i, n in enumerate(tensor_names)}
    last_use = {n: -1 for n in tensor_names}
    for oi, op in enumerate(prog.ops):
        at = oi if op.out_mode == arch.OUT_ACT else len(prog.ops)
        last_use[op.src] = max(last_use[op.src], at)
        if op.res:
            last_use[op.res] = max(last_use[op.res], at)
    size = {n: prog.tensors[n].h * prog.tensors[n].w * (4 if n == "input" else prog.tensors[n].c) * (2 if prog.tensors[n].hp else 1)
            for n in tensor_names}
    slot_of = [-1] * len(tensor_names)
    slot_size: List[int] = []
    free: List[int] = []
    slot_of[index["input"]] = 0
    slot_size.append(size["input"])
    for oi, op in enumerate(prog.ops):
        never_read = []                                      # released only after ALL outputs of the op have their slots
        for out in ([op.dst, op.dst2] if op.out_mode == arch.OUT_ACT else []):
            if out is None or slot_of[index[out]] >= 0:     # (a later writer of a concat tensor: the slot is taken)
                continue
            need = size[out]
            best = None
            for s in free:                                   # best fit among free slots
                if best is None or abs(slot_size[s] - need) < abs(slot_size[best] - need):
                    best = s
            if best is None:
                best = len(slot_size)
                slot_size.append(need)
            else:
                free.remove(best)
                slot_size[best] = max(slot_size[best], need)
            slot_of[index[out]] = best
            if last_use[out] < 0:                            # never read (cannot happen in this graph)
                never_read.append(best)
        free.extend(never_read)
        for n in {op.src, op.res} - {None}:
            if last_use[n] == oi:
                free.append(slot_of[index[n]])
    return slot_of


def build_engine(weights: Dict[str, np.ndarray], precision: int = 16, model_width: int = 300,
                 model_height: int = 300, post: Optional[dict] = None, fuse: bool = True,
                 fuse_stem: bool = True, hp_upto: Optional[int] = None, options: Optional[dict] = None,
                 robust: bool = False, tap_in_block: bool = True, float_form_upto: int = 9, conv1_split: Optional[bool] = None) -> bytes:
    """Returns the engine image.  Mirrors `build_engine` of watsor/engine.py:17-51.
    fuse=False keeps one op per layer (used by the per-layer parity tests; same results, slower).
    hp_upto: last inverted-residual block on the split-operand kernel (default for the `-p 16` program with fused
    blocks: arch.HP_LAST_BLOCK, which is what keeps its scores within 1e-3 of the fp32 detector; -1 = plain fp16
    everywhere, the faster engine that misses that tolerance by 3x).
    robust (precision 16): ALL 17 blocks on the split-operand kernel and the expanded tensors kept as unorm16 of sqrt(x / 6) instead
    of x / 6 -- the program for weights whose channels live at very different scales (a folded trained BatchNorm), where the
    default program loses the tolerance.
    float_form_upto (robust): the last block whose expanded tensor is kept in the 16-bit float form; the blocks behind it keep the
    linear unorm16 buffer of the default program.  Blocks 13 .. 16 make no difference to the scores (tools/err_budget.py) and the float
    form costs them 2 us each; blocks 10 .. 12 buy 1e-4 at two decades of channel spread for 2.8 us (measured, round 4: up to block
    9: 45.7 k frames/s, 7.6e-4 at 2.0 decades; up to block 12: 44.5 k, 6.7e-4).
    conv1_split (robust, default on): Conv_1's weights as hi + lo halves over a doubled block-16 output (arch.build).  Off: +2.4 k
    frames/s and 9.1e-4 instead of 7.6e-4 at two decades (6.9e-4 instead of 6.1e-4 at 1.5) -- inside the tolerance, without margin.
    tap_in_block=False: block 13's expand conv -- the first SSD feature map -- as a launch of its own in front of the block instead of
    the block's second output (the program of rounds 1 .. 3; for A/B runs)."""
    if precision not in (16, 32):
        raise ValueError("precision must be 16 (fp16 storage, fp16 MFMA, fused blocks) or 32 (fp32 storage, fp32 MFMA)")
    if precision == 32:
        fuse = False                 # the fp32 engine runs one op per layer (csrc/k_f32.hip)
    if model_width != model_height:
        raise ValueError("square model input expected")
    family = detect_family(weights) if any(k.startswith("FeatureExtractor/") for k in weights) else None
    if family in ("InceptionV2", "MobilenetV1"):
        if robust or hp_upto not in (None, -1) or conv1_split:
            raise ValueError("the robust, split-operand and fused-block programs are SSD-MobileNet-v2 programs; an %s "
                             "engine is built with -p 16 or -p 32 only" % FAMILIES[family])
        if family == "MobilenetV1":
            return build_mobilenet_v1_engine(weights, precision, model_width, model_height, post=post, options=options, fuse=fuse)
        return build_inception_engine(weights, precision, model_width, model_height, post=post, options=options)
    cfg, opt = _post_options(post, options)
    if robust and not (precision == 16 and fuse and fuse_stem and hp_upto is None):
        raise ValueError("the robust program is the `-p 16` program with fused blocks")
    if robust and not (-1 <= float_form_upto <= FLOAT_FORM_LAST_BLOCK):
        # (blocks 13 .. 16 -- the 10x10 maps -- exist with the linear chunk buffer only: an engine asking for the float form there would be
        #  refused by the runtime with "no split-operand kernel took op")
        raise ValueError("float_form_upto %r: the float-form chunk buffer exists for blocks 0 .. %d (-1: nowhere)" % (float_form_upto, FLOAT_FORM_LAST_BLOCK))
    if hp_upto is None:
        hp_upto = (arch.HP_ALL_BLOCKS if robust else arch.HP_LAST_BLOCK) if (precision == 16 and fuse and fuse_stem) else -1
    prog = arch.build(model_width, fuse=fuse, fuse_stem=fuse_stem, hp_upto=hp_upto, input_pair=precision == 32, tap_in_block=tap_in_block,
                      conv1_split=robust if conv1_split is None else bool(conv1_split))
    _check_variables(prog, weights)

    tensor_names = ["input"] + [t for op in prog.ops if op.out_mode == arch.OUT_ACT for t in (op.dst, op.dst2) if t]
    tindex = {n: i for i, n in enumerate(tensor_names)}
    slots = assign_slots(prog, tensor_names)

    wblob = bytearray()

    def put(arr: np.ndarray) -> int:
        off = _align(len(wblob))
        wblob.extend(b"\0" * (off - len(wblob)))
        wblob.extend(arr.tobytes())
        return off

    def put_conv(op):
        w, b = fold_batch_norm(weights, op)
        if op.split_w:                                           # [hi halves | lo halves] along the input channels (arch.Op.split_w)
            hi, lo = split_halves(w)
            w = np.concatenate([hi.astype(np.float64), lo.astype(np.float64)], axis=2)
            assert w.shape[2] == op.cin
        n_pad = _align(op.cout, 64 if op.cout >= 256 else 32)   # 64-wide wave tiles for the wide layers
        if precision == 32:
            kc = (op.cin + 15) // 16
            w_off = put(pack_conv_weights_f32(w.astype(np.float32), n_pad, kc))
        else:
            kc = (op.cin + 31) // 32
            w_off = put(pack_conv_weights(w.astype(np.float32), n_pad, kc))
        bp = np.zeros(n_pad, np.float32)
        bp[:op.cout] = b
        return w_off, put(bp), n_pad, kc

    op_recs = []
    for op in prog.ops:
        n_pad, kc = 0, 0
        mb = dict(cmid=0, cin0=0, kc0=0, cmid_pad=0, nmid_pad=0, we_off=0, be_off=0, wd_off=0, bd_off=0, stem=0, stem_pad=0)
        if op.kind == arch.OP_MBCONV and op.hp:
            # split-operand block: GEMM weights as hi + lo fp16 fragments; the expand stage (or the stem) produces
            # relu6(.)/6 in [0, 1] (kept in LDS as unorm16), so 1/6 goes into its weights and bias and 6/65535 into
            # the depthwise weights, which stay fp32
            parts = list(op.parts)

            def put_split(w, n_pad, kc):
                hi, lo = split_halves(w)
                return (put(pack_conv_weights(hi.astype(np.float32), n_pad, kc)),
                        put(pack_conv_weights(lo.astype(np.float32), n_pad, kc)))

            if op.stem:
                st = parts.pop(0)
                w, b = fold_batch_norm(weights, st)
                mb["we_off"], mb["we_lo_off"] = put_split(stem_k_rows(w).reshape(1, 1, 32, st.cout) / 6.0, 32, 1)
                mb["be_off"] = put((b / 6.0).astype(np.float32))
                mb.update(nmid_pad=32, kc0=1, stem=1, stem_pad=(op.stem_pad[0] << 16) | op.stem_pad[1])
            else:
                assert op.cin0, "a split-operand block without an expand stage must be the stem block"
                ex = parts.pop(0)
                w, b = fold_batch_norm(weights, ex)
                nmid_pad = _align(ex.cout, 64 if ex.cout >= 256 else 32)
                kc0 = (ex.cin + 31) // 32
                mb["we_off"], mb["we_lo_off"] = put_split(w / 6.0, nmid_pad, kc0)
                bep = np.zeros(nmid_pad, np.float32)
                bep[:ex.cout] = b / 6.0
                mb["be_off"] = put(bep)
                mb.update(nmid_pad=nmid_pad, kc0=kc0)
            dw, pj = parts
            wd, bd = fold_batch_norm(weights, dw)
            cmid_pad = _align(op.cmid, 32)
            wdp = np.zeros((9, cmid_pad), np.float32)
            bdp = np.zeros(cmid_pad, np.float32)
            float_form = robust and op.block <= float_form_upto
            if float_form:
                # the buffer holds the 16-bit float form of t = (x / 6) T, T = 2^-120 (2 - 2^-13) (k_hp_ops.h): x = 6 t / T.  The factor is
                # split -- the taps carry 6 * 2^60 / (2 - 2^-13), the kernel multiplies the tap sum by an exact 2^60 while it adds the bias --
                # so that a large folded depthwise weight cannot overflow fp32 (6 / T alone is 4e36).  Padding is code 0 = value 0: the
                # bias is the plain one
                w9 = wd.reshape(9, op.cmid)
                wdp[:, :op.cmid] = (w9 * FLOAT_FORM_TAP_SCALE).astype(np.float32)
                if not np.isfinite(wdp).all():
                    raise ValueError("%s: a depthwise weight of %.3g does not fit the float-form scaling" % (op.scope, np.abs(w9).max()))
                bdp[:op.cmid] = bd
            else:
                wdp[:, :op.cmid] = (wd.reshape(9, op.cmid) / UNORM16_PER_6).astype(np.float32)
                bdp[:op.cmid] = bd
            mb.update(cmid=op.cmid, cin0=op.cin0, cmid_pad=cmid_pad, wd_off=put(wdp), bd_off=put(bdp))
            w, b = fold_batch_norm(weights, pj)
            n_pad = _align(pj.cout, 64 if pj.cout >= 256 else 32)
            kc = (pj.cin + 31) // 32
            w_off, mb["w_lo_off"] = put_split(w, n_pad, kc)
            bp = np.zeros(n_pad, np.float32)
            bp[:pj.cout] = b
            b_off = put(bp)
            mb["flags"] = 1 | (2 if prog.tensors[op.dst].hp else 0) | (4 if float_form else 0) | (8 if op.dup_out else 0)
            op_recs.append(_op_record(op, tindex, n_pad, kc, w_off, b_off, mb))
            continue
        if op.kind == arch.OP_MBCONV:
            parts = list(op.parts)
            if op.stem:                                    # the stem conv as a K = 27 (padded 32) "expand" GEMM
                st = parts.pop(0)
                w, b = fold_batch_norm(weights, st)        # [3,3,3,32]: k = (ky*3+kx)*3 + c
                mb["we_off"] = put(pack_conv_weights(w.reshape(1, 1, 27, st.cout).astype(np.float32), 32, 1))
                mb["be_off"] = put(b.astype(np.float32))
                mb.update(nmid_pad=32, kc0=1, stem=1, stem_pad=(op.stem_pad[0] << 16) | op.stem_pad[1])
            elif op.cin0:
                ex = parts.pop(0)
                mb["we_off"], mb["be_off"], mb["nmid_pad"], mb["kc0"] = put_conv(ex)
            dw, pj = parts
            wd, bd = fold_batch_norm(weights, dw)
            cmid_pad = _align(op.cmid, 32)
            wdp = np.zeros((9, cmid_pad), np.float16)
            wdp[:, :op.cmid] = wd.reshape(9, op.cmid).astype(np.float16)
            bdp = np.zeros(cmid_pad, np.float32)
            bdp[:op.cmid] = bd
            mb.update(cmid=op.cmid, cin0=op.cin0, cmid_pad=cmid_pad, wd_off=put(wdp), bd_off=put(bdp))
            w_off, b_off, n_pad, kc = put_conv(pj)
            op_recs.append(_op_record(op, tindex, n_pad, kc, w_off, b_off, mb))
            continue
        w, b = fold_batch_norm(weights, op)
        if op.kind == arch.OP_STEM:
            w_off = put(w.reshape(27, 32).astype(np.float32))
            b_off = put(b.astype(np.float32))
        elif op.kind == arch.OP_DW:
            w_off = put(w.reshape(9, op.cin).astype(np.float32 if precision == 32 else np.float16))
            b_off = put(b.astype(np.float32))
        else:
            w_off, b_off, n_pad, kc = put_conv(op)
        op_recs.append(_op_record(op, tindex, n_pad, kc, w_off, b_off, mb))
    return _write_image(prog, precision, model_width, cfg, opt, tensor_names, slots, op_recs, wblob, hp_upto + 1)


def _write_image(prog, precision, model_width, cfg, opt, tensor_names, slots, op_recs, wblob, hp_blocks) -> bytes:
    """Header, tensor table, op records, anchors and weight blob as one image (struct WzBlobHeader of csrc/wz_program.h)."""
    assert all(len(r) == OP_RECORD_BYTES for r in op_recs)
    tensor_recs = []
    for n, s in zip(tensor_names, slots):
        t = prog.tensors[n]
        tensor_recs.append(struct.pack("<5i44s", t.h, t.w, 4 if n == "input" else t.c, s, 1 if t.hp else 0, n.encode()[:43]))

    anchors = ssd_anchor_table([g for _, g, _ in prog.feature_maps], [a for _, _, a in prog.feature_maps])
    assert anchors.shape == (prog.num_anchors, 4)

    header_size = 160
    tensors_off = _align(header_size)
    ops_off = _align(tensors_off + 64 * len(tensor_recs))
    anchors_off = _align(ops_off + OP_RECORD_BYTES * len(op_recs))
    weights_off = _align(anchors_off + anchors.nbytes)
    total = weights_off + len(wblob)
    sy, sx, sh, sw = cfg["scales"]
    header = struct.pack(
        "<10I6f6Q12I",
        MAGIC, FORMAT_VERSION, precision, model_width,
        arch.NUM_CLASSES, prog.num_anchors, len(tensor_recs), len(op_recs),
        cfg["max_total"], cfg["max_per_class"],
        cfg["score_threshold"], cfg["iou_threshold"], sy, sx, sh, sw,
        tensors_off, ops_off, anchors_off, weights_off, len(wblob), total,
        max(slots) + 1, hp_blocks, RESIZE_MODES[opt["resize"]], 1 if opt["clip_after_nms"] else 0, *([0] * 8))
    assert len(header) == header_size
    out = bytearray(total)
    out[:header_size] = header
    out[tensors_off:tensors_off + 64 * len(tensor_recs)] = b"".join(tensor_recs)
    out[ops_off:ops_off + OP_RECORD_BYTES * len(op_recs)] = b"".join(op_recs)
    out[anchors_off:anchors_off + anchors.nbytes] = anchors.tobytes()
    out[weights_off:] = wblob
    return bytes(out)


def _post_options(post: Optional[dict], options: Optional[dict]):
    cfg = dict(DEFAULT_POST)
    cfg.update(post or {})
    opt = dict(DEFAULT_OPTIONS)
    opt.update(options or {})
    if opt["resize"] not in RESIZE_MODES:
        raise ValueError("resize mode %r: expected one of %s" % (opt["resize"], ", ".join(RESIZE_MODES)))
    return cfg, opt


def _check_variables(prog: "arch.Program", weights: Dict[str, np.ndarray]) -> None:
    missing = [n for n in prog.variable_shapes() if n not in weights]
    if missing:
        raise KeyError("model is missing %d variables, e.g. %s" % (len(missing), missing[0]))
    for name, shape in prog.variable_shapes().items():
        if tuple(weights[name].shape) != tuple(shape):
            raise ValueError("%s has shape %s, expected %s" % (name, weights[name].shape, shape))


def head_kernel_sizes(weights: Dict[str, np.ndarray]) -> List[int]:
    """Kernel size of each of the six box predictors, from their weights ([k,k,cin,cols], k = 1 or 3)."""
    ks = []
    for i in range(6):
        name = "BoxPredictor_%d/BoxEncodingPredictor/weights" % i
        if name not in weights:
            raise KeyError("model is missing %s" % name)
        shp = weights[name].shape
        if len(shp) != 4 or shp[0] != shp[1] or shp[0] not in (1, 3):
            raise ValueError("%s has shape %s: a 1x1 or 3x3 box predictor expected" % (name, tuple(shp)))
        ks.append(int(shp[0]))
    return ks


def build_inception_engine(weights: Dict[str, np.ndarray], precision: int = 16, model_width: int = 300, model_height: int = 300,
                           post: Optional[dict] = None, options: Optional[dict] = None) -> bytes:
    """The SSD-Inception-v2 engine image (inception.py): one op per layer, module branches written by channel slice into the module
    tensors, the separable stem folded into one dense 7x7 conv (OP_STEM7).  `-p 16`: fp16 weights and tensors, fp32 sums (the plain
    fp16 program: 3.2e-4 of the scores on the CPU emulation); `-p 32`: fp32 throughout, input as a hi + lo pair."""
    if precision not in (16, 32):
        raise ValueError("precision must be 16 or 32")
    if model_width != model_height:
        raise ValueError("square model input expected")
    cfg, opt = _post_options(post, options)
    prog = inception.build(model_width, input_pair=precision == 32, head_ks=head_kernel_sizes(weights))
    _check_variables(prog, weights)
    tensor_names = ["input"] + list(dict.fromkeys(op.dst for op in prog.ops if op.out_mode == arch.OUT_ACT))
    tindex = {n: i for i, n in enumerate(tensor_names)}
    slots = assign_slots(prog, tensor_names)
    wblob = bytearray()

    def put(arr: np.ndarray) -> int:
        off = _align(len(wblob))
        wblob.extend(b"\0" * (off - len(wblob)))
        wblob.extend(arr.tobytes())
        return off

    op_recs = []
    for op in prog.ops:
        mb = dict(cmid=0, cin0=0, kc0=0, cmid_pad=0, nmid_pad=0, we_off=0, be_off=0, wd_off=0, bd_off=0, stem=0, stem_pad=0)
        n_pad, kc, w_off, b_off = 0, 0, 0, 0
        if op.kind == arch.OP_POOL:
            mb["flags"] = 0 if op.pool_max else POOL_AVG
        elif op.kind == arch.OP_STEM7:
            w, b = fold_batch_norm(weights, op)                      # dense [7,7,3,64]
            if precision == 32:                                      # fp32 [tap][c][cout]: the direct kernel (k_inception.hip)
                w_off = put(w.reshape(op.k * op.k * op.cin, op.cout).astype(np.float32))
            else:                                                    # one tap, K = tap * 4 + c in 7 chunks of 32
                n_pad, kc = op.cout, STEM7_KC
                w_off = put(pack_conv_weights(stem7_k_rows(w).reshape(1, 1, STEM7_KC * 32, op.cout).astype(np.float32), n_pad, kc))
            b_off = put(b.astype(np.float32))
        else:
            w, b = fold_batch_norm(weights, op)
            n_pad = _align(op.cout, 64 if op.cout >= 256 else 32)
            if precision == 32:
                kc = (op.cin + 15) // 16
                w_off = put(pack_conv_weights_f32(w.astype(np.float32), n_pad, kc))
            else:
                kc = (op.cin + 31) // 32
                w_off = put(pack_conv_weights(w.astype(np.float32), n_pad, kc))
            bp = np.zeros(n_pad, np.float32)
            bp[:op.cout] = b
            b_off = put(bp)
        op_recs.append(_op_record(op, tindex, n_pad, kc, w_off, b_off, mb))
    return _write_image(prog, precision, model_width, cfg, opt, tensor_names, slots, op_recs, wblob, 0)


def build_mobilenet_v1_engine(weights: Dict[str, np.ndarray], precision: int = 16, model_width: int = 300, model_height: int = 300,
                              post: Optional[dict] = None, options: Optional[dict] = None, fuse: bool = True) -> bytes:
    """The SSD-MobileNet-v1 engine image (mobilenet_v1.py).  `-p 16`: fp16 weights and tensors, fp32 sums (the plain fp16 program,
    DESIGN.md section 13); fuse=True packs every separable layer as one OP_DWSEP (depthwise weights in the OP_DW layout at wd_off /
    bd_off, pointwise weights in the OP_CONV layout at w_off / b_off), fuse=False one op per layer.  `-p 32`: fp32 throughout, one op
    per layer, input as a hi + lo pair."""
    if precision not in (16, 32):
        raise ValueError("precision must be 16 or 32")
    if model_width != model_height:
        raise ValueError("square model input expected")
    cfg, opt = _post_options(post, options)
    prog = mobilenet_v1.build(model_width, input_pair=precision == 32, head_ks=head_kernel_sizes(weights),
                              fuse=fuse and precision == 16)
    _check_variables(prog, weights)
    tensor_names = ["input"] + [op.dst for op in prog.ops if op.out_mode == arch.OUT_ACT]
    tindex = {n: i for i, n in enumerate(tensor_names)}
    slots = assign_slots(prog, tensor_names)
    wblob = bytearray()

    def put(arr: np.ndarray) -> int:
        off = _align(len(wblob))
        wblob.extend(b"\0" * (off - len(wblob)))
        wblob.extend(arr.tobytes())
        return off

    def put_conv(op):
        w, b = fold_batch_norm(weights, op)
        n_pad = _align(op.cout, 64 if op.cout >= 256 else 32)
        if precision == 32:
            kc = (op.cin + 15) // 16
            w_off = put(pack_conv_weights_f32(w.astype(np.float32), n_pad, kc))
        else:
            kc = (op.cin + 31) // 32
            w_off = put(pack_conv_weights(w.astype(np.float32), n_pad, kc))
        bp = np.zeros(n_pad, np.float32)
        bp[:op.cout] = b
        return w_off, put(bp), n_pad, kc

    def put_dw(op):
        w, b = fold_batch_norm(weights, op)
        return put(w.reshape(9, op.cin).astype(np.float32 if precision == 32 else np.float16)), put(b.astype(np.float32))

    op_recs = []
    for op in prog.ops:
        mb = dict(cmid=0, cin0=0, kc0=0, cmid_pad=0, nmid_pad=0, we_off=0, be_off=0, wd_off=0, bd_off=0, stem=0, stem_pad=0)
        n_pad, kc = 0, 0
        if op.kind == arch.OP_STEM:
            w, b = fold_batch_norm(weights, op)
            w_off, b_off = put(w.reshape(27, 32).astype(np.float32)), put(b.astype(np.float32))
        elif op.kind == arch.OP_DW:
            w_off, b_off = put_dw(op)
        elif op.kind == arch.OP_DWSEP:
            dw, pw = op.parts
            mb["wd_off"], mb["bd_off"] = put_dw(dw)
            w_off, b_off, n_pad, kc = put_conv(pw)
        else:
            w_off, b_off, n_pad, kc = put_conv(op)
        op_recs.append(_op_record(op, tindex, n_pad, kc, w_off, b_off, mb))
    return _write_image(prog, precision, model_width, cfg, opt, tensor_names, slots, op_recs, wblob, 0)


# The `-p 16` program's score tolerance (1e-3 against the fp32 detector) was established on weights whose channels all live at one
# scale.  Folding a TRAINED network's BatchNorm spreads the per-channel amplitudes of the expanded tensors over a decade or more, and
# the fp16 / unorm16 stages of the default program then lose the tolerance (tools/err_budget.py with SPREAD=..., profiles/r03_err_budget_*:
# 5e-4 at 0.2 decades, 9e-4 at 0.5, 1.9e-3 at 1.0, 3e-3 at 1.5, 1.2e-2 at 2.0).  The ROBUST program (all 17 blocks on the split-operand
# kernel, expanded tensors as unorm16 of sqrt(x / 6)) holds it further out: 2.4e-4 on the seeded weights, 7e-4 at 1.5 decades, 9e-4 at
# 2.0 (tools/robust_check.py on the GPU, tools/err_budget.py plan hp16q), for about a tenth of the throughput.  `channel_spread_decades`
# is the measure the builder reports; `--robust auto` picks the program by it.
SPREAD_VALIDATED_DECADES = 0.45
ROBUST_VALIDATED_DECADES = 1.5


def channel_spread_decades(weights: Dict[str, np.ndarray]) -> float:
    """Median over the network's expand convolutions (and the stem) of log10(p95 / p5) of the per-output-channel amplitude of
    the BatchNorm-folded layer, sqrt(sum w^2 + b^2): ~0.2 for He-initialised weights, d for `synth.spread_channel_scales(W, d)`.
    SSD-Inception-v2 weights: the same measure over all of that network's BatchNorm-ReLU6 convolutions, the stem included; SSD-MobileNet-v1
    weights: over its BatchNorm-ReLU6 convolutions (stem, pointwise layers, extras)."""
    family = detect_family(weights)
    inc = family in ("InceptionV2", "MobilenetV1")
    prog = inception.build() if family == "InceptionV2" else mobilenet_v1.build(fuse=False) if inc else arch.build(fuse=False)
    spreads = []
    for op in prog.ops:
        if op.kind in (arch.OP_CONV, arch.OP_STEM, arch.OP_STEM7) and op.act == arch.ACT_RELU6 and op.has_bn and \
                (inc or op.scope.endswith("/expand") or op.scope.endswith("MobilenetV2/Conv")):
            w, b = fold_batch_norm(weights, op)
            amp = np.sqrt((w.reshape(-1, w.shape[-1]) ** 2).sum(0) + b ** 2)
            lo, hi = np.percentile(amp, [5, 95])
            spreads.append(float(np.log10(max(hi, 1e-30) / max(lo, 1e-30))))
    return float(np.median(spreads)) if spreads else 0.0


def save_engine(engine: bytes, engine_dest_path: str) -> None:
    """watsor/engine.py:54-58."""
    os.makedirs(os.path.dirname(os.path.abspath(engine_dest_path)), exist_ok=True)
    tmp = engine_dest_path + ".tmp%d" % os.getpid()
    with open(tmp, "wb") as f:
        f.write(engine)
    os.replace(tmp, engine_dest_path)


def load_model(model_path: str):
    """(variables, settings): settings = what a frozen graph says about its own pre- / post-processing (empty for .npz)."""
    if model_path.endswith(".pb") and os.path.isfile(model_path):
        from .frozen_graph import read_frozen_graph_model
        return read_frozen_graph_model(model_path)
    return load_weights(model_path), {}


def load_weights(model_path: str) -> Dict[str, np.ndarray]:
    if model_path.startswith("synthetic_mobilenet_v1"):
        from .synth import synthetic_mobilenet_v1
        return synthetic_mobilenet_v1(int(model_path.split(":")[1]) if ":" in model_path else 1234)
    if model_path.startswith("synthetic_inception_v2"):
        from .synth import synthetic_inception_v2
        return synthetic_inception_v2(int(model_path.split(":")[1]) if ":" in model_path else 1234)
    if model_path.startswith("synthetic"):
        from .synth import synthetic_weights
        seed = int(model_path.split(":")[1]) if ":" in model_path else 1234
        return synthetic_weights(seed)
    if not os.path.isfile(model_path):
        raise FileNotFoundError(model_path)
    ext = os.path.splitext(model_path)[1].lower()
    if ext == ".npz":
        with np.load(model_path) as z:
            return {k: z[k] for k in z.files}
    if ext == ".pb":
        from .frozen_graph import read_frozen_graph_variables
        return read_frozen_graph_variables(model_path)
    raise AssertionError("Unsupported model format")          # watsor/engine.py:44


def main(argv=None) -> int:
    parser = argparse.ArgumentParser(description="Utility to build the MI355X engine prior to inference.",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("-i", "--input", dest="model_path", metavar="MODEL_PATH", required=True,
                        help="TF variables as .npz or a frozen_inference_graph.pb of SSD-MobileNet-v2, SSD-Inception-v2 or "
                             "SSD-MobileNet-v1, or synthetic[:seed] (MobileNet-v2) / synthetic_inception_v2[:seed] / "
                             "synthetic_mobilenet_v1[:seed]")
    parser.add_argument("-p", "--precision", type=int, choices=[32, 16], default=16,
                        help="activation/weight storage precision of the engine")
    parser.add_argument("-w", "--workspace", default=1024, type=int,
                        help="accepted for command-line compatibility with watsor/engine.py; unused")
    parser.add_argument("-mw", "--model-width", type=int, default=300, help="model image width")
    parser.add_argument("-mh", "--model-height", type=int, default=300, help="model image height")
    parser.add_argument("-o", "--output", dest="engine_path", help="path of the output file",
                        default=os.path.join(os.getcwd(), "model", "mi355x.bin"))
    parser.add_argument("--resize", choices=sorted(RESIZE_MODES), default=None,
                        help="coordinate rule of the bilinear resize: legacy = TF1 ResizeBilinear(align_corners=False), the 2018 graph; "
                             "half_pixel = half_pixel_centers=True of later exporters (default: what the .pb says, else legacy)")
    parser.add_argument("--clip-after-nms", action="store_true",
                        help="run the per-class NMS on the unclipped boxes and clip what it selected (later Object Detection API "
                             "exporters) instead of clipping first (the 2018 graph)")
    parser.add_argument("--robust", choices=["auto", "on", "off"], default="auto",
                        help="-p 16 only: the program for weights whose channels live at very different scales (a folded trained BatchNorm): "
                             "all 17 blocks with split fp16 operands, expanded tensors stored as square roots.  About 10 %% slower; keeps "
                             "the scores within 1e-3 of the fp32 detector where the default program is at 2e-3 .. 1e-2.  auto (default): "
                             "chosen when the per-channel dynamic range of the folded weights exceeds %.2f decades" % SPREAD_VALIDATED_DECADES)
    parser.add_argument("--precision-check", choices=["warn", "error", "off"], default="warn",
                        help="-p 16 only: what to do when the per-channel dynamic range of the BatchNorm-folded weights exceeds what the "
                             "chosen program's 1e-3 score tolerance was validated for")
    parser.add_argument("--plain-fp16", action="store_true",
                        help="-p 16 only: one fp16 rounding per operand everywhere (about 1.3x faster; scores then differ "
                             "from the fp32 detector by up to 3e-3 instead of staying within 1e-3)")
    args = parser.parse_args(argv)
    print("Building MI355X engine from {}.".format(args.model_path))
    weights, settings = load_model(args.model_path)
    options = {"clip_after_nms": True} if args.clip_after_nms else {}
    if args.resize:
        options["resize"] = args.resize
    post, options = apply_graph_settings(settings, args.model_width, args.model_height, None, options)
    if settings:
        print("Settings read from the graph: " + ", ".join("%s=%s" % (k, v) for k, v in sorted(settings.items()) if k != "anchor_vectors"))
    family = detect_family(weights)
    print("Network: %s (FeatureExtractor/%s/)." % (FAMILIES[family], family))
    if family in ("InceptionV2", "MobilenetV1"):
        if args.robust == "on" or args.plain_fp16:
            raise ValueError("--robust on and --plain-fp16 select SSD-MobileNet-v2 programs; an %s engine is built with "
                             "-p 16 (fp16, scores within 1e-3 of the fp32 detector on He-scaled weights) or -p 32" % FAMILIES[family])
        if args.precision == 16 and args.precision_check != "off":
            spread = channel_spread_decades(weights)
            print("Per-channel dynamic range of the folded convolutions: %.2f decades (the -p 16 program's 1e-3 score tolerance is "
                  "validated up to %.2f)." % (spread, SPREAD_VALIDATED_DECADES))
            if spread > SPREAD_VALIDATED_DECADES:
                msg = ("these weights spread their channels over %.2f decades: the -p 16 engine's scores may differ from the fp32 "
                       "detector's by more than 1e-3; build with -p 32 if that tolerance matters" % spread)
                if args.precision_check == "error":
                    raise ValueError(msg)
                print("WARNING: " + msg, file=sys.stderr)
        engine = build_engine(weights, args.precision, args.model_width, args.model_height, post=post, options=options)
        save_engine(engine, args.engine_path)
        print("MI355X engine saved to {} ({:.1f} MB)".format(args.engine_path, len(engine) / 1e6))
        return 0
    robust = args.robust == "on"
    if args.precision == 16 and not args.plain_fp16 and (args.precision_check != "off" or args.robust == "auto"):
        spread = channel_spread_decades(weights)
        if args.robust == "auto":
            robust = spread > SPREAD_VALIDATED_DECADES
        limit = ROBUST_VALIDATED_DECADES if robust else SPREAD_VALIDATED_DECADES
        print("Per-channel dynamic range of the folded expand layers: %.2f decades -> the %s -p 16 program (its 1e-3 score tolerance is "
              "validated up to %.2f)." % (spread, "robust" if robust else "default", limit))
        if spread > limit and args.precision_check != "off":
            msg = ("these weights spread their channels over %.2f decades: expect score differences %s against the fp32 detector from "
                   "this engine; build with %s-p 32 (scores within 1e-5, about a quarter of the throughput) if the 1e-3 tolerance matters"
                   % (spread, "around 1e-3" if robust else "of 2e-3 .. 1e-2", "" if robust else "--robust on (within 1e-3 up to %.1f decades, 10 %% slower) or " % ROBUST_VALIDATED_DECADES))
            if args.precision_check == "error":
                raise ValueError(msg)
            print("WARNING: " + msg, file=sys.stderr)
    if robust and (args.precision != 16 or args.plain_fp16):
        raise ValueError("--robust on is a -p 16 program (and not the --plain-fp16 one)")
    engine = build_engine(weights, args.precision, args.model_width, args.model_height, post=post,
                          hp_upto=-1 if args.plain_fp16 else None, options=options, robust=robust)
    save_engine(engine, args.engine_path)
    print("MI355X engine saved to {} ({:.1f} MB)".format(args.engine_path, len(engine) / 1e6))
    return 0


if __name__ == "__main__":
    sys.exit(main())
