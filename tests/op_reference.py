"""The float64 reference of ONE op of an engine program, the bound on what an fp32-accumulating kernel may differ from it, and the
walker that checks every op of a program on the tensors an engine actually produced (tests/test_op_reference_cpu.py,
tests/test_gpu_op_conformance.py).

The method is op-local: an op's reference is computed from the source tensor *as the engine stored it*, with the engine's own
rounded weights, so upstream error cancels and what is left is the kernel's fp32 summation order and one final rounding.

For every output element `reference()` returns
  ref  the exact value (float64),
  T    the sum of the absolute values of every term that entered it (|w.x| over taps and channels, + |bias|, + |residual|),
  r    the number of fp32 roundings on the way: terms + 2 where the products are exact in fp32 (fp16 x fp16), 2 * terms + 2 where they
       are not (fp32 weights); terms = the in-image taps x input channels; the average pool has one more (the multiplication by 1 / taps).
With u = 2^-24:
  e_acc = min(8 sqrt(r), r) u T          r u T is the worst case of ANY summation order (split-K and grouped reduces included);
                                         8 sqrt(r) u T the probabilistic bound for round-to-nearest sums (Higham & Mary 2019), exceeded
                                         with probability below 2 exp(-32) per element
  tol   = e_acc + ulp16(|ref| + e_acc) / 2     stored as fp16
  tol   = e_acc                                stored as fp32 (the last rounding is one of the r)
ReLU6 is 1-Lipschitz, so the bound passes through it.  None of these numbers comes from a kernel.

Exact where the order is a contract: max pool (no arithmetic), and the `-p 16` depthwise conv, whose kernels state their order (the sum
starts from the fp32 bias and runs fmaf over ky, then kx; an fp16 x fp16 product is exact in fp32, so float32(acc + x * k) IS that
fmaf): emulated in float32 and compared value for value (a signed zero is the one thing `==` does not tell apart).

Weights come from the model variables through engine.fold_batch_norm and are rounded as the packer rounds them, so a wrong weight
layout in the engine image shows up as a wrong tensor.

A fused inverted-residual block (OP_MBCONV) is one op with three stages and two roundings that never reach HBM (the chunk buffer, the
depthwise output): `block_reference` chains the three float64 stages on the halves the engine stored and carries a worst-case radius and
a sum of squared radii through them (its docstring has the derivation); `pair_checks` holds what needs no tolerance.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from watsor_amd import arch, engine

U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------------------
def ulp16(x):
    """Spacing of fp16 numbers at |x| (2^-24 in the subnormal range)."""
    _, e = np.frexp(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14))     # x = m 2^e, m in [0.5, 1): floor(log2 x) = e - 1
    return np.ldexp(1.0, e - 11)


def e_acc(T, r):
    r = np.asarray(r, np.float64)
    return np.minimum(8.0 * np.sqrt(r), r) * U * np.asarray(T, np.float64)


def tolerance(ref, T, r, fp16_store: bool):
    e = e_acc(T, r)
    return e + 0.5 * ulp16(np.abs(ref) + e) if fp16_store else e


# ---------------------------------------------------------------------------------------------------------------------------------
# weights as the engine holds them
# ---------------------------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _f16_via_f32(a):          # pack_conv_weights: float64 -> float32 -> float16
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float16).astype(np.float64)


def _f16(a):                  # the depthwise taps: float64 -> float16
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def engine_weights(op: "arch.Op", weights: Dict[str, np.ndarray], precision: int, exact: bool = False):
    """(w float64 in TF layout, bias float64) of one conv op, BatchNorm folded, rounded as the packer rounds them (exact=True: not
    rounded at all).  `split_w`: K = [hi halves | lo halves] along the input channels."""
    w, b = engine.fold_batch_norm(weights, op)
    if op.split_w:
        if exact:
            w = np.concatenate([w, np.zeros_like(w)], axis=2)
        else:
            hi, lo = engine.split_halves(w)
            w = np.concatenate([hi, lo], axis=2)
    if exact:
        return w, b
    if precision == 32 or op.kind == arch.OP_STEM:
        w = _f32(w)
    elif op.kind == arch.OP_DW:
        w = _f16(w)
    else:
        w = _f16_via_f32(w)
    return w, _f32(b)


# ---------------------------------------------------------------------------------------------------------------------------------
# plain float64 ops, NHWC in and out
# ---------------------------------------------------------------------------------------------------------------------------------
def _pads(n_in: int, k: int, s: int, before: int):
    n_out = (n_in + s - 1) // s
    return n_out, max((n_out - 1) * s + k - n_in - before, 0)


def _padded(x: np.ndarray, k: int, s: int, pad_t: int, pad_l: int, value: float = 0.0) -> np.ndarray:
    n, h, w, c = x.shape
    _, pb = _pads(h, k, s, pad_t)
    _, pr = _pads(w, k, s, pad_l)
    return np.pad(x, ((0, 0), (pad_t, pb), (pad_l, pr), (0, 0)), constant_values=value)


def _windows(xp: np.ndarray, k: int, s: int, hout: int, wout: int):
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, xp[:, ky:ky + (hout - 1) * s + 1:s, kx:kx + (wout - 1) * s + 1:s, :]


def in_image_taps(h: int, w: int, k: int, s: int, pad_t: int, pad_l: int) -> np.ndarray:
    """[hout, wout]: how many of the k x k taps of each output pixel lie inside the image."""
    ones = _padded(np.ones((1, h, w, 1)), k, s, pad_t, pad_l)
    hout, wout = (h + s - 1) // s, (w + s - 1) // s
    return sum(win for _, _, win in _windows(ones, k, s, hout, wout))[0, :, :, 0]


def conv64(x: np.ndarray, w: np.ndarray, stride: int, pad_t: int, pad_l: int, depthwise: bool = False) -> np.ndarray:
    """x [n,h,w,cin], w [k,k,cin,cout] (depthwise: [k,k,c,1]), TF SAME with the given leading pads -> [n,hout,wout,cout], float64."""
    k = w.shape[0]
    xp = torch.from_numpy(np.ascontiguousarray(_padded(np.asarray(x, np.float64), k, stride, pad_t, pad_l).transpose(0, 3, 1, 2)))
    wt = torch.from_numpy(np.ascontiguousarray(np.asarray(w, np.float64).transpose((2, 3, 0, 1) if depthwise else (3, 2, 0, 1))))
    y = F.conv2d(xp, wt, None, stride=stride, groups=x.shape[3] if depthwise else 1)
    return np.ascontiguousarray(y.permute(0, 2, 3, 1).numpy())


def _act(y: np.ndarray, act: int) -> np.ndarray:
    return np.clip(y, 0.0, 6.0) if act == arch.ACT_RELU6 else y


def depthwise_fp32_emulated(x: np.ndarray, w: np.ndarray, b: np.ndarray, stride: int, pad_t: int, pad_l: int, act: int) -> np.ndarray:
    """The `-p 16` depthwise kernels' arithmetic: acc = bias (fp32); acc = fmaf(x, k, acc) over ky, then kx; ReLU6 -- float32, before
    the fp16 rounding.  x and w hold fp16 values, so x * k is exact in float64 and float32(acc + x * k) is the fmaf; a tap outside the
    image adds an exact zero."""
    n, h, wd, c = x.shape
    hout, wout = (h + stride - 1) // stride, (wd + stride - 1) // stride
    xp = _padded(np.asarray(x, np.float64), 3, stride, pad_t, pad_l)
    acc = np.broadcast_to(np.asarray(b, np.float32), (n, hout, wout, c)).copy()
    for ky, kx, win in _windows(xp, 3, stride, hout, wout):
        acc = (acc.astype(np.float64) + win * w[ky, kx, :, 0]).astype(np.float32)
    return np.clip(acc, np.float32(0), np.float32(6)) if act == arch.ACT_RELU6 else acc


@dataclass
class OpResult:
    ref: np.ndarray                       # [n, hout, wout, cout] float64; exact ops: the value to compare after the cast to the stored type
    T: Optional[np.ndarray] = None
    r: Optional[np.ndarray] = None        # broadcastable against ref
    exact: bool = False


def _dense(op, w, b, x, res, inexact_products: bool, want_T: bool, stride=None, pad_t=None, pad_l=None) -> OpResult:
    stride = op.stride if stride is None else stride
    pad_t = op.pad_t if pad_t is None else pad_t
    pad_l = op.pad_l if pad_l is None else pad_l
    depthwise = op.kind == arch.OP_DW
    y = _act(conv64(x, w, stride, pad_t, pad_l, depthwise) + b, op.act)
    if res is not None:
        y = y + np.asarray(res, np.float64)       # the residual is added after the activation (wz_epilogue4)
    if not want_T:
        return OpResult(y)
    T = conv64(np.abs(x), np.abs(w), stride, pad_t, pad_l, depthwise) + np.abs(b)
    if res is not None:
        T = T + np.abs(np.asarray(res, np.float64))
    terms = in_image_taps(x.shape[1], x.shape[2], w.shape[0], stride, pad_t, pad_l)[None, :, :, None] * (1 if depthwise else w.shape[2])
    return OpResult(y, T, (2 if inexact_products else 1) * terms + 2)


def reference(op: "arch.Op", weights: Dict[str, np.ndarray], src: np.ndarray, res: Optional[np.ndarray] = None, precision: int = 16,
              exact: bool = False) -> OpResult:
    """The float64 reference of `op` on `src` ([n,h,w,c], the values as stored; the network input may carry its zero fourth channel).
    exact=True: weights and biases stay float64, nothing is emulated, no T (the float64 network of the oracle comparison)."""
    x = np.asarray(src, np.float64)
    want_T = not exact
    if op.kind == arch.OP_POOL:
        hout, wout = (x.shape[1] + op.stride - 1) // op.stride, (x.shape[2] + op.stride - 1) // op.stride
        if op.pool_max:                                         # padding never wins
            xp = _padded(x, op.k, op.stride, op.pad_t, op.pad_l, -np.inf)
            y = None
            for _, _, win in _windows(xp, op.k, op.stride, hout, wout):
                y = win.copy() if y is None else np.maximum(y, win)
            return OpResult(y, exact=True)
        taps = in_image_taps(x.shape[1], x.shape[2], op.k, op.stride, op.pad_t, op.pad_l)[None, :, :, None]
        s = sum(win for _, _, win in _windows(_padded(x, op.k, op.stride, op.pad_t, op.pad_l), op.k, op.stride, hout, wout))
        if not want_T:
            return OpResult(s / taps)
        sa = sum(win for _, _, win in _windows(_padded(np.abs(x), op.k, op.stride, op.pad_t, op.pad_l), op.k, op.stride, hout, wout))
        return OpResult(s / taps, sa / taps, taps + 3)
    if op.kind == arch.OP_DWSEP:
        dw, pw = op.parts
        wd, bd = engine_weights(dw, weights, precision, exact)
        wp, bp = engine_weights(pw, weights, precision, exact)
        if exact:
            mid = _dense(dw, wd, bd, x, None, False, False, op.stride, op.pad_t, op.pad_l).ref
        else:                                                   # what the kernel keeps in LDS: the emulated depthwise output as fp16
            mid = depthwise_fp32_emulated(x, wd, bd, op.stride, op.pad_t, op.pad_l, dw.act).astype(np.float16).astype(np.float64)
        return _dense(pw, wp, bp, mid, None, False, want_T, 1, 0, 0)
    w, b = engine_weights(op, weights, precision, exact)
    if op.kind in (arch.OP_STEM, arch.OP_STEM7):
        x = x[..., :3]                                          # channel 3 of the input is ignored
        if w.shape[2] != 3:
            raise AssertionError("%s: stem weights with %d input channels" % (op.scope, w.shape[2]))
        return _dense(op, w, b, x, None, precision == 32 or op.kind == arch.OP_STEM, want_T)
    if op.kind == arch.OP_DW:
        if precision == 16 and not exact:
            return OpResult(depthwise_fp32_emulated(x, w, b, op.stride, op.pad_t, op.pad_l, op.act).astype(np.float64), exact=True)
        return _dense(op, w, b, x, None, True, want_T)
    if op.kind == arch.OP_CONV:
        if w.shape[2] != x.shape[3]:
            raise AssertionError("%s: K = %d over a %d-channel source" % (op.scope, w.shape[2], x.shape[3]))
        return _dense(op, w, b, x, res, precision == 32, want_T)
    raise AssertionError("no reference for op kind %d (%s)" % (op.kind, op.scope))


# ---------------------------------------------------------------------------------------------------------------------------------
# one fused inverted-residual block (OP_MBCONV)
# ---------------------------------------------------------------------------------------------------------------------------------
FORM_FP16, FORM_UNORM16, FORM_FLOAT = "fp16", "unorm16", "float16bit"
FLOAT_FORM_UPTO = 9          # engine.build_engine's default float_form_upto: the robust program's blocks 0 .. 9


def chunk_form(op: "arch.Op", float_form_upto: int = -1) -> str:
    """How the block keeps its expanded tensor in LDS: fp16 (plain blocks), unorm16 of z = relu6(v) / 6, or the 16-bit float form."""
    if not op.hp:
        return FORM_FP16
    return FORM_FLOAT if op.block <= float_form_upto else FORM_UNORM16


def float_form_step(z):
    """Spacing of the 16-bit float form of k_hp_ops.h at z in [0, 1]: the code is bits 10 .. 25 of the fp32 pattern of t = z T,
    T = 2^-120 (2 - 2^-13) -- 13 mantissa bits in the normal binades (t >= 2^-126: a relative step of 2^-13, z >= 2^-7), the fp32
    subnormal spacing 2^-149 * 2^10 below (2^-20 of full scale)."""
    t = np.clip(np.asarray(z, np.float64), 0.0, 1.0) * engine.FLOAT_FORM_T
    _, e = np.frexp(np.maximum(t, 2.0 ** -126))
    return np.ldexp(1.0 / engine.FLOAT_FORM_T, e - 14)


def pair_store_radius(v):
    """hi = RN16(v), lo = RN16(v - hi) (v - hi is exact in fp32): hi + lo misses v by at most half an ulp16 of the remainder, which is
    itself at most half an ulp16 of v."""
    return 0.5 * ulp16(0.5 * ulp16(v))


@dataclass
class BlockResult:
    ref: np.ndarray                       # [n, hout, wout, cout] float64: the block's output
    tol: np.ndarray
    acc: np.ndarray                       # the part of tol that is not the final store (min(8 sqrt V, W) + the lo-half term)
    store: str                            # "pair", "fp16" or "dup"
    ref2: Optional[np.ndarray] = None     # dst2: the expanded tensor [n, hin, win, cmid] as plain fp16
    tol2: Optional[np.ndarray] = None
    acc2: Optional[np.ndarray] = None


def _mm(x, w):
    return np.asarray(x, np.float64) @ np.asarray(w, np.float64)


def _dw(x, w, stride, pad_t, pad_l):
    """depthwise 3x3 of [n,h,w,c] with taps w [3,3,c], zeros outside the frame."""
    return conv64(x, w[..., None], stride, pad_t, pad_l, depthwise=True)


def block_weights(op: "arch.Op", weights: Dict[str, np.ndarray], form: str):
    """The three stages' weights as engine.build_engine packs them, float64.  -> dict:
    e_hi, e_lo [k,k,cin,cmid] and e_b (None without an expand stage; split-operand blocks: of w / 6, b / 6), d_w [3,3,cmid] in the units
    of the chunk buffer's VALUE (z for the 16-bit codes, v for fp16), d_b, p_hi, p_lo [cmid,cout], p_b."""
    parts = list(op.parts)
    out = dict(e_hi=None, e_lo=None, e_b=None)
    if op.stem or op.cin0:
        ex = parts.pop(0)
        w, b = engine.fold_batch_norm(weights, ex)
        if op.hp:                                               # 1 / 6 folded in, then split; the bias as fp32
            out["e_hi"], out["e_lo"] = engine.split_halves(w / 6.0)
            out["e_b"] = _f32(b / 6.0)
        else:
            out["e_hi"], out["e_lo"], out["e_b"] = _f16_via_f32(w), np.zeros_like(w), _f32(b)
    dw, pj = parts
    wd, bd = engine.fold_batch_norm(weights, dw)
    wd = wd[..., 0]
    if form == FORM_FP16:
        out["d_w"] = _f16(wd)
    elif form == FORM_UNORM16:                                  # the kernel multiplies the CODE (0 .. 65535) by fp32(w * 6 / 65535)
        out["d_w"] = _f32(wd / engine.UNORM16_PER_6) * 65535.0
    else:                                                       # ... the decoded t = z T by fp32(w * 6 * 2^60 / (2 - 2^-13)), the sum by 2^60
        out["d_w"] = _f32(wd * engine.FLOAT_FORM_TAP_SCALE) * (engine.FLOAT_FORM_T * 2.0 ** 60)
    out["d_b"] = _f32(bd)
    w, b = engine.fold_batch_norm(weights, pj)
    w = w[0, 0]
    if op.hp:
        out["p_hi"], out["p_lo"] = engine.split_halves(w)
    else:
        out["p_hi"], out["p_lo"] = _f16_via_f32(w), np.zeros_like(w)
    out["p_b"] = _f32(b)
    return out


def block_reference(op: "arch.Op", weights: Dict[str, np.ndarray], src_hi, src_lo=None, res_hi=None, res_lo=None,
                    form: Optional[str] = None, store: str = "fp16") -> BlockResult:
    """The float64 reference of one fused block and its element-by-element tolerance.

    Inputs as the engine stored them: the source (and residual) as their two fp16 halves (lo None: a plain tensor), summed in float64.
    Weights from the model variables, rounded / split / scaled as engine.build_engine does (block_weights).  The contract (k_mbconv*.hip):
      expand    z = clamp(sum + b, 0, top); split-operand blocks: the sum is Whi.xhi + Whi.xlo + Wlo.xhi in exact arithmetic (Wlo.xlo is
                dropped by design), W and b carry the 1 / 6, top = 1; plain blocks: fp16 operands, top = 6.  The stem block's expand stage
                is the 3x3 stride-2 stem conv on the input.  Halo pixels outside the frame are exact zeros (TF pads the depthwise INPUT).
      buffer    z is kept as fp16, as unorm16 (step 1 / 65535) or in the 16-bit float form (float_form_step)
      depthwise y = relu6(b + sum over the in-frame taps), fp32 taps; kept as hi + lo (split blocks) or one fp16
      project   sum over the expanded channels (three products again), + b, + residual (its halves added in fp32); stored as a pair,
                one fp16, or [hi | hi] (`store`: "pair", "fp16", "dup")
    The bound carries two radii through the stages: W, the worst case, and V, the sum of the squared radii of independent roundings.
    An fp32 accumulation of r roundings over terms of absolute sum T adds r u T to W and r (u T)^2 to V (8 sqrt(V) is then the file's
    8 sqrt(r) u T); r counts three products per term for split operands, one per term otherwise (fp16 x fp16 is exact; the depthwise
    taps are fused multiply-adds), + 2 for bias and the last rounding, + 1 for the multiplication by T (float form) / by 2^60 (its tap
    sum), + 2 for a residual (its halves' sum, then the add).  A storage step adds its radius h -- taken at |ref| + W so far -- to W and
    h^2 to V: half a step for fp16, hi + lo and the float form (wz_hp_fenc4 adds half of the kept ulp to the pattern and truncates:
    round to nearest by construction), a WHOLE step for unorm16: the codes come from v_cvt_pknorm_u16_f32, and nothing this project can
    cite promises that the instruction rounds to nearest (a truncating conversion is off by up to a step).  A linear stage maps W -> sum |w| W, V -> sum w^2 V;
    the clamp and ReLU6 are 1-Lipschitz.  At the end
        tol = min(8 sqrt(V), W) + L + the final store's radius at |ref| + the rest,
    with the 8 once (2 exp(-32) per element, as everywhere in this file).  L is the one term that is neither: the kernel's Wlo meets
    RN16(y_kernel), the reference's RN16(y_ref); where the two lie on different sides of an fp16 rounding boundary the products differ
    by |Wlo| ulp16(y) -- about 2^-22 |w y| per channel, 4 u T in all and 1 % of the tolerance, added in full.
    Block 13's dst2 (the expanded tensor, an SSD feature map) is checked as the 1x1 conv it is: e_acc + half an ulp16; the split-operand
    kernel stores fp16(6 * z), one more rounding."""
    form = form or chunk_form(op)
    hp = op.hp
    bw = block_weights(op, weights, form)
    xh = np.asarray(src_hi, np.float64)
    xl = np.zeros_like(xh) if src_lo is None else np.asarray(src_lo, np.float64)
    top = 1.0 if hp else 6.0
    nprod = 3 if hp else 1
    ref2 = tol2 = acc2 = None
    # ---- expand
    if bw["e_hi"] is not None:
        whi, wlo, b = bw["e_hi"], bw["e_lo"], bw["e_b"]
        if op.stem:
            xh, xl = xh[..., :3], xl[..., :3]
            st, sl = op.stem_pad
            pre = conv64(xh, whi + wlo, 2, st, sl) + conv64(xl, whi, 2, st, sl) + b
            T1 = conv64(np.abs(xh), np.abs(whi) + np.abs(wlo), 2, st, sl) + conv64(np.abs(xl), np.abs(whi), 2, st, sl) + np.abs(b)
            terms = in_image_taps(xh.shape[1], xh.shape[2], 3, 2, st, sl)[None, :, :, None] * 3
        else:
            whi, wlo = whi[0, 0], wlo[0, 0]
            pre = _mm(xh, whi + wlo) + _mm(xl, whi) + b
            T1 = _mm(np.abs(xh), np.abs(whi) + np.abs(wlo)) + _mm(np.abs(xl), np.abs(whi)) + np.abs(b)
            terms = float(whi.shape[0])
        r1 = nprod * terms + 2 + (1 if form == FORM_FLOAT else 0)
        z = np.clip(pre, 0.0, top)
        W = r1 * U * T1
        V = r1 * (U * T1) ** 2
        if op.dst2:
            scale = 6.0 if hp else 1.0                          # the split-operand kernel stores fp16(6 * z): one more rounding
            ref2 = scale * z
            acc2 = e_acc(scale * T1, r1 + (1 if hp else 0)) * np.ones_like(z)
            tol2 = acc2 + 0.5 * ulp16(ref2 + acc2)
        at = np.minimum(z + W, top)
        h = 0.5 * ulp16(at) if form == FORM_FP16 else 0.5 * float_form_step(at) if form == FORM_FLOAT else np.full_like(z, 1.0 / 65535.0)
        W, V = W + h, V + h * h
    else:                                                       # no expand stage: the depthwise conv reads the stored tensor itself
        if hp:
            raise AssertionError("%s: a split-operand block without an expand stage" % op.scope)
        z, W, V = xh + xl, np.zeros_like(xh), np.zeros_like(xh)
    # ---- depthwise
    wd, bd = bw["d_w"], bw["d_b"]
    s, pt, pl = op.stride, op.pad_t, op.pad_l
    y_pre = _dw(z, wd, s, pt, pl) + bd
    T2 = _dw(np.abs(z), np.abs(wd), s, pt, pl) + np.abs(bd)
    r2 = in_image_taps(z.shape[1], z.shape[2], 3, s, pt, pl)[None, :, :, None] + 2 + (1 if form == FORM_FLOAT else 0)
    W = _dw(W, np.abs(wd), s, pt, pl) + r2 * U * T2
    V = _dw(V, wd * wd, s, pt, pl) + r2 * (U * T2) ** 2
    y = np.clip(y_pre, 0.0, 6.0)
    h = pair_store_radius(y + W) if hp else 0.5 * ulp16(y + W)
    W, V = W + h, V + h * h
    # ---- project
    whi, wlo, b = bw["p_hi"], bw["p_lo"], bw["p_b"]
    if hp:
        yhi = y.astype(np.float16).astype(np.float64)
        ylo = y - yhi
        ref = _mm(y, whi) + _mm(yhi, wlo) + b
        T3 = _mm(np.abs(yhi) + np.abs(ylo), np.abs(whi)) + _mm(np.abs(yhi), np.abs(wlo)) + np.abs(b)
        L = _mm(ulp16(y + W), np.abs(wlo))
    else:
        ref = _mm(y, whi) + b
        T3 = _mm(np.abs(y), np.abs(whi)) + np.abs(b)
        L = 0.0
    r3 = nprod * whi.shape[0] + 2
    if op.res:
        rh = np.asarray(res_hi, np.float64)
        rl = np.zeros_like(rh) if res_lo is None else np.asarray(res_lo, np.float64)
        ref = ref + rh + rl
        T3 = T3 + np.abs(rh) + np.abs(rl)
        r3 += 2
    wsum = whi + wlo
    W = _mm(W, np.abs(wsum)) + r3 * U * T3
    V = _mm(V, wsum * wsum) + r3 * (U * T3) ** 2
    acc = np.minimum(8.0 * np.sqrt(V), W) + L
    last = pair_store_radius(np.abs(ref) + acc) if store == "pair" else 0.5 * ulp16(np.abs(ref) + acc)
    return BlockResult(ref, acc + last, acc, store, ref2, tol2, acc2)


def pair_checks(hi: np.ndarray, lo: np.ndarray):
    """The exact properties of a stored pair tensor ([n,h,w,c] float16 halves) -> list of messages (empty: all hold).
      * both halves finite, |lo| <= ulp16(hi) / 2 (lo = RN16(v - hi) with hi = RN16(v));
      * the lo half is alive: in every (frame, 4 x 4 pixel tile, 16-channel group) with at least eight elements of |hi| >= 2^-10, not
        every lo is zero (a tile that lost its lo half is 2^-12 relative off: far below any bound)."""
    msgs = []
    h64, l64 = hi.astype(np.float64), lo.astype(np.float64)
    if not (np.isfinite(h64).all() and np.isfinite(l64).all()):
        msgs.append("pair halves: not finite")
        return msgs
    bad = np.abs(l64) > 0.5 * ulp16(h64)
    if bad.any():
        at = np.unravel_index(int(np.argmax(bad)), bad.shape)
        msgs.append("pair halves: |lo| > ulp16(hi) / 2 at %d of %d elements, first at %s: hi %.9g lo %.9g"
                    % (int(bad.sum()), bad.size, tuple(int(i) for i in at), h64[at], l64[at]))
    n, h, w, c = hi.shape
    ph, pw, pc = -h % 4, -w % 4, -c % 16
    big = np.pad(np.abs(h64) >= 2.0 ** -10, ((0, 0), (0, ph), (0, pw), (0, pc)))
    nz = np.pad(l64 != 0, ((0, 0), (0, ph), (0, pw), (0, pc)))

    def groups(a):
        return a.reshape(n, (h + ph) // 4, 4, (w + pw) // 4, 4, (c + pc) // 16, 16).sum(axis=(2, 4, 6))

    dead = (groups(big) >= 8) & (groups(nz) == 0)
    if dead.any():
        at = np.unravel_index(int(np.argmax(dead)), dead.shape)
        msgs.append("lo half dead: %d (frame, 4 x 4 tile, 16-channel group) with eight or more |hi| >= 2^-10 and every lo zero, first at "
                    "frame index %d, tile (%d, %d), channels %d .. %d" % (int(dead.sum()), at[0], at[1], at[2], at[3] * 16, at[3] * 16 + 15))
    return msgs


def head_rows(op: "arch.Op", y: np.ndarray):
    """[n,h,w, a*4 | a*91] of an OUT_HEAD op -> (box [n, h*w*a, 4], class [n, h*w*a, 91]): pixel p, anchor a is row p * anchors + a."""
    n = y.shape[0]
    rows = op.hout * op.wout * op.anchors_per_loc
    return y[..., :op.n_box].reshape(n, rows, 4), y[..., op.n_box:].reshape(n, rows, (op.cout - op.n_box) // op.anchors_per_loc)


def run_program(prog: "arch.Program", weights: Dict[str, np.ndarray], x: np.ndarray, precision: int = 32):
    """The float64 network: the references chained with exact=True, each op fed with the unrounded result of the op before.
    -> (tensors name -> [n,h,w,c] float64, box encodings [n,A,4], class logits [n,A,91])."""
    n = x.shape[0]
    T: Dict[str, np.ndarray] = {"input": np.asarray(x, np.float64)}
    be = np.zeros((n, prog.num_anchors, 4))
    lg = np.zeros((n, prog.num_anchors, arch.NUM_CLASSES))
    for op in prog.ops:
        y = reference(op, weights, T[op.src], T[op.res] if op.res else None, precision, exact=True).ref
        if op.out_mode == arch.OUT_HEAD:
            b, c = head_rows(op, y)
            be[:, op.anchor_offset:op.anchor_offset + b.shape[1]] = b
            lg[:, op.anchor_offset:op.anchor_offset + c.shape[1]] = c
        elif op.cdst:
            t = T.setdefault(op.dst, np.zeros(y.shape[:3] + (op.cdst,)))
            t[..., op.coff:op.coff + op.cout] = y
        else:
            T[op.dst] = y
    return T, be, lg


# ---------------------------------------------------------------------------------------------------------------------------------
# the walker
# ---------------------------------------------------------------------------------------------------------------------------------
def op_kind_name(op: "arch.Op", float_form_upto: int = -1) -> str:
    if op.kind == arch.OP_POOL:
        return "pool_max" if op.pool_max else "pool_avg"
    if op.kind == arch.OP_MBCONV:                               # by the kernel family that runs the block
        if not op.hp:
            return "block_plain"
        if chunk_form(op, float_form_upto) == FORM_FLOAT:
            return "block_hp_q"
        return "block_hp2" if (not op.stem and op.wout <= 10) else "block_hp"
    if op.kind != arch.OP_CONV:
        return {arch.OP_STEM: "stem3x3", arch.OP_STEM7: "stem7x7", arch.OP_DW: "depthwise", arch.OP_DWSEP: "dwsep"}[op.kind]
    if op.out_mode == arch.OUT_HEAD:
        return "head%dx%d" % (op.k, op.k)
    return "conv%dx%d%s%s%s%s" % (op.k, op.k, "_s2" if op.stride == 2 else "", "_res" if op.res else "", "_slice" if op.cdst else "",
                                   "_splitw" if op.split_w else "")


@dataclass
class Report:
    ops_checked: int = 0
    blocks_checked: int = 0                                   # the fused blocks (OP_MBCONV) among ops_checked
    ops_mbconv: int = 0                                       # fused blocks passed over: none, they are checked like any other op
    ops_unchecked: int = 0
    elements: int = 0
    worst: Dict[str, tuple] = field(default_factory=dict)     # op kind -> (worst err / tol, op scope)
    worst_acc: Dict[str, float] = field(default_factory=dict)  # op kind -> worst (err - the fp16 store's half ulp) / e_acc: a lower bound on
                                                               # the share of the ACCUMULATION allowance in use (err / tol of an fp16 tensor is
                                                               # near 1 whenever the final rounding lands near half an ulp)
    failures: List[str] = field(default_factory=list)
    subnormal_refs: int = 0                                   # compared elements whose reference is non-zero and below 2^-14 in magnitude
    dead_elements: int = 0                                    # compared elements in the channels `marks` calls dead / saturated
    saturated_elements: int = 0

    def populations(self) -> str:
        return "%d references fp16-subnormal, %d elements in dead channels, %d in saturated channels" % (
            self.subnormal_refs, self.dead_elements, self.saturated_elements)

    def summary(self) -> str:
        kinds = "  ".join("%s %.3g (acc %.3g)" % (k, v[0], self.worst_acc.get(k, 0.0)) for k, v in sorted(self.worst.items()))
        return "%d ops checked (%d of them fused blocks, %d unchecked), %d elements; worst err / tol: %s" % (
            self.ops_checked, self.blocks_checked, self.ops_unchecked, self.elements, kinds)


def _compare(rep: Report, op, idx: int, what: str, got: np.ndarray, ref: np.ndarray, T, r, exact: bool, fp16_store: bool,
             frames: Sequence[int], tol=None, acc=None, kind: Optional[str] = None):
    """got / ref / T [n, ..., c] (any middle axes = the pixel), r broadcastable; records a failure with the worst element.
    tol / acc given (a fused block): the tolerance and its part that is not the final store, element by element, instead of T and r.
    -> (worst err / tol, worst share of e_acc in use)."""
    got64 = got.astype(np.float64)
    acc_share = 0.0
    if exact:
        expected = ref.astype(np.float16 if fp16_store else np.float32).astype(np.float64)
        bad = ~(got64 == expected)
        ratio = np.where(bad, np.inf, 0.0)
        ref = expected
    else:
        if tol is None:
            tol, e = tolerance(ref, T, r, fp16_store), e_acc(T, r)
        else:
            e = acc
        err = np.abs(got64 - ref)
        bad = ~(err <= tol)                                   # (a NaN fails)
        ratio = np.where(bad & ~np.isfinite(err), np.inf, err / np.maximum(tol, 1e-300))
        share = np.where(e > 0, (err - (tol - e)) / np.where(e > 0, e, 1.0), 0.0)
        acc_share = float(np.nanmax(share)) if share.size else 0.0
    if not np.isfinite(got64).all():
        bad = bad | ~np.isfinite(got64)
        ratio = np.where(np.isfinite(got64), ratio, np.inf)
    rep.elements += int(got.size)
    a = np.abs(ref)
    rep.subnormal_refs += int(((a > 0) & (a < 2.0 ** -14)).sum())
    worst = float(ratio.max()) if ratio.size else 0.0
    if bad.any():
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        rep.failures.append("op %d (%s, %s)%s: frame %d, pixel %s, channel %d: got %.9g, ref %.9g, err / tol %.3g%s; %d of %d elements outside"
                            % (idx, op.scope, kind or op_kind_name(op), what, frames[at[0]], tuple(int(i) for i in at[1:-1]), at[-1], got64[at],
                               ref[at], ratio[at], " (exact comparison)" if exact else "", int(bad.sum()), bad.size))
    return worst, max(acc_share, 0.0)


def walk(eng, prog: "arch.Program", weights: Dict[str, np.ndarray], x_half: Optional[np.ndarray], precision: int = 16,
         frames: Optional[Sequence[int]] = None, check: bool = True, float_form_upto: int = -1,
         marks: Optional[Dict[str, dict]] = None, heads: Optional[tuple] = None) -> Report:
    """One forward pass of `eng` (tensors(), stage_forward(), stage_read_tensor(); every tensor must stay readable) on x_half
    [n,S,S,4] float16, then EVERY op of `prog` on its own: source (and residual) as the engine produced them -> ref, tol -> the
    destination the engine produced.  `frames`: the frames whose references are computed (default: all).  float_form_upto: the last
    split-operand block whose chunk buffer holds the 16-bit float form (the robust program: FLOAT_FORM_UPTO).
    A fused block (OP_MBCONV) is an op like any other: block_reference on the stored halves of its source and residual
    (stage_read_tensor(..., halves=True) for the tensors the program marks as pairs), its output -- and block 13's second one, the
    expanded tensor -- against the element-by-element tolerance, and the exact properties of what it stored: pair_checks on a pair
    output, bit-equal halves of a `dup_out` one.
    marks (trained_like.marks): stored tensor -> dead / saturated channel masks and the dead channels' constant.  The elements of
    both kinds are counted; a dead channel of a `-p 16` tensor is compared BIT FOR BIT with its constant fp16(relu6(beta)) (gamma is
    exactly 0, so the weight column is zero in both halves and nothing but the bias reaches the store).
    Counts what it covers and asserts that nothing is left out: every op is checked; every channel of every tensor other than the
    input is written by exactly one checked op; every row of the two head outputs by exactly one head.  check=True raises
    AssertionError naming every failing op; the Report says what was seen.
    heads = (box_enc [n,A,4], logits [n,A,C]): nothing is run here -- the tensors are those of the batch the caller ran on lane 0
    (detect_batch / submit + collect on an engine whose tensors stay readable) and these are its head outputs
    (stage_post_lane(0, n)); x_half is not looked at.  The input tensor is then whatever the resize kernel stored: a pair input's lo
    half is not zero, and every op that reads a pair outside a fused block (the `-p 32` stems) gets hi + lo summed in float64."""
    if heads is None:
        n = x_half.shape[0]
        be, lg = eng.stage_forward(x_half)
    else:
        be, lg = heads
        n = be.shape[0]
        assert lg.shape[0] == n and be.shape[1:] == (prog.num_anchors, 4) and lg.shape[1] == prog.num_anchors
    frames = list(range(n)) if frames is None else sorted(set(int(f) for f in frames))
    assert frames and 0 <= frames[0] and frames[-1] < n
    info = {name: (i, h, w, c) for i, (name, h, w, c) in enumerate(eng.tensors())}
    last_use: Dict[str, int] = {}
    for i, op in enumerate(prog.ops):
        for t in (op.src, op.res, None if op.out_mode == arch.OUT_HEAD else op.dst, op.dst2):
            if t:
                last_use[t] = i
    cache: Dict[str, np.ndarray] = {}
    hcache: Dict[str, tuple] = {}

    def read(name: str) -> np.ndarray:
        if name not in cache:
            cache[name] = np.stack([eng.stage_read_tensor(info[name][0], f) for f in frames])
        return cache[name]

    def halves(name: str):
        """(hi, lo) float16 as stored; lo None for a tensor that is no pair."""
        if not prog.tensors[name].hp:
            return read(name), None
        if name not in hcache:
            hl = [eng.stage_read_tensor(info[name][0], f, halves=True) for f in frames]
            hcache[name] = (np.stack([h for h, _ in hl]), np.stack([l for _, l in hl]))
        return hcache[name]

    def value(name: str) -> np.ndarray:
        """What an op outside the fused blocks reads: a pair as the float64 sum of its stored halves (read() would give the float32
        sum, one rounding that is not the kernel's), any other tensor as stored."""
        if not prog.tensors[name].hp:
            return read(name)
        hi, lo = halves(name)
        return hi.astype(np.float64) + lo.astype(np.float64)

    def record(kind, scope, worst, acc):
        if kind not in rep.worst or worst > rep.worst[kind][0]:
            rep.worst[kind] = (worst, scope)
        rep.worst_acc[kind] = max(rep.worst_acc.get(kind, 0.0), acc)

    def degenerate(idx, op, name, got, c0, c1):
        """got [n,h,w,c1 - c0]: channels c0 .. c1 of the stored tensor `name`, as op `idx` wrote them."""
        m = (marks or {}).get(name)
        if m is None:
            return
        dead, sat = m["dead"][c0:c1], m["saturated"][c0:c1]
        rep.dead_elements += int(dead.sum()) * int(np.prod(got.shape[:3]))
        rep.saturated_elements += int(sat.sum()) * int(np.prod(got.shape[:3]))
        if precision == 16 and dead.any():
            want = np.ascontiguousarray(m["const"][c0:c1][dead]).view(np.uint16)
            have = np.ascontiguousarray(got[..., dead]).view(np.uint16)
            bad = have != want
            if bad.any():
                at = np.unravel_index(int(np.argmax(bad)), bad.shape)
                ch = int(np.flatnonzero(dead)[at[-1]])
                rep.failures.append("op %d (%s, %s) dead channel: %d of %d elements differ from fp16(relu6(beta)), first at frame %d, pixel %s, "
                                    "channel %d: bits 0x%04x, constant 0x%04x" % (idx, op.scope, op_kind_name(op, float_form_upto), int(bad.sum()),
                                                                                  bad.size, frames[at[0]], tuple(int(i) for i in at[1:-1]), ch,
                                                                                  int(have[at]), int(want[at[-1]])))

    rep = Report()
    cover = {name: np.zeros(c, np.int64) for name, (_, _, _, c) in info.items() if name != "input"}
    rows_cover = np.zeros(prog.num_anchors, np.int64)
    for idx, op in enumerate(prog.ops):
        if op.kind == arch.OP_MBCONV:
            kind = op_kind_name(op, float_form_upto)
            store = "dup" if op.dup_out else "pair" if prog.tensors[op.dst].hp else "fp16"
            try:
                sh, sl = halves(op.src)
                rh, rl = halves(op.res) if op.res else (None, None)
                res = block_reference(op, weights, sh, sl, rh, rl, chunk_form(op, float_form_upto), store)
            except AssertionError as e:
                rep.ops_unchecked += 1
                rep.failures.append("op %d (%s): %s" % (idx, op.scope, e))
                continue
            gh, gl = halves(op.dst)
            want_c = 2 * op.cout if store == "dup" else op.cout
            if gh.shape[1:] != res.ref.shape[1:3] + (want_c,) or (store == "pair") != (gl is not None) or \
                    (op.dst2 and read(op.dst2).shape[1:] != res.ref2.shape[1:]):
                rep.failures.append("op %d (%s): the engine's tensor %s is %s%s, the block writes %s x %d as %s"
                                    % (idx, op.scope, op.dst, gh.shape[1:], " (a pair)" if gl is not None else "", res.ref.shape[1:3], want_c, store))
                rep.ops_unchecked += 1
                continue
            exact_msgs = []
            if store == "pair":
                got = gh.astype(np.float64) + gl.astype(np.float64)
                exact_msgs = pair_checks(gh, gl)
            elif store == "dup":
                got = gh[..., :op.cout]
                a, b = np.ascontiguousarray(got).view(np.uint16), np.ascontiguousarray(gh[..., op.cout:]).view(np.uint16)
                if not (a == b).all():
                    exact_msgs = ["[hi | hi]: the two copies differ in %d of %d elements" % (int((a != b).sum()), a.size)]
            else:
                got = gh
            for m in exact_msgs:
                rep.failures.append("op %d (%s, %s) %s" % (idx, op.scope, kind, m))
            cover[op.dst] += 1
            worst, acc = _compare(rep, op, idx, "", got, res.ref, None, None, False, True, frames, tol=res.tol, acc=res.acc, kind=kind)
            record(kind, op.scope, worst, acc)
            if op.dst2:
                cover[op.dst2] += 1
                w2, a2 = _compare(rep, op, idx, " expanded tensor", read(op.dst2), res.ref2, None, None, False, True, frames, tol=res.tol2,
                                  acc=res.acc2, kind="block13_expand")
                record("block13_expand", op.scope, w2, a2)
                degenerate(idx, op, op.dst2, read(op.dst2), 0, op.cmid)
            rep.ops_checked += 1
            rep.blocks_checked += 1
            for c_ in (cache, hcache):
                for t in [t for t in c_ if last_use.get(t, -1) <= idx]:
                    del c_[t]
            continue
        try:
            res = reference(op, weights, value(op.src), value(op.res) if op.res else None, precision)
        except AssertionError as e:
            rep.ops_unchecked += 1
            rep.failures.append("op %d (%s): %s" % (idx, op.scope, e))
            continue
        kind = op_kind_name(op)
        if op.out_mode == arch.OUT_HEAD:
            rb, rc = head_rows(op, res.ref)
            tb, tc = head_rows(op, res.T)
            r = np.repeat(np.broadcast_to(res.r, (1,) + res.ref.shape[1:3] + (1,)).reshape(-1), op.anchors_per_loc)[None, :, None]
            sl = slice(op.anchor_offset, op.anchor_offset + rb.shape[1])
            rows_cover[sl] += 1
            wb = _compare(rep, op, idx, " box encodings", be[frames][:, sl], rb, tb, r, False, False, frames)
            wc = _compare(rep, op, idx, " class logits", lg[frames][:, sl], rc, tc, r, False, False, frames)
            worst, acc = max(wb[0], wc[0]), max(wb[1], wc[1])
        else:
            got = read(op.dst)
            c0, c1 = (op.coff, op.coff + op.cout) if op.cdst else (0, op.cout)
            if got.shape[1:3] != res.ref.shape[1:3] or got.shape[3] != (op.cdst or op.cout):
                rep.failures.append("op %d (%s): the engine's tensor %s is %s, the op writes %s of %d channels"
                                    % (idx, op.scope, op.dst, got.shape[1:], res.ref.shape[1:3], op.cdst or op.cout))
                rep.ops_unchecked += 1
                continue
            cover[op.dst][c0:c1] += 1
            worst, acc = _compare(rep, op, idx, "", got[..., c0:c1], res.ref, res.T, res.r, res.exact, precision == 16, frames)
            degenerate(idx, op, op.dst, got[..., c0:c1], c0, c1)
        rep.ops_checked += 1
        record(kind, op.scope, worst, acc)
        for c_ in (cache, hcache):
            for t in [t for t in c_ if last_use.get(t, -1) <= idx]:
                del c_[t]

    # nothing left out silently
    if rep.ops_checked != len(prog.ops) or rep.ops_unchecked:
        rep.failures.append("coverage: %d ops checked of %d ops (%d unchecked)" % (rep.ops_checked, len(prog.ops), rep.ops_unchecked))
    for name, cnt in cover.items():
        if not (cnt == 1).all():
            rep.failures.append("coverage: tensor %s: channels written by %s checked ops (every channel exactly once expected)"
                                % (name, sorted(set(int(v) for v in cnt))))
    if not (rows_cover == 1).all():
        rep.failures.append("coverage: head rows covered %s times (every one of the %d rows exactly once expected)"
                            % (sorted(set(int(v) for v in rows_cover)), prog.num_anchors))
    if check and rep.failures:
        raise AssertionError("%d failure(s):\n  %s" % (len(rep.failures), "\n  ".join(rep.failures[:20])))
    return rep


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs of the conformance runs
# ---------------------------------------------------------------------------------------------------------------------------------
def impulse_input(size: int, seed: int) -> np.ndarray:
    """[size,size,4] float16 zeros with pixels of 1.0 (all three channels) in the four corners, on each edge, in the centre, and at
    one seeded position more (so that two impulse frames of one batch differ)."""
    x = np.zeros((size, size, 4), np.float16)
    m, e = size // 2, size - 1
    rng = np.random.Generator(np.random.PCG64(seed))
    for y, xx in [(0, 0), (0, e), (e, 0), (e, e), (0, m), (e, m), (m, 0), (m, e), (m, m), tuple(rng.integers(1, e, 2))]:
        x[y, xx, :3] = 1.0
    return x


def noise_input(size: int, seed: int, amplitude: float = 4.0) -> np.ndarray:
    """fp16 noise of the given amplitude (beyond the normalised range [-1, 1]): drives ReLU6 into both clamps."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.zeros((size, size, 4), np.float16)
    x[..., :3] = (rng.uniform(-amplitude, amplitude, (size, size, 3))).astype(np.float16)
    return x


def conformance_batch(n: int, size: int, start: int, seed: int, frame_input) -> np.ndarray:
    """[n,size,size,4] float16, a different input in every frame: frame i is kind (i + start) % 4 of (preprocessed synthetic frame,
    noise, impulses, zeros), each with its own seed; zeros appear once per batch (a second all-zero frame would equal the first: a
    synthetic frame takes its place).  frame_input(seed) -> [size,size,4] float16 is the preprocessed synthetic frame."""
    out = np.zeros((n, size, size, 4), np.float16)
    zeros_used = False
    for i in range(n):
        kind = (i + start) % 4
        s = seed * 100 + i
        if kind == 3 and not zeros_used:
            zeros_used = True
        elif kind == 2:
            out[i] = impulse_input(size, s)
        elif kind == 1:
            out[i] = noise_input(size, s)
        else:
            out[i] = frame_input(s)
    return out


def frame_subset(n: int, all_upto: int = 8) -> List[int]:
    """All frames up to batch `all_upto`; beyond, frame 0, one in the middle and the last."""
    return list(range(n)) if n <= all_upto else [0, n // 2, n - 1]


def old_bound_passes(got: np.ndarray, ref: np.ndarray) -> bool:
    """The end-to-end tests' per-tensor bound for `-p 16` programs: max|got - ref| <= 0.04 max|ref| + 0.02."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.abs(got - ref).max() <= 0.04 * np.abs(ref).max() + 0.02)

