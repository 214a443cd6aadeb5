"""Weights spread the way a trained checkpoint's are, for ANY arch.Program (test infrastructure; watsor_amd/synth.py's
`spread_channel_scales`, which knows the MobileNet-v2 variable names, stays what test_gpu_stress.py and bench.py use).

`trained_like` walks the program's graph, not its variable names.  Every activation tensor other than the input -- the intermediates
of a separable layer, of a fused block and of an Inception branch included -- gets a per-channel factor vector f in (10^-decades, 1],
log-uniform (one value per stratum of the exponent range, in a drawn order, so that a 16-channel tensor covers the range as a
1280-channel one does).  The BatchNorm gamma and beta of the op that produces the tensor are multiplied by f; the weights of every
consumer (heads, the depthwise filter of that channel, the readers of a concat tensor at their channel offset) are divided by it
along their input-channel axis.  Tied vectors: a residual's destination takes its source's vector; a max or average pool passes its
source's vector through (per channel, positively homogeneous); a tensor written by slices holds every writer's vector at the writer's
offset.  Apart from where ReLU6 clips this is the same function of the input.

Two kinds of degenerate channel, on the ReLU6 BatchNorms that have no residual:
  dead       gamma exactly 0.0: the folded weight column is all zeros (both halves of a split one), the output the constant relu6(beta)
  saturated  beta = SATURATED_BETA, gamma times SATURATED_GAMMA, factor 1: the pre-activation is above 6 at nearly every pixel, the output 6 (code 65535, z = 1)
`marks` reads both back from the weights (gamma == 0, beta == SATURATED_BETA) for the tensors a program's engine stores.
"""
from __future__ import annotations

from typing import Dict, Iterator, Optional, Tuple

import numpy as np

from watsor_amd import arch, engine

SATURATED_BETA = np.float32(24.0)
SATURATED_GAMMA = 0.1          # ... and a tenth of the slope: what saturates a trained channel is a large beta against a small gamma
FP16_MIN_NORMAL = 2.0 ** -14


def unit_ops(prog: "arch.Program") -> Iterator[Tuple["arch.Op", str, str, Optional[str], int, int, Optional[str]]]:
    """(op, src, dst, res, coff, cdst, alias) of every single-layer op of `prog`, fused ops (OP_MBCONV, OP_DWSEP) as their parts chained
    one behind the other: a part's output is the tensor `<scope>#<i>` (never stored), the last part writes the fused op's `dst`.
    alias: the stored tensor that holds a copy of dst (block 13's expanded tensor, `dst2`).  A doubled output ([x | x], `dup_out`)
    has the one vector of x, which is also the input-channel axis of the variable its split-weight reader folds."""
    for op in prog.ops:
        if op.kind in (arch.OP_MBCONV, arch.OP_DWSEP):
            cur = op.src
            for i, part in enumerate(op.parts):
                last = i == len(op.parts) - 1
                dst = op.dst if last else "%s#%d" % (op.scope, i)
                expand = op.kind == arch.OP_MBCONV and part.kind in (arch.OP_CONV, arch.OP_STEM) and not last
                yield part, cur, dst, op.res if last else None, 0, 0, op.dst2 if expand else None
                cur = dst
        else:
            yield op, op.src, op.dst, op.res, op.coff, op.cdst, None


def _degenerate(op: "arch.Op", res) -> bool:
    """Does this op's BatchNorm get dead and saturated channels?  ReLU6 BatchNorms without a residual (with one the output is not constant)."""
    return op.has_bn and op.act == arch.ACT_RELU6 and res is None and op.kind != arch.OP_POOL and op.out_mode != arch.OUT_HEAD


def trained_like(weights: Dict[str, np.ndarray], prog: "arch.Program", decades: float, seed: int, dead: float = 0.03,
                 saturated: float = 0.02) -> Dict[str, np.ndarray]:
    """A copy of `weights` (the variables of `prog`) spread over `decades` decades as the module docstring says, with a `dead` share of
    dead and a `saturated` share of saturating channels in every ReLU6 BatchNorm.  Deterministic in (seed, decades): the generator
    draws the order of the strata, the place inside each stratum and the degenerate channels, op by op, and nothing else."""
    rng = np.random.Generator(np.random.PCG64([int(seed), int(round(decades * 1000))]))
    W = {k: np.asarray(v).astype(np.float64) for k, v in weights.items()}
    vec: Dict[str, np.ndarray] = {}

    def factors(c: int) -> np.ndarray:
        e = (rng.permutation(c) + rng.random(c)) / c            # one exponent per stratum: log-uniform, and every tensor spans the range
        return np.power(10.0, -decades * e)

    for op, src, dst, res, coff, cdst, alias in unit_ops(prog):
        fs = vec.get(src)                                        # None: the network input
        if op.kind == arch.OP_POOL:
            out = np.ones(op.cout) if fs is None else fs
        elif op.out_mode == arch.OUT_HEAD:
            if fs is not None:
                for sub in ("BoxEncodingPredictor", "ClassPredictor"):
                    W["%s/%s/weights" % (op.scope, sub)] /= fs[None, None, :, None]
            continue
        else:
            if not op.has_bn:
                raise ValueError("%s: a conv without BatchNorm that is no head" % op.scope)
            name = op.scope + ("/depthwise_weights" if op.kind == arch.OP_DW else "/weights")
            if fs is not None:
                if op.kind == arch.OP_STEM7:
                    raise ValueError("%s: the 7x7 stem reads the network input" % op.scope)
                W[name] /= fs[None, None, :, None]               # (the depthwise filter [k,k,C,1]: channel c's filter by f[c])
            out = vec[res] if res else factors(op.cout)
            gamma, beta = op.scope + "/BatchNorm/gamma", op.scope + "/BatchNorm/beta"
            if _degenerate(op, res):
                order = rng.permutation(op.cout)
                n_dead, n_sat = int(round(dead * op.cout)), int(round(saturated * op.cout))
                i_dead, i_sat = order[:n_dead], order[n_dead:n_dead + n_sat]
                out = out.copy()
                out[i_sat] = 1.0
                W[gamma] *= out
                W[beta] *= out
                W[gamma][i_dead] = 0.0
                W[gamma][i_sat] *= SATURATED_GAMMA
                W[beta][i_sat] = float(SATURATED_BETA)
            else:
                W[gamma] *= out
                W[beta] *= out
        if cdst:
            t = vec.setdefault(dst, np.ones(cdst))
            t[coff:coff + op.cout] = out
        else:
            vec[dst] = out
        if alias:
            vec[alias] = out
    return {k: v.astype(np.float32) for k, v in W.items()}


def marks(prog: "arch.Program", weights: Dict[str, np.ndarray], precision: int = 16) -> Dict[str, dict]:
    """stored tensor -> dict(dead bool[c], saturated bool[c], const [c]) read back from the weights, for the tensors `prog`'s engine
    stores (a fused op's intermediates are not among them).  const: what a dead channel holds, as the kernels compute it -- the folded
    bias (gamma = 0: beta itself) as fp32, ReLU6, stored as fp16 (`-p 16`) or fp32; a split-operand block's second output stores
    fp16(6 z) of z = clamp(fp32(beta / 6), 0, 1) (k_mbconv_hp.hip)."""
    out: Dict[str, dict] = {}
    for op, src, dst, res, coff, cdst, alias in unit_ops(prog):
        if not _degenerate(op, res):
            continue
        g = np.asarray(weights[op.scope + "/BatchNorm/gamma"])
        b = np.asarray(weights[op.scope + "/BatchNorm/beta"])
        _, bias = engine.fold_batch_norm(weights, op)
        b32 = bias.astype(np.float32)
        for name, scaled in ((dst, False), (alias, True)):
            if name is None or name not in prog.tensors:
                continue
            hp_block = scaled and any(o.dst2 == name and o.hp for o in prog.ops)
            if hp_block:
                const = np.float32(6.0) * np.clip((bias / 6.0).astype(np.float32), np.float32(0), np.float32(1))
            else:
                const = np.clip(b32, np.float32(0), np.float32(6))
            const = const.astype(np.float16 if precision == 16 else np.float32)
            c = prog.tensors[name].c
            m = out.setdefault(name, dict(dead=np.zeros(c, bool), saturated=np.zeros(c, bool), const=np.zeros(c, const.dtype)))
            sl = slice(coff, coff + op.cout) if cdst else slice(0, op.cout)
            m["dead"][sl] = g == 0
            m["saturated"][sl] = (b == SATURATED_BETA) & (g != 0)
            m["const"][sl] = const
    return out


def count_fp16_subnormal(a) -> int:
    """How many values of `a` are non-zero and below the smallest normal fp16 number in magnitude."""
    a = np.abs(np.asarray(a, np.float64))
    return int(((a > 0) & (a < FP16_MIN_NORMAL)).sum())
