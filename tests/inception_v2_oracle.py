"""Oracle (test infrastructure): SSD-Inception-v2 300x300 forward pass in fp32 on the CPU, torch, BatchNorm unfolded.

The counterpart of `oracle/ssd_mobilenet_v2.py` for the second network family (watsor_amd/inception.py).  The graph is restated
here on its own -- module table, branch order, pool kinds, the separable stem as depthwise THEN pointwise -- so that it checks the
engine's program rather than repeating it.  Like the MobileNet oracle it follows the TF-slim / Object Detection API definition as
recalled (see watsor_amd/inception.py); parity against real TensorFlow is unpinned.

`InceptionOracleNet.forward(x_nhwc, keep)` has the signature of `oracle.ssd_mobilenet_v2.OracleNet.forward`;
`InceptionOracleDetector` is `oracle.detect.OracleObjectDetector` on this network (pre- and post-processing are the oracle's own).
`emulate16=True` is the `-p 16` engine emulated on the CPU: BatchNorm folded in float64, weights rounded to fp16, every stored tensor
rounded to fp16, fp32 accumulation, the fp16 input.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from oracle import postprocess as post
from oracle.detect import OracleObjectDetector

BN_EPS = 1e-3
NUM_CLASSES_WITH_BG = 91
FE = "FeatureExtractor/InceptionV2/"

# name: (B0, B1, B2, B3 1x1 depth or None, B3 pool kind); reduction modules (B3 None) have B0 = 1x1 -> 3x3 s2, B1 = 1x1 -> 3x3 -> 3x3 s2
# and a 3x3 s2 max pool as their last branch
_MIXED = [
    ("Mixed_3b", [64], [64, 64], [64, 96, 96], 32, "avg"),
    ("Mixed_3c", [64], [64, 96], [64, 96, 96], 64, "avg"),
    ("Mixed_4a", [128, 160], [64, 96, 96], None, None, "max"),
    ("Mixed_4b", [224], [64, 96], [96, 128, 128], 128, "avg"),
    ("Mixed_4c", [192], [96, 128], [96, 128, 128], 128, "avg"),
    ("Mixed_4d", [160], [128, 160], [128, 160, 160], 96, "avg"),
    ("Mixed_4e", [96], [128, 192], [160, 192, 192], 96, "avg"),
    ("Mixed_5a", [128, 192], [192, 256, 256], None, None, "max"),
    ("Mixed_5b", [352], [192, 320], [160, 224, 224], 128, "avg"),
    ("Mixed_5c", [352], [192, 320], [192, 224, 224], 128, "max"),
]
_EXTRAS = [(256, 512), (128, 256), (128, 256), (64, 128)]


def same_pad(n_in: int, k: int, stride: int) -> Tuple[int, int, int]:
    n_out = -(-n_in // stride)
    total = max((n_out - 1) * stride + k - n_in, 0)
    return n_out, total // 2, total - total // 2


def _pad(x, k, s, value=0.0):
    import torch.nn.functional as F
    _, pt, pb = same_pad(x.shape[2], k, s)
    _, pl, pr = same_pad(x.shape[3], k, s)
    return F.pad(x, (pl, pr, pt, pb), value=value) if (pt or pb or pl or pr) else x


def max_pool_same(x, s):
    """TF MaxPool 3x3 'SAME' on NCHW: the padding never wins (it is -inf)."""
    import torch.nn.functional as F
    return F.max_pool2d(_pad(x, 3, s, float("-inf")), 3, s)


def avg_pool_same(x, s):
    """TF AvgPool 3x3 'SAME' on NCHW: the sum of the in-image taps divided by their number (4 at a corner, 6 on an edge, 9 inside)."""
    import torch
    import torch.nn.functional as F
    total = F.avg_pool2d(_pad(x, 3, s), 3, s, divisor_override=1)
    ones = torch.ones((1, 1, x.shape[2], x.shape[3]), dtype=x.dtype)
    return total / F.avg_pool2d(_pad(ones, 3, s), 3, s, divisor_override=1)


def conv_list() -> List[Tuple[str, int, int, int, int]]:
    """(scope, cin, cout, k, stride) of every BatchNorm-ReLU6 conv but the stem, in graph order."""
    out = [("Conv2d_2b_1x1", 64, 64, 1, 1), ("Conv2d_2c_3x3", 64, 192, 3, 1)]
    cin = 192
    for name, b0, b1, b2, b3, _ in _MIXED:
        if b3 is None:
            out += [(name + "/Branch_0/Conv2d_0a_1x1", cin, b0[0], 1, 1), (name + "/Branch_0/Conv2d_1a_3x3", b0[0], b0[1], 3, 2),
                    (name + "/Branch_1/Conv2d_0a_1x1", cin, b1[0], 1, 1), (name + "/Branch_1/Conv2d_0b_3x3", b1[0], b1[1], 3, 1),
                    (name + "/Branch_1/Conv2d_1a_3x3", b1[1], b1[2], 3, 2)]
            cin = b0[1] + b1[2] + cin
        else:
            out += [(name + "/Branch_0/Conv2d_0a_1x1", cin, b0[0], 1, 1),
                    (name + "/Branch_1/Conv2d_0a_1x1", cin, b1[0], 1, 1), (name + "/Branch_1/Conv2d_0b_3x3", b1[0], b1[1], 3, 1),
                    (name + "/Branch_2/Conv2d_0a_1x1", cin, b2[0], 1, 1), (name + "/Branch_2/Conv2d_0b_3x3", b2[0], b2[1], 3, 1),
                    (name + "/Branch_2/Conv2d_0c_3x3", b2[1], b2[2], 3, 1), (name + "/Branch_3/Conv2d_0b_1x1", cin, b3, 1, 1)]
            cin = b0[0] + b1[1] + b2[2] + b3
    for i, (d1, d2) in enumerate(_EXTRAS):
        out += [("Mixed_5c_1_Conv2d_%d_1x1_%d" % (i + 2, d1), cin, d1, 1, 1), ("Mixed_5c_2_Conv2d_%d_3x3_s2_%d" % (i + 2, d2), d1, d2, 3, 2)]
        cin = d2
    return out


def feature_map_names() -> List[str]:
    return ["Mixed_4c", "Mixed_5c"] + ["Mixed_5c_2_Conv2d_%d_3x3_s2_%d" % (i + 2, d2) for i, (_, d2) in enumerate(_EXTRAS)]


class InceptionOracleNet:
    """fp32 forward pass (unfolded BatchNorm, separable stem) on the weights dict W; emulate16: the `-p 16` engine emulated instead
    (the stem folded into one dense 7x7 kernel, BatchNorm folded in float64, fp16 weights and fp16 stored tensors, fp32 sums)."""

    def __init__(self, W: Dict[str, np.ndarray], emulate16: bool = False):
        import torch

        torch.set_grad_enabled(False)
        self.W = W
        self.emulate16 = emulate16
        self.head_k = [W["BoxPredictor_%d/BoxEncodingPredictor/weights" % i].shape[0] for i in range(6)]
        self.convs = {scope: self._bn_conv(FE + scope, W[FE + scope + "/weights"]) for scope, *_ in conv_list()}
        stem = FE + "Conv2d_1a_7x7"
        dw = W[stem + "/depthwise_weights"].astype(np.float64)            # [7,7,3,8]
        pw = W[stem + "/pointwise_weights"].astype(np.float64)            # [1,1,24,64]
        if emulate16:
            self.stem = self._bn_conv(stem, np.einsum("yxcm,cmo->yxco", dw, pw[0, 0].reshape(dw.shape[2], dw.shape[3], -1)))
        else:
            # depthwise output channel c * 8 + m, as TF's DepthwiseConv2dNative orders it
            self.stem_dw = torch.from_numpy(np.ascontiguousarray(dw.transpose(2, 3, 0, 1).reshape(-1, 1, 7, 7)).astype(np.float32))
            self.stem = self._bn_conv(stem, pw)

    def _bn_conv(self, scope, w):
        import torch
        g, b, m, v = (self.W[scope + "/BatchNorm/" + n].astype(np.float64) for n in ("gamma", "beta", "moving_mean", "moving_variance"))
        if self.emulate16:
            s = g / np.sqrt(v + BN_EPS)
            wf = (w.astype(np.float64) * s).astype(np.float16).astype(np.float32)
            return (torch.from_numpy(np.ascontiguousarray(wf.transpose(3, 2, 0, 1))), None, None,
                    torch.from_numpy((b - m * s).astype(np.float32))[None, :, None, None])
        wt = torch.from_numpy(np.ascontiguousarray(w.astype(np.float32).transpose(3, 2, 0, 1)))
        gf, bf, mf, vf = (torch.from_numpy(a.astype(np.float32)) for a in (g, b, m, v))
        # FusedBatchNorm (inference): (x - mean) * (gamma * rsqrt(var + eps)) + beta
        return wt, mf[None, :, None, None], (gf * torch.rsqrt(vf + BN_EPS))[None, :, None, None], bf[None, :, None, None]

    def _store(self, y):
        return y.half().float() if self.emulate16 else y

    def _conv(self, x, p, k, s):
        import torch
        import torch.nn.functional as F
        w, mean, scale, beta = p
        y = F.conv2d(_pad(x, k, s), w, None, stride=s)
        y = y + beta if mean is None else (y - mean) * scale + beta
        return self._store(torch.clamp(y, 0.0, 6.0))

    def forward(self, x_nhwc: np.ndarray, keep: bool = False):
        """x_nhwc float32 [B,300,300,3], resized + normalised -> (box_enc [B,1917,4], logits [B,1917,91], tensors or None);
        `tensors` maps the engine's tensor names (watsor_amd/inception.py) to NHWC float32 arrays."""
        import torch
        import torch.nn.functional as F

        x = torch.from_numpy(np.ascontiguousarray(x_nhwc.transpose(0, 3, 1, 2)).astype(np.float32))
        T = {}
        if self.emulate16:
            T["Conv2d_1a_7x7"] = self._conv(x.half().float(), self.stem, 7, 2)
        else:
            d = F.conv2d(_pad(x, 7, 2), self.stem_dw, None, stride=2, groups=3)
            T["Conv2d_1a_7x7"] = self._conv(d, self.stem, 1, 1)
        T["MaxPool_2a_3x3"] = max_pool_same(T["Conv2d_1a_7x7"], 2)
        T["Conv2d_2b_1x1"] = self._conv(T["MaxPool_2a_3x3"], self.convs["Conv2d_2b_1x1"], 1, 1)
        T["Conv2d_2c_3x3"] = self._conv(T["Conv2d_2b_1x1"], self.convs["Conv2d_2c_3x3"], 3, 1)
        cur = T["MaxPool_3a_3x3"] = max_pool_same(T["Conv2d_2c_3x3"], 2)
        c = self.convs
        for name, b0, b1, b2, b3, pool in _MIXED:
            if b3 is None:
                y0 = self._conv(self._conv(cur, c[name + "/Branch_0/Conv2d_0a_1x1"], 1, 1), c[name + "/Branch_0/Conv2d_1a_3x3"], 3, 2)
                y1 = self._conv(cur, c[name + "/Branch_1/Conv2d_0a_1x1"], 1, 1)
                y1 = self._conv(y1, c[name + "/Branch_1/Conv2d_0b_3x3"], 3, 1)
                y1 = self._conv(y1, c[name + "/Branch_1/Conv2d_1a_3x3"], 3, 2)
                parts = [y0, y1, max_pool_same(cur, 2)]
            else:
                y0 = self._conv(cur, c[name + "/Branch_0/Conv2d_0a_1x1"], 1, 1)
                y1 = self._conv(self._conv(cur, c[name + "/Branch_1/Conv2d_0a_1x1"], 1, 1), c[name + "/Branch_1/Conv2d_0b_3x3"], 3, 1)
                y2 = self._conv(cur, c[name + "/Branch_2/Conv2d_0a_1x1"], 1, 1)
                y2 = self._conv(y2, c[name + "/Branch_2/Conv2d_0b_3x3"], 3, 1)
                y2 = self._conv(y2, c[name + "/Branch_2/Conv2d_0c_3x3"], 3, 1)
                p = self._store(max_pool_same(cur, 1) if pool == "max" else avg_pool_same(cur, 1))
                parts = [y0, y1, y2, self._conv(p, c[name + "/Branch_3/Conv2d_0b_1x1"], 1, 1)]
            cur = T[name] = torch.cat(parts, 1)
        for i, (d1, d2) in enumerate(_EXTRAS):
            n1, n2 = "Mixed_5c_1_Conv2d_%d_1x1_%d" % (i + 2, d1), "Mixed_5c_2_Conv2d_%d_3x3_s2_%d" % (i + 2, d2)
            T[n1] = self._conv(cur, c[n1], 1, 1)
            cur = T[n2] = self._conv(T[n1], c[n2], 3, 2)
        boxes, logits = [], []
        for i, tname in enumerate(feature_map_names()):
            k = self.head_k[i]
            for sub, out, cols in (("BoxEncodingPredictor", boxes, 4), ("ClassPredictor", logits, NUM_CLASSES_WITH_BG)):
                w = self.W["BoxPredictor_%d/%s/weights" % (i, sub)]
                if self.emulate16:
                    w = w.astype(np.float16)
                wt = torch.from_numpy(np.ascontiguousarray(w.astype(np.float32).transpose(3, 2, 0, 1)))
                b = torch.from_numpy(self.W["BoxPredictor_%d/%s/biases" % (i, sub)].astype(np.float32))
                y = F.conv2d(_pad(T[tname], k, 1), wt, b, stride=1)
                out.append(y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, cols))
        box_enc = torch.cat(boxes, 1).numpy()
        cls = torch.cat(logits, 1).numpy()
        tensors = {k: v.permute(0, 2, 3, 1).contiguous().numpy() for k, v in T.items()} if keep else None
        return box_enc, cls, tensors


def forward(W: Dict[str, np.ndarray], x_nhwc: np.ndarray, keep: bool = False):
    return InceptionOracleNet(W).forward(x_nhwc, keep)


class InceptionOracleDetector(OracleObjectDetector):
    """`OracleObjectDetector` (raw(), detect(): the reference CPU plugin's detect restated) on the Inception network."""

    def __init__(self, weights: Dict[str, np.ndarray], size: int = 300, half_pixel_centers: bool = False,
                 clip_after_nms: bool = False, post_config=None):
        self._fast_post = False
        self._half_pixel, self._clip_after, self._post = half_pixel_centers, clip_after_nms, dict(post_config or {})
        self._net = InceptionOracleNet(weights)
        self._size = size
        self._anchors = post.anchors_center_size(post.generate_anchors(size))
