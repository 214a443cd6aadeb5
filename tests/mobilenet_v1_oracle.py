"""Oracle (test infrastructure): SSD-MobileNet-v1 300x300 forward pass in fp32 on the CPU, torch, BatchNorm unfolded.

The counterpart of `oracle/ssd_mobilenet_v2.py` and `tests/inception_v2_oracle.py` for the third network family
(watsor_amd/mobilenet_v1.py).  The layer table is restated here on its own rather than imported from the builder, so that it checks
the engine's program rather than repeating it.  It follows the TF-slim / Object Detection API definition as recalled (see
watsor_amd/mobilenet_v1.py); parity against real TensorFlow is unpinned.

`MobilenetV1OracleNet.forward(x_nhwc, keep)` has the signature of `oracle.ssd_mobilenet_v2.OracleNet.forward`;
`MobilenetV1OracleDetector` is `oracle.detect.OracleObjectDetector` on this network (pre- and post-processing are the oracle's own).
`emulate16=True` is the `-p 16` engine emulated on the CPU: BatchNorm folded in float64, weights rounded to fp16, every stored tensor
rounded to fp16 (the depthwise outputs included), fp32 sums, the fp16 input.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from inception_v2_oracle import _pad
from oracle import postprocess as post
from oracle.detect import OracleObjectDetector

BN_EPS = 1e-3
NUM_CLASSES_WITH_BG = 91
FE = "FeatureExtractor/MobilenetV1/"

# Conv2d_1 .. Conv2d_13: (depthwise stride, pointwise output channels); Conv2d_0 is a 3x3 stride-2 conv 3 -> 32
_LAYERS = [(1, 64), (2, 128), (1, 128), (2, 256), (1, 256), (2, 512), (1, 512), (1, 512), (1, 512), (1, 512), (1, 512),
           (2, 1024), (1, 1024)]
_EXTRAS = [(256, 512), (128, 256), (128, 256), (64, 128)]


def feature_map_names() -> List[str]:
    return ["Conv2d_11_pointwise", "Conv2d_13_pointwise"] + [
        "Conv2d_13_pointwise_2_Conv2d_%d_3x3_s2_%d" % (i + 2, d2) for i, (_, d2) in enumerate(_EXTRAS)]


def conv_list() -> List[Tuple[str, int, int, int, int, bool]]:
    """(scope, cin, cout, k, stride, depthwise) of every BatchNorm-ReLU6 conv, in graph order."""
    out = [("Conv2d_0", 3, 32, 3, 2, False)]
    cin = 32
    for i, (s, c) in enumerate(_LAYERS, start=1):
        out += [("Conv2d_%d_depthwise" % i, cin, cin, 3, s, True), ("Conv2d_%d_pointwise" % i, cin, c, 1, 1, False)]
        cin = c
    for i, (d1, d2) in enumerate(_EXTRAS):
        out += [("Conv2d_13_pointwise_1_Conv2d_%d_1x1_%d" % (i + 2, d1), cin, d1, 1, 1, False),
                ("Conv2d_13_pointwise_2_Conv2d_%d_3x3_s2_%d" % (i + 2, d2), d1, d2, 3, 2, False)]
        cin = d2
    return out


class MobilenetV1OracleNet:
    """fp32 forward pass (unfolded BatchNorm) on the weights dict W; emulate16: the `-p 16` engine emulated instead (BatchNorm folded
    in float64, fp16 weights and fp16 stored tensors, fp32 sums)."""

    def __init__(self, W: Dict[str, np.ndarray], emulate16: bool = False):
        import torch

        torch.set_grad_enabled(False)
        self.W = W
        self.emulate16 = emulate16
        self.head_k = [W["BoxPredictor_%d/BoxEncodingPredictor/weights" % i].shape[0] for i in range(6)]
        self.convs = {}
        for scope, cin, cout, k, s, dw in conv_list():
            w = W[FE + scope + ("/depthwise_weights" if dw else "/weights")]
            assert w.shape == ((k, k, cin, 1) if dw else (k, k, cin, cout)), scope
            self.convs[scope] = (self._bn_conv(FE + scope, w, dw), k, s, cin if dw else 1)

    def _bn_conv(self, scope, w, dw):
        import torch
        g, b, m, v = (self.W[scope + "/BatchNorm/" + n].astype(np.float64) for n in ("gamma", "beta", "moving_mean", "moving_variance"))
        # torch layout: [cout, cin / groups, k, k]; a depthwise [k,k,C,1] filter is [C, 1, k, k]
        perm = (2, 3, 0, 1) if dw else (3, 2, 0, 1)
        if self.emulate16:
            s = g / np.sqrt(v + BN_EPS)
            wf = (w.astype(np.float64) * (s[None, None, :, None] if dw else s)).astype(np.float16).astype(np.float32)
            return (torch.from_numpy(np.ascontiguousarray(wf.transpose(*perm))), None, None,
                    torch.from_numpy((b - m * s).astype(np.float32))[None, :, None, None])
        wt = torch.from_numpy(np.ascontiguousarray(w.astype(np.float32).transpose(*perm)))
        gf, bf, mf, vf = (torch.from_numpy(a.astype(np.float32)) for a in (g, b, m, v))
        # FusedBatchNorm (inference): (x - mean) * (gamma * rsqrt(var + eps)) + beta
        return wt, mf[None, :, None, None], (gf * torch.rsqrt(vf + BN_EPS))[None, :, None, None], bf[None, :, None, None]

    def _conv(self, x, scope):
        import torch
        import torch.nn.functional as F
        (w, mean, scale, beta), k, s, groups = self.convs[scope]
        y = F.conv2d(_pad(x, k, s), w, None, stride=s, groups=groups)
        y = y + beta if mean is None else (y - mean) * scale + beta
        y = torch.clamp(y, 0.0, 6.0)
        return y.half().float() if self.emulate16 else y

    def forward(self, x_nhwc: np.ndarray, keep: bool = False):
        """x_nhwc float32 [B,300,300,3], resized + normalised -> (box_enc [B,1917,4], logits [B,1917,91], tensors or None);
        `tensors` maps the engine's tensor names (watsor_amd/mobilenet_v1.py) to NHWC float32 arrays -- the depthwise outputs
        included, which only the one-op-per-layer program holds."""
        import torch
        import torch.nn.functional as F

        x = torch.from_numpy(np.ascontiguousarray(x_nhwc.transpose(0, 3, 1, 2)).astype(np.float32))
        if self.emulate16:
            x = x.half().float()
        T = {}
        cur = T["Conv2d_0"] = self._conv(x, "Conv2d_0")
        for i in range(1, len(_LAYERS) + 1):
            T["Conv2d_%d_depthwise" % i] = self._conv(cur, "Conv2d_%d_depthwise" % i)
            cur = T["Conv2d_%d_pointwise" % i] = self._conv(T["Conv2d_%d_depthwise" % i], "Conv2d_%d_pointwise" % i)
        for i, (d1, d2) in enumerate(_EXTRAS):
            n1, n2 = "Conv2d_13_pointwise_1_Conv2d_%d_1x1_%d" % (i + 2, d1), "Conv2d_13_pointwise_2_Conv2d_%d_3x3_s2_%d" % (i + 2, d2)
            T[n1] = self._conv(cur, n1)
            cur = T[n2] = self._conv(T[n1], n2)
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
    return MobilenetV1OracleNet(W).forward(x_nhwc, keep)


class MobilenetV1OracleDetector(OracleObjectDetector):
    """`OracleObjectDetector` (raw(), detect(): the reference CPU plugin's detect restated) on the MobileNet-v1 network."""

    def __init__(self, weights: Dict[str, np.ndarray], size: int = 300, half_pixel_centers: bool = False,
                 clip_after_nms: bool = False, post_config=None):
        self._fast_post = False
        self._half_pixel, self._clip_after, self._post = half_pixel_centers, clip_after_nms, dict(post_config or {})
        self._net = MobilenetV1OracleNet(weights)
        self._size = size
        self._anchors = post.anchors_center_size(post.generate_anchors(size))
