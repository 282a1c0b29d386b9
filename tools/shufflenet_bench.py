#!/usr/bin/env python
"""ShuffleNetV2 on the HIP path: (1) one unit, the fused path (fused 1x1 conv on a channel-offset source + slu_shuffle_tail_fwd) against the
composition of the ops the library had before it (ops.conv2d_fused on a contiguous copy of the half, ops.dwconv3x3, ops.conv2d_fused, torch.cat,
view / transpose / contiguous), at the shapes of a shufflenet_v2_x1_0 encoder on a 64 x 2048 scan; (2) B = 1 latency of both FPN classes on the
four widths at 64 x 2048 and 128 x 2048 in fp32, with the fp32 resnet18 of the same run next to them.

Timing: HIP events around REPS back-to-back calls, the two variants alternating inside one loop, warm-up first, median of --iters windows.
One JSON line per measurement.   python tools/shufflenet_bench.py [--iters 30] [--skip-models]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticlidarunc_amd import ops  # noqa: E402
from semanticlidarunc_amd.ops import ConvSource  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--skip-models", action="store_true")
a = ap.parse_args()
assert a.iters >= 20
dev = torch.device("cuda:0")


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.reps


def timed_pair(f, g, warmup=3):
    """median microseconds per call of f and of g, measured in alternating windows"""
    for _ in range(warmup):
        window(f)
        window(g)
    tf, tg = [], []
    for _ in range(a.iters):
        tf.append(window(f))
        tg.append(window(g))
    return statistics.median(tf), statistics.median(tg)


class Unit:
    """Random folded weights of one InvertedResidual with branch width cb (stride 2: input width cin)."""

    def __init__(self, cin, cb, stride, seed):
        g = torch.Generator().manual_seed(seed)
        self.cb, self.cin, self.stride = cb, cin, stride
        c2 = cin if stride == 2 else cb

        def r(*s, scale=1.0):
            return (torch.randn(*s, generator=g) * scale).to(dev)
        self.w_first, self.b_first = r(cb, c2, 1, 1, scale=c2 ** -0.5), r(cb, scale=0.1)
        self.p_first = ops.pack_conv_weight(self.w_first)
        self.w9, self.b9 = r(cb, 9, scale=1 / 3), r(cb, scale=0.1)
        self.w_last, self.b_last = r(cb, cb, scale=cb ** -0.5), r(cb, scale=0.1)
        self.p_last_conv = ops.pack_conv_weight(self.w_last.view(cb, cb, 1, 1).contiguous())
        self.p_last_tail = ops.pack_shuffle_tail_weight(self.w_last)
        if stride == 2:
            self.w9_1, self.b9_1 = r(cin, 9, scale=1 / 3), r(cin, scale=0.1)
            self.w_1, self.b_1 = r(cb, cin, scale=cin ** -0.5), r(cb, scale=0.1)
            self.p_1_conv = ops.pack_conv_weight(self.w_1.view(cb, cin, 1, 1).contiguous())
            self.p_1_tail = ops.pack_shuffle_tail_weight(self.w_1)

    def fused(self, x):
        cb = self.cb
        if self.stride == 1:
            h = ops.conv2d_fused([ConvSource(x, None, False, 0, cb, cb)], self.p_first, cb, 1, 1, 0, bias=self.b_first, act="relu")
            return ops.shuffle_tail(h, self.w9, self.b9, self.p_last_tail, self.b_last, cb, 1, passthrough=x)
        out = torch.empty((x.shape[0], 2 * cb, (x.shape[2] + 1) // 2, (x.shape[3] + 1) // 2), dtype=torch.float32, device=x.device)
        ops.shuffle_tail(x, self.w9_1, self.b9_1, self.p_1_tail, self.b_1, cb, 2, out=out, parity=0)
        h = ops.conv2d_fused([ConvSource(x)], self.p_first, cb, 1, 1, 0, bias=self.b_first, act="relu")
        return ops.shuffle_tail(h, self.w9, self.b9, self.p_last_tail, self.b_last, cb, 2, out=out, parity=1)

    def composed(self, x):
        cb = self.cb
        if self.stride == 1:
            first = x[:, :cb]
            h = ops.conv2d_fused([ConvSource(x[:, cb:].contiguous())], self.p_first, cb, 1, 1, 0, bias=self.b_first, act="relu")
        else:
            d1 = ops.dwconv3x3(x, self.w9_1, self.b9_1, 2)
            first = ops.conv2d_fused([ConvSource(d1)], self.p_1_conv, cb, 1, 1, 0, bias=self.b_1, act="relu")
            h = ops.conv2d_fused([ConvSource(x)], self.p_first, cb, 1, 1, 0, bias=self.b_first, act="relu")
        d = ops.dwconv3x3(h, self.w9, self.b9, self.stride)
        y = ops.conv2d_fused([ConvSource(d)], self.p_last_conv, cb, 1, 1, 0, bias=self.b_last, act="relu")
        cat = torch.cat([first, y], 1)
        n, c, hh, ww = cat.shape
        return cat.view(n, 2, c // 2, hh, ww).transpose(1, 2).contiguous().view(n, c, hh, ww)


# (label, input channels, branch width, stride, input H, input W, judged): shufflenet_v2_x1_0 on a 64 x 2048 scan
UNITS = [("stage2 first unit", 24, 58, 2, 64, 2048, True), ("stage2 unit", 116, 58, 1, 32, 1024, True),
         ("stage3 first unit", 116, 116, 2, 32, 1024, True), ("stage3 unit", 232, 116, 1, 16, 512, True),
         ("stage4 first unit", 232, 232, 2, 16, 512, False), ("stage4 unit", 464, 232, 1, 8, 256, False)]

for label, cin, cb, stride, h, w, judged in UNITS:
    u = Unit(cin, cb, stride, seed=cb + stride)
    x = torch.randn(1, cin, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    yf, yc = u.fused(x), u.composed(x)
    diff = float((yf - yc).abs().max())
    assert diff <= 1e-4 * max(1.0, float(yc.abs().max())), (label, diff)
    tf, tc = timed_pair(lambda: u.fused(x), lambda: u.composed(x))
    ho, wo = yf.shape[2:]
    tail_bytes = 4.0 * ho * wo * (cb * stride * stride + (cb if stride == 1 else 0) + (2 * cb if stride == 1 else cb))
    print(json.dumps({"unit": label, "Cb": cb, "stride": stride, "in": [1, cin, h, w], "fused_us": round(tf, 1), "composed_us": round(tc, 1),
                      "fused_over_composed": round(tf / tc, 3), "judged": judged, "launches": [2 if stride == 1 else 3, "3 or 5 + ATen copies"],
                      "max_abs_diff": diff, "tail_min_bytes": tail_bytes}), flush=True)

if not a.skip_models:
    from semanticlidarunc_amd.fpn import SemanticNetworkWithFPN as Plain
    from semanticlidarunc_amd.fpn_opt import SemanticNetworkWithFPN as Opt
    from semanticlidarunc_amd.testing import randomize_bn_

    def latency(model, h, w, m):
        g = torch.Generator().manual_seed(3)
        x, meta = torch.randn(1, 2, h, w, generator=g).to(dev), torch.randn(1, m, h, w, generator=g).to(dev)
        with torch.no_grad():
            for _ in range(3):
                model(x, meta)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                model(x, meta)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    for backbone in ("resnet18", "shufflenet_v2_x0_5", "shufflenet_v2_x1_0", "shufflenet_v2_x1_5", "shufflenet_v2_x2_0"):
        for name, cls in (("models.semanticFCN", Plain), ("semanticFCN_opt", Opt)):
            torch.manual_seed(0)
            model = randomize_bn_(cls(backbone=backbone, input_channels=2, meta_channel_dim=6, num_classes=20), 3).eval().to(dev)
            ms = {f"{h}x{w}": round(latency(model, h, w, 6), 3) for h, w in ((64, 2048), (128, 2048))}
            print(json.dumps({"model": name, "backbone": backbone, "precision": "fp32", "B": 1, "latency_ms": ms}), flush=True)
            del model
