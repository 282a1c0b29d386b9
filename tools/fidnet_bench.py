#!/usr/bin/env python
"""FIDNet ResNet34_point inference timing at B = 1, 64 x 2048 and 128 x 2048 (128 x 2048 is the shape of the reference's own self-benchmark,
FIDNet.py:44-66): the HIP path under conv precision fp32 and f16x3 against the same containers as a plain torch module on PyTorch-ROCm eager on
the same card; then the two A/Bs that decide the model's defaults (fidnet.FUSED_STEM / COMMUTED_HEAD) --
    stem   slu_point_mlp (one launch)                                   against four conv2d_fused launches
    head   three low-resolution convs + slu_bilinear_ac_sum + conv_1    against slu_bilinear_ac_cat + the three-source 1024-channel conv_1
-- each timed alone on the model's own maps and inside the whole model, and the two new kernels alone.

    python tools/fidnet_bench.py [--iters 30] [--heights 64 128] [--kernels-only]

One JSON line per measurement.  Every time is the median over --iters of HIP-event windows around one call (warmed up; the windows of the
single kernels hold --reps back-to-back launches; the windows of the forms of an A/B are taken in turn).  The 512-channel maps are 268 and
537 MB, at and above the 256 MB last-level cache.
GFLOP/s and GB/s come from the shapes: 2 x MACs of the four layers; bytes read + written once.  point_mlp's fraction of the fp32-MFMA peak is
taken against 157.3 TFLOP/s, bilinear_ac_sum's fraction of HBM bandwidth against 8 TB/s.  Kernel-only times from the profiler:
`rocprofv3 --kernel-trace --stats -- python tools/fidnet_bench.py --kernels-only` (profiles/r32)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticlidarunc_amd import fidnet, ops, salsanext as sn  # noqa: E402
from semanticlidarunc_amd.testing import randomize_bn_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=5, help="back-to-back launches per timed window of a single kernel")
ap.add_argument("--heights", type=int, nargs="+", default=[64, 128])
ap.add_argument("--classes", type=int, default=20)
ap.add_argument("--kernels-only", action="store_true", help="only the two new kernels (for a run under rocprofv3 --kernel-trace --stats)")
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/fidnet_bench.py measures on the GPU only"
dev = torch.device("cuda:0")
torch.manual_seed(0)
W = 2048
PEAK_FP32_MFMA_TFLOPS, PEAK_HBM_TBPS = 157.3, 8.0


class EagerFIDNet(nn.Module):
    """The reference's forward (ResNet.py:560-590, 160-170) over the package containers' own torch sub-modules: the PyTorch-ROCm eager baseline."""

    def __init__(self, m: fidnet.FIDNet):
        super().__init__()
        self.m = m

    @staticmethod
    def _stage(layer, x):
        for blk in layer:
            o = F.leaky_relu(blk.bn1(blk.conv1(x)))
            o = blk.bn2(blk.conv2(o))
            x = F.leaky_relu(o + (x if blk.downsample is None else blk.downsample(x)))
        return x

    def forward(self, x):
        b, h = self.m.model.backend, self.m.model.semantic_head
        for conv, bn in ((b.conv1, b.bn_0), (b.conv2, b.bn), (b.conv3, b.bn_1), (b.conv4, b.bn_2)):
            x = F.leaky_relu(bn(conv(x)))
        x_1 = self._stage(b.layer1, x)
        x_2 = self._stage(b.layer2, x_1)
        x_3 = self._stage(b.layer3, x_2)
        x_4 = self._stage(b.layer4, x_3)
        res = [F.interpolate(t, size=x.shape[2:], mode="bilinear", align_corners=True) for t in (x_2, x_3, x_4)]
        t = torch.cat([x, x_1] + res, 1)
        t = F.leaky_relu(h.bn1(h.conv_1(t)))
        t = F.leaky_relu(h.bn2(h.conv_2(t)))
        return h.semantic_output(t)


def median_ms(fn, iters, warmup=3, reps=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ts)


def alternating_ms(fns, iters, warmup=3):
    """Median ms of each callable of the dict `fns`, their timed windows taken in turn (A, B, .., A, B, ..) so that drift on a shared host
    falls on all of them alike."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in ts.items()}


def emit(**kw):
    print(json.dumps(kw), flush=True)


model = randomize_bn_(fidnet.FIDNet(a.classes, "ResNet34_point"), 3).eval().to(dev)
backend, head = model.model.backend, model.model.semantic_head
eager = EagerFIDNet(model)
WIDTHS = (64, 128, 256, 512)
with torch.no_grad():
    for H in a.heights:
        x = torch.randn(1, 5, H, W, device=dev)
        shape = [1, 5, H, W]
        hw = H * W
        stem_flop = 2.0 * hw * sum(ci * co for ci, co in zip((5,) + WIDTHS[:-1], WIDTHS))
        stem_bytes = 4.0 * hw * (5 + 512)
        lows = [torch.randn(1, 128, H // s, W // s, device=dev) for s in (2, 4, 8)]
        parts = [torch.randn(1, 512, H // s, W // s, device=dev) for s in (2, 4, 8)]
        sum_bytes = 4.0 * 512 * hw + sum(4.0 * p.numel() for p in parts)

        # ---- the two new kernels alone ----
        sn.set_conv_precision("fp32")
        ms = median_ms(lambda: backend._stem(x, True), a.iters, reps=a.reps)
        tf = stem_flop / ms / 1e9
        emit(kernel="slu_point_mlp 5 -> 64 -> 128 -> 256 -> 512", shape=shape, ms=round(ms, 4), GFLOP=round(stem_flop / 1e9, 2),
             TFLOP_per_s=round(tf, 1), fraction_of_fp32_mfma_peak=round(tf / PEAK_FP32_MFMA_TFLOPS, 3), algorithmic_MB=round(stem_bytes / 1e6, 1))
        ms = median_ms(lambda: ops.bilinear_ac_sum(parts, (H, W)), a.iters, reps=a.reps)
        emit(kernel="slu_bilinear_ac_sum 3 x 512 ch (1/2, 1/4, 1/8) -> 512 ch", shape=[1, 512, H, W], ms=round(ms, 4),
             algorithmic_MB=round(sum_bytes / 1e6, 1), GB_per_s=round(sum_bytes / ms / 1e6, 1),
             fraction_of_hbm_peak=round(sum_bytes / ms / 1e9 / PEAK_HBM_TBPS, 3), note="allocates its output per call")
        if a.kernels_only:
            continue

        # ---- the model against eager ----
        ms, worst = {}, 0.0
        for prec in ("fp32", "f16x3"):
            sn.set_conv_precision(prec)
            ms[prec] = round(median_ms(lambda: model(x), a.iters), 3)
            worst = max(worst, float((model(x) - eager(x)).abs().max()))
        sn.set_conv_precision("fp32")
        ms["torch_eager"] = round(median_ms(lambda: eager(x), a.iters), 3)
        emit(model="FIDNet/ResNet34_point", shape=shape, classes=a.classes, median_ms_per_scan=ms,
             defaults={"fused_stem": fidnet.FUSED_STEM, "commuted_head": fidnet.COMMUTED_HEAD},
             speedup_vs_eager={k: round(ms["torch_eager"] / v, 2) for k, v in ms.items() if k != "torch_eager"})
        emit(check="max |HIP logits - torch eager logits|, both precisions", shape=shape, value=worst,
             scale=float(eager(x).abs().max()))

        # ---- A/B: each form alone on the model's own maps, and the whole model with each form ----
        x0 = backend._stem(x, True)
        x_1 = torch.randn(1, 128, H, W, device=dev)
        for prec in ("fp32", "f16x3"):
            sn.set_conv_precision(prec)
            stem = alternating_ms({"fused": lambda: backend._stem(x, True), "composed": lambda: backend._stem(x, False)}, a.iters)
            hd = alternating_ms({"commuted": lambda: head._conv_1_from_pyramid(x0, x_1, lows, (H, W), True),
                                 "composed": lambda: head._conv_1_from_pyramid(x0, x_1, lows, (H, W), False)}, a.iters)
            forms = {f"stem_{'fused' if fs else 'composed'}+head_{'commuted' if ch else 'composed'}":
                     (lambda fs=fs, ch=ch: model.model._forward(x, fused_stem=fs, commuted_head=ch)) for fs in (True, False) for ch in (True, False)}
            whole = {k: round(v, 3) for k, v in alternating_ms(forms, a.iters).items()}
            emit(ab="stem: slu_point_mlp vs four conv2d_fused launches", precision=prec, shape=shape, median_ms={k: round(v, 3) for k, v in stem.items()},
                 fused_not_slower=stem["fused"] <= stem["composed"])
            emit(ab="head conv_1: commuted (3 low-res convs + bilinear_ac_sum + conv) vs bilinear_ac_cat + three-source conv", precision=prec, shape=shape,
                 median_ms={k: round(v, 3) for k, v in hd.items()}, fused_not_slower=hd["commuted"] <= hd["composed"])
            emit(ab="whole model per form", precision=prec, shape=shape, median_ms_per_scan=whole)
        sn.set_conv_precision("fp32")
        del x0, x_1, lows, parts
