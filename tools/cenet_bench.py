#!/usr/bin/env python
"""CENet ResNet-34 inference timing at B = 1, 64 x 2048 and 128 x 2048 (the shape of the reference's own self-benchmarks, CENet.py:28-50 and
CENet_ResNet34.py:200-221): the HIP path under conv precision fp32 and f16x3, with and without the aux heads, against the same architecture as a
plain torch module on PyTorch-ROCm eager on the same card; then the two decoder kernels against slu_bilinear_upsample writing the same bytes.

    python tools/cenet_bench.py [--iters 30] [--heights 64 128] [--kernels-only]

One JSON line per measurement.  Model lines: median per-scan ms of HIP-event timings around one forward (warmed up).  Kernel lines: HIP events
around `--reps` back-to-back launches, median over --iters, divided by the launches; GB/s = (bytes read + bytes written, from the shapes) / time.
Maps below the 256 MB of the last-level cache (the 20-class softmax outputs are 10 to 21 MB) are timed cache-warm; the lines say so.  A kernel
of ~10 us is enqueued no faster than it runs: for those the event window measures the host's launch rate, and the kernel time comes from
`rocprofv3 --kernel-trace --stats -- python tools/cenet_bench.py --kernels-only` (profiles/r31)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticlidarunc_amd import ops, salsanext as sn  # noqa: E402
from semanticlidarunc_amd.cenet import ResNet_34  # noqa: E402
from semanticlidarunc_amd.testing import randomize_bn_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=20, help="back-to-back launches per timed window of a single kernel")
ap.add_argument("--heights", type=int, nargs="+", default=[64, 128])
ap.add_argument("--classes", type=int, default=20)
ap.add_argument("--kernels-only", action="store_true", help="skip the model timings (for a run under rocprofv3 --kernel-trace --stats)")
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/cenet_bench.py measures on the GPU only"
dev = torch.device("cuda:0")
torch.manual_seed(0)
W = 2048


class EagerResNet34(nn.Module):
    """The reference's forward (CENet_ResNet34.py:154-198) over the package container's own torch sub-modules: the PyTorch-ROCm eager baseline."""

    def __init__(self, m: ResNet_34):
        super().__init__()
        self.m = m

    @staticmethod
    def _cbr(b, x):
        return F.leaky_relu(b.bn(b.conv(x)))

    @staticmethod
    def _stage(layer, x):
        for blk in layer:
            o = F.leaky_relu(blk.bn1(blk.conv1(x)))
            o = blk.bn2(blk.conv2(o))
            x = F.leaky_relu(o + (x if blk.downsample is None else blk.downsample(x)))
        return x

    def forward(self, x):
        m = self.m
        x = self._cbr(m.conv3, self._cbr(m.conv2, self._cbr(m.conv1, x)))
        x_1 = self._stage(m.layer1, x)
        x_2 = self._stage(m.layer2, x_1)
        x_3 = self._stage(m.layer3, x_2)
        x_4 = self._stage(m.layer4, x_3)
        res = [F.interpolate(t, size=x.shape[2:], mode="bilinear", align_corners=True) for t in (x_2, x_3, x_4)]
        out = self._cbr(m.conv_2, self._cbr(m.conv_1, torch.cat([x, x_1] + res, 1)))
        out = F.softmax(m.semantic_output(out), 1)
        if not m.aux:
            return out
        return [out] + [F.softmax(h(r), 1) for h, r in zip((m.aux_head1, m.aux_head2, m.aux_head3), res)]


def median_ms(fn, iters, warmup=5, reps=1):
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


def emit(**kw):
    print(json.dumps(kw), flush=True)


model = randomize_bn_(ResNet_34(a.classes, input_dim=5, aux=True), 3).eval().to(dev)
eager = EagerResNet34(model)
with torch.no_grad():
    for H in a.heights:
        x = torch.randn(1, 5, H, W, device=dev)
        worst = 0.0
        for aux in () if a.kernels_only else (True, False):
            model.aux = aux
            ms = {}
            for prec in ("fp32", "f16x3"):
                sn.set_conv_precision(prec)
                ms[prec] = round(median_ms(lambda: model(x), a.iters), 3)
                if aux:
                    worst = max(worst, max(float((g - w).abs().max()) for g, w in zip(model(x), eager(x))))
            sn.set_conv_precision("fp32")
            ms["torch_eager"] = round(median_ms(lambda: eager(x), a.iters), 3)
            emit(model="CENet/ResNet_34", shape=[1, 5, H, W], classes=a.classes, aux=aux, median_ms_per_scan=ms,
                 speedup_vs_eager={k: round(ms["torch_eager"] / v, 2) for k, v in ms.items() if k != "torch_eager"})
        model.aux = True
        if not a.kernels_only:
            emit(check="max |HIP - torch eager| over the four probability maps, both precisions", shape=[1, 5, H, W], value=worst)

        # ---- the two decoder kernels against slu_bilinear_upsample at the same output bytes ----
        def rate(name, fn, nbytes, note=""):
            ms_ = median_ms(fn, a.iters, reps=a.reps)
            emit(kernel=name, H=H, W=W, us=round(1e3 * ms_, 2), algorithmic_MB=round(nbytes / 1e6, 1), GB_per_s=round(nbytes / ms_ / 1e6, 1), note=note)
            return nbytes / ms_ / 1e6

        srcs = [torch.randn(1, 128, H // s, W // s, device=dev) for s in (2, 4, 8)]
        out_b = 4 * 384 * H * W
        buf = torch.empty(1, 384, H, W, device=dev)
        r_cat = rate("slu_bilinear_ac_cat 3 x 128 ch (1/2, 1/4, 1/8) -> 384 ch", lambda: ops.bilinear_ac_cat(srcs, (H, W), out=buf),
                     out_b + sum(4 * s.numel() for s in srcs))
        half = torch.randn(1, 384, H // 2, W // 2, device=dev)
        r_up = rate("slu_bilinear_upsample 384 ch x2 (same output bytes)", lambda: ops.bilinear_upsample(half, 2), out_b + 4 * half.numel(),
                    "allocates its output per call")
        emit(ratio="slu_bilinear_ac_cat / slu_bilinear_upsample", H=H, value=round(r_cat / r_up, 2))
        lo = torch.randn(1, a.classes, H // 4, W // 4, device=dev)
        full = torch.randn(1, a.classes, H, W, device=dev)
        sm_b = 4 * a.classes * H * W
        warm = "cache-warm: the maps fit the last-level cache"
        r_sm = rate(f"slu_bilinear_ac_softmax {a.classes} classes 1/4 -> full", lambda: ops.bilinear_ac_softmax(lo, (H, W)), sm_b + 4 * lo.numel(), warm)
        r_id = rate(f"slu_bilinear_ac_softmax {a.classes} classes, equal sizes", lambda: ops.bilinear_ac_softmax(full), 2 * sm_b, warm)
        r_u4 = rate(f"slu_bilinear_upsample {a.classes} ch x4 (same output bytes)", lambda: ops.bilinear_upsample(lo, 4), sm_b + 4 * lo.numel(), warm)
        emit(ratio="slu_bilinear_ac_softmax (1/4 -> full) / slu_bilinear_upsample", H=H, value=round(r_sm / r_u4, 2))
        emit(ratio="slu_bilinear_ac_softmax (equal sizes) / slu_bilinear_upsample", H=H, value=round(r_id / r_u4, 2))
        del srcs, buf, half, lo, full
