#!/usr/bin/env python
"""slu_head_mc_f32 alone against the launches it replaces (GroupNorm statistics + apply, the 1x1 head conv, slu_mc_reduce) on a random
decoder output [T*B, Cin, H, W]: median of HIP-event timings, GB/s on the fused kernel's minimum bytes, FLOP/s.
python tools/head_mc_f32_bench.py [--cin 16] [--classes 20] [--passes 8] [--batch 1] [--h 64] [--w 2048]"""
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
ap.add_argument("--cin", type=int, default=16)
ap.add_argument("--classes", type=int, default=20)
ap.add_argument("--passes", type=int, default=8)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--h", type=int, default=64)
ap.add_argument("--w", type=int, default=2048)
ap.add_argument("--groups", type=int, default=8)
ap.add_argument("--iters", type=int, default=50)
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
n = a.passes * a.batch
x = torch.randn(n, a.cin, a.h, a.w, device=dev) * 3 + 1
wt = torch.randn(a.classes, a.cin, 1, 1, device=dev) / a.cin ** 0.5
bias, gamma, beta = torch.randn(a.classes, device=dev), torch.rand(a.cin, device=dev) + 0.5, torch.randn(a.cin, device=dev) * 0.1
wp = ops.pack_conv_weight(wt)


def timed(fn, iters=a.iters, warmup=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


stats = ops.groupnorm_stats(x, a.groups)
y = ops.groupnorm(x, a.groups, gamma, beta, relu=True)
logits = ops.conv2d_fused([ConvSource(y)], wp, a.classes, 1, 1, 0, bias=bias, act="none")
us = {"groupnorm_stats": timed(lambda: ops.groupnorm_stats(x, a.groups)),
      "head_mc_f32": timed(lambda: ops.head_mc_f32(x, wt, bias, a.passes, a.batch, gn_stats=stats, gn_groups=a.groups, gn_gamma=gamma, gn_beta=beta, relu=True)),
      "groupnorm_stats_and_apply": timed(lambda: ops.groupnorm(x, a.groups, gamma, beta, relu=True)),
      "head_conv": timed(lambda: ops.conv2d_fused([ConvSource(y)], wp, a.classes, 1, 1, 0, bias=bias, act="none")),
      "mc_reduce": timed(lambda: ops.mc_reduce(logits.view(a.passes, a.batch, a.classes, a.h, a.w)))}
px = n * a.h * a.w
min_bytes = 4.0 * px * a.cin + a.batch * a.h * a.w * (4.0 * a.classes + 16.0)
t = us["head_mc_f32"] * 1e-6
print(json.dumps({"shape": [n, a.cin, a.h, a.w], "classes": a.classes, "T": a.passes, "us": {k: round(v, 1) for k, v in us.items()},
                  "fused_us": round(us["groupnorm_stats"] + us["head_mc_f32"], 1),
                  "replaced_us": round(us["groupnorm_stats_and_apply"] + us["head_conv"] + us["mc_reduce"], 1),
                  "head_mc_f32_GBps_min_bytes": round(min_bytes / t / 1e9, 1), "fraction_of_8TBps": round(min_bytes / t / 8e12, 3),
                  "head_mc_f32_TFLOPs": round(2.0 * a.cin * a.classes * px / t / 1e12, 2),
                  "head_mc_f32_TFLOPs_padded_M32": round(2.0 * a.cin * 32 * px / t / 1e12, 2)}))
