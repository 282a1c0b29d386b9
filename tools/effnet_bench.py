#!/usr/bin/env python
"""EfficientNetV2 on the HIP path of models.semanticFCN: (1) the middle of one MBConv block -- depthwise 3x3 + BatchNorm + SiLU + the SE's mean +
the gate -- on the fused route (slu_dwconv3x3_se_fwd + slu_se_gate_psum, 2 launches) against the composed route fpn_opt.py still takes
(slu_dwconv3x3_fwd + slu_global_avgpool + slu_se_gate, 3 launches), at every depthwise conv of features[4] of efficientnet_v2_s / _m / _l -- widths
256 / 320 / 384 at stride 2 (the stage's first block) and 512 / 640 / 768 at stride 1 -- on a 64 x 2048 and a 128 x 2048 scan; (2) B = 1 latency of
models.semanticFCN on the three encoders at both scans in fp32, with the fp32 resnet18 of the same run next to them.

Timing: HIP events around REPS back-to-back calls, the two routes alternating inside one loop, warm-up first; median and quartiles of --iters
windows.  One JSON line per measurement.   python tools/effnet_bench.py [--iters 30] [--skip-models] [--skip-blocks]

Two launches of a few microseconds each are issued by the host more slowly than the device runs them, so the per-call times above are mostly the
host's; the kernels' own times come from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/effnet_bench.py --trace-calls 20
    python tools/effnet_bench.py --summarize-trace DIR/.../*_kernel_trace.csv --trace-calls 20
The first runs, per shape, 20 calls of the fused route and then 20 of the composed one (no events, no checks); the second needs no GPU: it cuts
the dispatches of the five kernels into runs of 20 in that order and prints the median kernel time per shape and route."""
import argparse
import json
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semanticlidarunc_amd import _lib, effnet as eff, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--skip-models", action="store_true")
ap.add_argument("--skip-blocks", action="store_true")
ap.add_argument("--trace-calls", type=int, default=0)
ap.add_argument("--summarize-trace", default=None)
a = ap.parse_args()
assert a.iters >= 20
# the gate is one template (csrc/se_gate.hip): the routes differ in its launch bound; no closing bracket, the names are matched between \b
KERNELS = {"fused": ("dwconv3x3_se_kernel", "se_gate_kernel<true, 1024"), "composed": ("dwconv3x3_kernel", "global_avgpool_kernel", "se_gate_kernel<true, 256")}


def block_shapes(name):
    """(stride, expanded width, squeeze width) of the distinct depthwise convs of features[4]."""
    kind, expand, k, stride, cin, cout, n = eff._CONFIGS[name][0][3]
    assert kind == "mb" and stride == 2
    return [(2, eff._make_divisible(cin * expand), max(1, cin // 4)), (1, eff._make_divisible(cout * expand), max(1, cout // 4))]


def all_shapes():
    """(backbone, scan, stride, C, S, H, W of the depthwise conv's input): features[4] takes the 1/4 map to 1/8."""
    for scan_h, scan_w in ((64, 2048), (128, 2048)):
        for name in eff._CONFIGS:
            for stride, c, s in block_shapes(name):
                h, w = (scan_h // 4, scan_w // 4) if stride == 2 else (scan_h // 8, scan_w // 8)
                yield name, [scan_h, scan_w], stride, c, s, h, w


if a.summarize_trace:
    import csv
    k = a.trace_calls
    assert k > 0, "--trace-calls must repeat the value of the traced run"
    runs = {n: [] for names in KERNELS.values() for n in names}
    for row in csv.DictReader(open(a.summarize_trace)):
        for n in runs:
            if re.search(r"\b" + n + r"\b", row["Kernel_Name"]):
                runs[n].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    shapes = list(all_shapes())
    for n, v in runs.items():
        v.sort()
        assert len(v) == k * len(shapes), (n, len(v))
    for i, (name, scan, stride, c, s, h, w) in enumerate(shapes):
        med = {n: round(statistics.median(t for _, t in v[i * k:(i + 1) * k]), 2) for n, v in runs.items()}
        tot = {route: round(sum(med[n] for n in names), 2) for route, names in KERNELS.items()}
        mbytes = 4.0 * c * (h * w + (h // stride) * (w // stride)) / 1e6
        print(json.dumps({"backbone": name, "scan": scan, "stride": stride, "C": c, "S": s, "in": [1, c, h, w], "kernel_us_median": med,
                          "fused_kernels_us": tot["fused"], "composed_kernels_us": tot["composed"],
                          "fused_over_composed": round(tot["fused"] / tot["composed"], 3), "min_traffic_mb": round(mbytes, 2),
                          "dw_se_gb_per_s": round(mbytes / med["dwconv3x3_se_kernel"] * 1e3, 0)}))
    sys.exit(0)

dev = torch.device("cuda:0")


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.reps


def quartiles(t):
    q = statistics.quantiles(t, n=4)
    return [round(q[0], 1), round(q[1], 1), round(q[2], 1)]


def timed(fns, warmup=3):
    """[p25, median, p75] microseconds per call of each function, measured in alternating windows"""
    for _ in range(warmup):
        for f in fns:
            window(f)
    ts = [[] for _ in fns]
    for _ in range(a.iters):
        for t, f in zip(ts, fns):
            t.append(window(f))
    return [quartiles(t) for t in ts]


class Middle:
    """The depthwise conv (BatchNorm folded) + the SE of one MBConv of expanded width c, He-drawn weights and N(0, 0.5) SE biases."""

    def __init__(self, c, stride, s, seed):
        g = torch.Generator().manual_seed(seed)

        def r(*shape, scale):
            return (torch.randn(*shape, generator=g) * scale).to(dev)
        self.stride = stride
        self.w9, self.bias = r(c, 9, scale=(2 / 9) ** 0.5), r(c, scale=0.1)
        self.w1, self.b1, self.w2, self.b2 = r(s, c, scale=(2 / c) ** 0.5), r(s, scale=0.5), r(c, s, scale=(2 / s) ** 0.5), r(c, scale=0.5)

    def fused(self, x):
        y, psum = ops.dwconv3x3_se(x, self.w9, self.bias, self.stride)
        return y, ops.se_gate_psum(psum, y.shape[2] * y.shape[3], self.w1, self.b1, self.w2, self.b2)

    def composed(self, x):
        y = ops.dwconv3x3(x, self.w9, self.bias, self.stride, "silu")
        return y, ops.se_scale(y, self.w1, self.b1, self.w2, self.b2)


if a.trace_calls:
    for name, scan, stride, c, s, h, w in all_shapes():
        u = Middle(c, stride, s, seed=c + stride)
        x = torch.randn(1, c, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
        for route in (u.fused, u.composed):
            for _ in range(a.trace_calls):
                route(x)
            torch.cuda.synchronize()
    sys.exit(0)

if not a.skip_blocks:
    for name, (scan_h, scan_w), stride, c, s, h, w in all_shapes():
        u = Middle(c, stride, s, seed=c + stride)
        x = torch.randn(1, c, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
        (yf, gf), (yc, gc) = u.fused(x), u.composed(x)
        same = bool(torch.equal(yf, yc))
        gdiff = float((gf - gc).abs().max())
        assert same and gdiff <= 1e-5, (name, stride, same, gdiff)
        tf, tc = timed([lambda: u.fused(x), lambda: u.composed(x)])
        oh, ow = h // stride, w // stride
        mbytes = 4.0 * c * (h * w + oh * ow) / 1e6      # the input read once, the output written once
        print(json.dumps({"backbone": name, "scan": [scan_h, scan_w], "stride": stride, "C": c, "S": s, "in": [1, c, h, w],
                          "tiles": _lib.load().slu_dwconv3x3_se_tiles(h, w, stride),
                          "fused_us": tf, "composed_us": tc, "fused_over_composed": round(tf[1] / tc[1], 3), "launches": [2, 3],
                          "y_bit_identical": same, "gate_abs_diff": gdiff, "min_traffic_mb": round(mbytes, 2),
                          "fused_gb_per_s_at_least": round(mbytes / tf[1] * 1e3, 0)}), flush=True)
        del u

if not a.skip_models:
    from semanticlidarunc_amd.fpn import SemanticNetworkWithFPN as Plain
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
        q = statistics.quantiles(ts, n=4)
        return [round(v, 3) for v in q]

    for backbone in ("resnet18",) + tuple(eff._CONFIGS):
        torch.manual_seed(0)
        model = randomize_bn_(Plain(backbone=backbone, input_channels=2, meta_channel_dim=6, num_classes=20), 3).eval().to(dev)
        ms = {f"{h}x{w}": latency(model, h, w, 6) for h, w in ((64, 2048), (128, 2048))}
        print(json.dumps({"model": "models.semanticFCN", "backbone": backbone, "precision": "fp32", "B": 1, "latency_ms_p25_median_p75": ms}), flush=True)
        del model
