#!/usr/bin/env python
"""Single-pass FPN inference timing at the reference's own self-benchmark shape (src/models/semanticFCN.py:381-395:
1 x (2 + 6) x 128 x 2048, median of CUDA-event timings).  python tools/fpn_bench.py [--backbone resnet18] [--batch 1]
--model opt [--precision fp32|f16x3|f16]: one forward of `semanticFCN_opt` at the same shape, eager and replayed from a HIP graph.
--model opt --mc T: the MC-dropout evaluation step (utils.mc_dropout.mc_predict, T passes) of `semanticFCN_opt` at B x (2 + 6) x 64 x 2048,
three ways: stacked (every pass runs the whole network), shared (pyramid once, fpn_opt.forward_mc) and shared + fused (slu_head_mc_f32, or
slu_head_mc_h8 with --precision f16)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticlidarunc_amd import salsanext as sn  # noqa: E402
from semanticlidarunc_amd.fpn import SemanticNetworkWithFPN  # noqa: E402
from semanticlidarunc_amd.testing import randomize_bn_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--backbone", default="resnet18")
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--model", default="fpn", choices=["fpn", "opt"])
ap.add_argument("--mc", type=int, default=0, help="with --model opt: MC-dropout passes T")
ap.add_argument("--precision", default="fp32", choices=["fp32", "f16x3", "f16"], help="with --model opt: conv precision (f16: fp16 storage, the h8 path)")
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)


def _median_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


if a.model == "opt":
    from semanticlidarunc_amd import ops  # noqa: E402
    from semanticlidarunc_amd.fpn_opt import SemanticNetworkWithFPN as OptFPN  # noqa: E402
    from semanticlidarunc_amd.utils.mc_dropout import mc_forward, mc_predict  # noqa: E402
    model = randomize_bn_(OptFPN(a.backbone, 2, 6, num_classes=20), 3).eval().to(dev)
    if a.mc < 1:                                   # one forward at the reference's self-benchmark shape
        x, meta = torch.randn(a.batch, 2, 128, 2048, device=dev), torch.randn(a.batch, 6, 128, 2048, device=dev)
        sn.set_conv_precision(a.precision)
        with torch.no_grad():
            ms = _median_ms(lambda: model(x, meta), a.iters, warmup=10)
            s_ = torch.cuda.Stream()
            s_.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s_):
                for _ in range(3):
                    model(x, meta)
            torch.cuda.current_stream().wait_stream(s_)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                y_static = model(x, meta)
            eager = model(x, meta)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(eager, y_static), "graph replay differs from the eager forward"
            gms = _median_ms(graph.replay, a.iters)
        print(json.dumps({"model": f"semanticFCN_opt/{a.backbone}", "shape": [a.batch, 8, 128, 2048], "precision": a.precision,
                          "median_ms": round(ms, 3), "scans_per_s": round(a.batch * 1e3 / ms, 1), "hipgraph_median_ms": round(gms, 3)}))
        sys.exit(0)
    x, meta = torch.randn(a.batch, 2, 64, 2048, device=dev), torch.randn(a.batch, 6, 64, 2048, device=dev)
    sn.set_conv_precision(a.precision)
    ways = {"stacked": lambda: mc_predict(model, [x, meta], T=a.mc, share_prefix=False),
            "shared": lambda: ops.mc_reduce(mc_forward(model, [x, meta], T=a.mc, share_prefix=True).contiguous()),
            "shared_fused": lambda: mc_predict(model, [x, meta], T=a.mc, share_prefix=True)}
    ms = {k: round(_median_ms(f, a.iters), 3) for k, f in ways.items()}
    print(json.dumps({"model": f"semanticFCN_opt/{a.backbone}", "shape": [a.batch, 8, 64, 2048], "T": a.mc, "precision": a.precision, "median_ms": ms,
                      "speedup_shared": round(ms["stacked"] / ms["shared"], 3), "speedup_shared_fused": round(ms["stacked"] / ms["shared_fused"], 3)}))
    sys.exit(0)

model = randomize_bn_(SemanticNetworkWithFPN(a.backbone, 2, 6, num_classes=20), 3).eval().to(dev)
x, meta = torch.randn(a.batch, 2, 128, 2048, device=dev), torch.randn(a.batch, 6, 128, 2048, device=dev)
out = {}
for prec in ("fp32", "f16x3", "f16"):      # "f16": fp16 storage (the h8 path)
    sn.set_conv_precision(prec)
    with torch.no_grad():
        for _ in range(10):
            model(x, meta)
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model(x, meta)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    out[prec] = {"median_ms": round(statistics.median(ts), 3), "scans_per_s": round(a.batch * 1e3 / statistics.median(ts), 1)}
    # the same forward replayed from a HIP graph (hipGraph via torch.cuda.CUDAGraph): removes the per-launch host cost
    with torch.no_grad():
        static_x, static_m = x.clone(), meta.clone()
        s_ = torch.cuda.Stream()
        s_.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s_):
            for _ in range(3):
                model(static_x, static_m)
        torch.cuda.current_stream().wait_stream(s_)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y_static = model(static_x, static_m)
        eager = model(static_x, static_m)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(eager, y_static), "graph replay differs from the eager forward"
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    out[prec]["hipgraph_median_ms"] = round(statistics.median(ts), 3)
print(json.dumps({"model": f"FPN/{a.backbone}", "shape": [a.batch, 8, 128, 2048], "reference_published_ms": 9.8 if a.backbone == "resnet18" else 13.6, **out}))
