#!/usr/bin/env python
"""RegNetY on the HIP path: (1) the middle of one Y block -- f.b + BatchNorm + ReLU + the SE's mean + the gate -- on the new route
(slu_regnet_gconv_fwd + slu_regnet_se_gate, 2 launches) against the route composed from what the library had before (the grouped conv as a
dense 3x3 through ops.conv2d_fused with block-diagonal weights -- at stride 2 over ops.space_to_depth2, as the ResNet stages do --, then
ops.global_avgpool, then the gate), at every (width, stride, map) f.b takes in regnet_y_1_6gf and regnet_y_3_2gf on a 64 x 2048 scan; the composed
time under 'f16x3' is reported next to it; (2) B = 1 latency of both FPN classes on both backbones at 64 x 2048 and 128 x 2048 in fp32, with the
fp32 resnet18 of the same run next to them; (3) --errors: the model cases of tests/regnet_restatement.py under 'fp32' and 'f16x3' against the
fp64 restatement (error in S, share of flipped pixels).

Timing: HIP events around REPS back-to-back calls, the variants alternating inside one loop, warm-up first; median and quartiles of --iters
windows.  One JSON line per measurement.   python tools/regnet_bench.py [--iters 30] [--skip-models] [--skip-blocks] [--errors]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semanticlidarunc_amd import ops, regnet as rgn, salsanext as sn  # noqa: E402
from semanticlidarunc_amd.ops import ConvSource  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--skip-models", action="store_true")
ap.add_argument("--skip-blocks", action="store_true")
ap.add_argument("--errors", action="store_true")
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
    """f.b (BatchNorm folded) + the SE of one Y block of width c, He-drawn weights and N(0, 0.5) SE biases."""

    def __init__(self, c, gw, stride, s, seed):
        g = torch.Generator().manual_seed(seed)

        def r(*shape, scale):
            return (torch.randn(*shape, generator=g) * scale).to(dev)
        self.c, self.gw, self.stride = c, gw, stride
        w = r(c, gw, 3, 3, scale=(2 / (9 * gw)) ** 0.5)
        self.bias = r(c, scale=0.1)
        self.w1, self.b1, self.w2, self.b2 = r(s, c, scale=(2 / c) ** 0.5), r(s, scale=0.5), r(c, s, scale=(2 / s) ** 0.5), r(c, scale=0.5)
        self.wg = ops.pack_regnet_gconv_weight(w, gw)
        dense = torch.zeros(c, c, 3, 3, device=dev)
        for i in range(c // gw):
            dense[i * gw:(i + 1) * gw, i * gw:(i + 1) * gw] = w[i * gw:(i + 1) * gw]
        if stride == 2:      # the 3x3 / stride 2 / pad 1 conv as the 2x2 / pad 1 conv over the space-to-depth image (fpn.py `_p_conv_s2`)
            w2 = torch.zeros((c, 4, c, 2, 2), device=dev)
            tap = {0: (1, 0), 1: (0, 1), 2: (1, 1)}
            for i, (p, aa) in tap.items():
                for j, (q, bb) in tap.items():
                    w2[:, 2 * p + q, :, aa, bb] = dense[:, :, i, j]
            dense, self.k = w2.reshape(c, 4 * c, 2, 2), 2
        else:
            self.k = 3
        self.packs = {"fp32": ops.pack_conv_weight(dense.contiguous()), "f16x3": ops.pack_conv_weight_f16x3(dense.contiguous())}
        del dense

    def new(self, x):
        y, psum = ops.regnet_gconv(x, self.wg, self.bias, self.stride)
        return y, ops.regnet_se_gate(psum, y.shape[2] * y.shape[3], self.w1, self.b1, self.w2, self.b2)

    def composed(self, x, prec="fp32"):
        src = ops.space_to_depth2(x) if self.stride == 2 else x
        y = ops.conv2d_fused([ConvSource(src)], self.packs[prec], self.c, self.k, 1, 1, bias=self.bias, precision=prec, act="relu")
        return y, ops.regnet_se_gate(ops.global_avgpool(y), 1, self.w1, self.b1, self.w2, self.b2)


def block_shapes(name):
    """(stage, width, stride, squeeze width, input H, input W of f.b) of every distinct f.b of the model on a 64 x 2048 scan."""
    widths, depths = rgn.stage_widths_and_depths(name)
    out, cur, h, w = [], rgn.STEM_WIDTH, 64, 2048
    for i, (wd, d) in enumerate(zip(widths, depths)):
        out.append((i + 1, wd, 2, int(round(rgn.SE_RATIO * cur)), h, w))
        h, w = h // 2, w // 2
        if d > 1:
            out.append((i + 1, wd, 1, int(round(rgn.SE_RATIO * wd)), h, w))
        cur = wd
    return out


if not a.skip_blocks:
    for name in rgn.ENABLED:
        gw = rgn.GROUP_WIDTH[name]
        for stage, c, stride, s, h, w in block_shapes(name):
            u = Middle(c, gw, stride, s, seed=stage * 10 + stride)
            x = torch.randn(1, c, h, w, generator=torch.Generator().manual_seed(1)).abs().to(dev)
            (yn, gn), (yc, gc) = u.new(x), u.composed(x)
            diff, gdiff = float((yn - yc).abs().max()), float((gn - gc).abs().max())
            assert diff <= 1e-4 * max(1.0, float(yc.abs().max())) and gdiff <= 1e-4, (name, stage, stride, diff, gdiff)
            tn, tc, tc3 = timed([lambda: u.new(x), lambda: u.composed(x), lambda: u.composed(x, "f16x3")])
            oh, ow = h // stride, w // stride
            flops = 2.0 * oh * ow * c * gw * 9
            print(json.dumps({"backbone": name, "block": f"stage {stage}, stride {stride}", "C": c, "gw": gw, "S": s, "in": [1, c, h, w], "new_us": tn,
                              "composed_us": tc, "new_over_composed": round(tn[1] / tc[1], 3), "composed_f16x3_us": tc3, "judged": True,
                              "launches": [2, 3 if stride == 1 else 4], "max_abs_diff": diff, "gate_abs_diff": gdiff, "gflop": round(flops / 1e9, 3),
                              "new_conv_tflops_at_most": round(flops / tn[1] / 1e6, 1)}), flush=True)
            del u

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
        q = statistics.quantiles(ts, n=4)
        return [round(v, 3) for v in q]

    for backbone in ("resnet18",) + tuple(rgn.ENABLED):
        for name, cls in (("models.semanticFCN", Plain), ("semanticFCN_opt", Opt)):
            torch.manual_seed(0)
            model = randomize_bn_(cls(backbone=backbone, input_channels=2, meta_channel_dim=6, num_classes=20), 3).eval().to(dev)
            ms = {f"{h}x{w}": latency(model, h, w, 6) for h, w in ((64, 2048), (128, 2048))}
            print(json.dumps({"model": name, "backbone": backbone, "precision": "fp32", "B": 1, "latency_ms_p25_median_p75": ms}), flush=True)
            del model

if a.errors:
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import numpy as np
    import regnet_restatement as R

    for case in R.model_cases():
        cid, kind, backbone, config, b, h, w, classes, seed, gname = case
        model = R.build(R.package_class(kind), backbone, config, classes)
        if gname is None:
            x, meta = R.inputs(config, b, h, w, seed)
        else:
            g = np.load(os.path.join(ROOT, "tests", "golden", gname + ".npz"))
            x, meta = torch.from_numpy(g["x"]), torch.from_numpy(g["meta"])
        want = R.forward(kind, model.state_dict(), x, meta, config, dtype=torch.float64)
        s = R.scale_of(want)
        m = model.to(dev)
        row = {"case": cid, "S": round(s, 3)}
        for prec in ("fp32", "f16x3"):
            sn.set_conv_precision(prec)
            try:
                with torch.no_grad():
                    y = m(x.to(dev), meta.to(dev)).cpu()
            finally:
                sn.set_conv_precision("fp32")
            row[prec] = {"err_in_S": float((y.double() - want).abs().max()) / s, "flip_share": R.flips(y, want)}
        print(json.dumps(row), flush=True)
