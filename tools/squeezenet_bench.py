#!/usr/bin/env python
"""SqueezeNet 1.0 on the HIP path: (1) one Fire module, the fused launch (slu_fire_fwd) against the composition of the ops the library had before
it (three ops.conv2d_fused with bias + ReLU, plus torch.cat), at the shapes of the eight Fires of a 64 x 2048 scan; the composed time under
'f16x3' is reported next to it; (2) B = 1 latency of both FPN classes on squeezenet1_0 at 64 x 2048 and 128 x 2048 in fp32, with the fp32
resnet18 of the same run next to them; (3) --errors: the model cases of tests/squeezenet_restatement.py under 'fp32' and 'f16x3' against the fp64
restatement (error in S, share of flipped pixels).

Timing: HIP events around REPS back-to-back calls, the two variants alternating inside one loop, warm-up first, median of --iters windows.
One JSON line per measurement.   python tools/squeezenet_bench.py [--iters 30] [--skip-models] [--errors]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semanticlidarunc_amd import ops, salsanext as sn  # noqa: E402
from semanticlidarunc_amd.ops import ConvSource  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--skip-models", action="store_true")
ap.add_argument("--skip-fires", action="store_true")
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


def timed(fns, warmup=3):
    """median microseconds per call of each function, measured in alternating windows"""
    for _ in range(warmup):
        for f in fns:
            window(f)
    ts = [[] for _ in fns]
    for _ in range(a.iters):
        for t, f in zip(ts, fns):
            t.append(window(f))
    return [statistics.median(t) for t in ts]


class FireUnit:
    """He-drawn weights and N(0, 0.1) biases of one Fire(cin, s, e, e)."""

    def __init__(self, cin, s, e, seed):
        g = torch.Generator().manual_seed(seed)

        def r(*shape, scale):
            return (torch.randn(*shape, generator=g) * scale).to(dev)
        self.s, self.e = s, e
        self.wsq, self.w1, self.w3 = r(s, cin, 1, 1, scale=(2 / cin) ** 0.5), r(e, s, 1, 1, scale=(2 / s) ** 0.5), r(e, s, 3, 3, scale=(2 / (9 * s)) ** 0.5)
        self.bsq, self.b1, self.b3 = r(s, scale=0.1), r(e, scale=0.1), r(e, scale=0.1)
        self.wpack = ops.pack_fire_weight(self.wsq.view(s, cin), self.w1.view(e, s), self.w3)
        self.packs = {"fp32": [ops.pack_conv_weight(w) for w in (self.wsq, self.w1, self.w3)],
                      "f16x3": [ops.pack_conv_weight_f16x3(w) for w in (self.wsq, self.w1, self.w3)]}

    def fused(self, x):
        return ops.fire(x, self.wpack, self.bsq, self.b1, self.b3)

    def composed(self, x, prec="fp32"):
        p = self.packs[prec]
        sq = ops.conv2d_fused([ConvSource(x)], p[0], self.s, 1, 1, 0, bias=self.bsq, precision=prec, act="relu")
        e1 = ops.conv2d_fused([ConvSource(sq)], p[1], self.e, 1, 1, 0, bias=self.b1, precision=prec, act="relu")
        e3 = ops.conv2d_fused([ConvSource(sq)], p[2], self.e, 3, 1, 1, bias=self.b3, precision=prec, act="relu")
        return torch.cat([e1, e3], 1)


# (features index, input channels, squeeze, expand (each), H, W, judged): squeezenet1_0 on a 64 x 2048 scan
FIRES = [(3, 96, 16, 64, 32, 1024, True), (4, 128, 16, 64, 32, 1024, True), (5, 128, 32, 128, 32, 1024, True), (7, 256, 32, 128, 16, 512, True),
         (8, 256, 48, 192, 16, 512, True), (9, 384, 48, 192, 16, 512, True), (10, 384, 64, 256, 16, 512, True), (12, 512, 64, 256, 8, 256, False)]

if not a.skip_fires:
    for idx, cin, s, e, h, w, judged in FIRES:
        u = FireUnit(cin, s, e, seed=idx)
        x = torch.randn(1, cin, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
        yf, yc = u.fused(x), u.composed(x)
        diff = float((yf - yc).abs().max())
        assert diff <= 1e-4 * max(1.0, float(yc.abs().max())), (idx, diff)
        tf, tc, tc3 = timed([lambda: u.fused(x), lambda: u.composed(x), lambda: u.composed(x, "f16x3")])
        flops = 2.0 * h * w * (cin * s + s * e + 9 * s * e)
        nbytes = 4.0 * h * w * (cin + 2 * e)
        print(json.dumps({"fire": f"features.{idx}", "Cin": cin, "S": s, "E1": e, "E3": e, "in": [1, cin, h, w], "fused_us": round(tf, 1),
                          "composed_us": round(tc, 1), "fused_over_composed": round(tf / tc, 3), "composed_f16x3_us": round(tc3, 1), "judged": judged,
                          "launches": [1, "3 + torch.cat"], "max_abs_diff": diff, "gflop": round(flops / 1e9, 3), "min_mbytes": round(nbytes / 1e6, 2),
                          "fused_tflops": round(flops / tf / 1e6, 1)}), flush=True)

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

    for backbone in ("resnet18", "squeezenet1_0"):
        for name, cls in (("models.semanticFCN", Plain), ("semanticFCN_opt", Opt)):
            torch.manual_seed(0)
            model = randomize_bn_(cls(backbone=backbone, input_channels=2, meta_channel_dim=6, num_classes=20), 3).eval().to(dev)
            ms = {f"{h}x{w}": round(latency(model, h, w, 6), 3) for h, w in ((64, 2048), (128, 2048))}
            print(json.dumps({"model": name, "backbone": backbone, "precision": "fp32", "B": 1, "latency_ms": ms}), flush=True)
            del model

if a.errors:
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import numpy as np
    import squeezenet_restatement as R

    for case in R.model_cases():
        cid, kind, config, b, h, w, classes, seed, gname = case
        model = R.build(R.package_class(kind), config, classes)
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
