#!/usr/bin/env python
"""Development aid: the fused 128-channel block tail (conv_tail_h8) against the same two layers as two conv2d_h8 launches, at the three levels
of the strict step (N = 64): mean, standard deviation and minimum of 20 timed launches each.  SLU_TAIL_V1=1 times the round-1 kernel."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticlidarunc_amd import h8  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
dev = torch.device("cuda:0")
c = 128


def timed(fn, it=20):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(it):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    t = torch.tensor(ts)
    return float(t.mean()), float(t.std()), float(t.min())


for hh, ww, res in ((32, 1024, True), (16, 512, False), (8, 256, False)):
    g = torch.Generator(device=dev).manual_seed(c)
    a1 = torch.randn(n, c // 8, hh, ww, 8, device=dev, generator=g).half()
    a2 = torch.randn(n, c // 8, hh, ww, 8, device=dev, generator=g).half()
    r = torch.randn(n, c // 8, hh, ww, 8, device=dev, generator=g).half() if res else None
    w2 = h8.pack_conv_weight_h8(torch.randn(c, c, 2, 2, device=dev, generator=g) / (4 * c) ** 0.5)
    w1 = h8.pack_conv_weight_h8(torch.randn(c, 3 * c, 1, 1, device=dev, generator=g) / (3 * c) ** 0.5)
    z = torch.zeros(c, device=dev)
    name = h8.conv_tail_kernel_name(c, n, hh, ww, res)
    fused = lambda: h8.conv_tail_h8(a1, a2, w2, w1, z, 0.01, (z + 1, z), z, 0.01, (z + 1, z), resid=r)

    def pair():
        h3 = h8.conv2d_h8([h8.H8Source(a2)], w2, c, c, 2, 2, 1, bias=z, slope=0.01, bn_a=z + 1, bn_b=z)
        return h8.conv2d_h8([h8.H8Source(a1), h8.H8Source(a2), h8.H8Source(h3)], w1, 3 * c, c, 1, 1, 0, bias=z, slope=0.01, resid=r, bn_a=z + 1, bn_b=z)
    fm, fs, fmin = timed(fused)
    pm, ps, pmin = timed(pair)
    d = float((fused().float() - pair().float()).abs().max())
    print(f"C=128 N={n} {hh}x{ww} resid={res}: fused [{name}] {fm:7.1f} +- {fs:4.1f} us (min {fmin:7.1f})   two launches {pm:7.1f} +- {ps:4.1f} us (min {pmin:7.1f})   max|diff| {d:.3e}", flush=True)
