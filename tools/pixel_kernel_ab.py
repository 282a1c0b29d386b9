#!/usr/bin/env python
"""Per-launch time of single fp32 per-pixel kernels that no bench launches (development aid for changes to csrc/pixel_common.h):

    python tools/pixel_kernel_ab.py [--rounds 12] [--reps 50]                                   the library in the tree
    python tools/run_with_lib.py ab_libs/libslu_parent.so tools/pixel_kernel_ab.py ...          another build

Shapes: pyramid level 1 of the resnet18 FPN at the 1 x 8 x 128 x 2048 input of tools/fpn_bench.py (256 x 32 x 512 into the attention) and a
full-resolution layer of the SalsaNext training step of tools/train_bench.py (4 x 32 x 64 x 2048).  A round is `reps` launches back to back
between two events; one JSON line per kernel with mean / stdev / min over the rounds in microseconds per launch -- that includes the host
side of the launch, so for kernel time run it under `rocprofv3 --kernel-trace --stats` and read the stats table.  Alternate the two
libraries run by run and compare by the two-sigma rule against the spread of the parent's own runs (profiles/r21)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semanticlidarunc_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
r = lambda *s: torch.randn(*s, generator=g).to(dev)

score, value, dout = r(1, 1, 32, 512), r(1, 256, 32, 512), r(1, 256, 32, 512)
act, resid = r(4, 32, 64, 2048), r(4, 32, 64, 2048)
ca, cb = torch.rand(32, generator=g).to(dev) + 0.5, r(32)
CASES = {
    "row_softmax_mul_kernel": lambda: ops.row_softmax_mul(score, value),
    "row_softmax_mul_bwd_kernel": lambda: ops.row_softmax_mul_bwd(score, value, dout),
    "affine_kernel<4>": lambda: ops.affine(act, ca, cb, resid),
}
for name, fn in CASES.items():
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(a.rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        us.append(t0.elapsed_time(t1) * 1000.0 / a.reps)
    print(json.dumps({"kernel": name, "mean_us": round(statistics.mean(us), 2), "stdev_us": round(statistics.stdev(us), 2), "min_us": round(min(us), 2),
                      "rounds": a.rounds, "reps": a.reps}), flush=True)
