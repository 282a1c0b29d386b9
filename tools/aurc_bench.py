#!/usr/bin/env python
"""Device time of the AURC aggregator: ``add_batch`` for one 64x2048x20 scan and ``finalize(make_plots=False)`` at 131 072,
2 000 000 and 50 000 000 samples.  HIP events around each call (the scalars' copy to the host included), one warm-up, the median
of ``--runs`` (>= 20) runs.  Prints a markdown table and, with ``--reference PATH_TO_SRC``, the host time of the
reference's ``aurc_from_risks_confids`` at 131 072 samples on this CPU as the comparison point.

    python tools/aurc_bench.py [--runs 20] [--sizes 131072 2000000 50000000] [--reference /path/to/reference/src]
"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from semanticlidarunc_amd.metrics.aurc import UncertaintyAggregator      # noqa: E402


def timed(fn, runs):
    fn()                                                   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[131_072, 2_000_000, 50_000_000])
    ap.add_argument("--reference", default=None, help="the reference's src/ directory: also time its aurc_from_risks_confids on the CPU")
    args = ap.parse_args()
    runs = max(args.runs, 20)
    if torch.cuda.is_available():
        device_rows(args, runs)
    elif not args.reference:
        raise SystemExit("no GPU visible: only --reference (the host comparison point) can run here")
    if args.reference:
        reference_row(args.reference)


def device_rows(args, runs):
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    rows = []

    probs = (torch.randn(1, 20, 64, 2048, generator=gen) * 2).softmax(1).to(dev)
    labels = torch.randint(0, 20, (1, 1, 64, 2048), generator=gen)
    labels[torch.rand(1, 1, 64, 2048, generator=gen) < 0.1] = 255
    labels = labels.to(dev)
    for name, maxprob in (("entropy confidence", False), ("max-prob confidence", True)):
        def add(maxprob=maxprob):
            UncertaintyAggregator(use_max_prob_confidence=maxprob).add_batch(probs, labels)
        med, best = timed(add, runs)
        rows.append((f"`add_batch`, one 1x20x64x2048 scan, {name}", med, best))

    for n in args.sizes:
        conf = torch.rand(n, generator=gen).to(dev)
        err = (torch.rand(n, generator=gen) < 0.1).to(torch.uint8).to(dev)
        agg = UncertaintyAggregator()
        agg._buf.push(conf, err)
        agg._added = True
        med, best = timed(lambda: agg.finalize(make_plots=False), runs)
        rows.append(("`finalize(make_plots=False)`, " + f"{n:,}".replace(",", " ") + " samples", med, best))
        del agg, conf, err
        torch.cuda.empty_cache()

    print(f"| step ({torch.cuda.get_device_name(0)}, median of {runs}) | median ms | best ms |")
    print("|---|---|---|")
    for name, med, best in rows:
        print(f"| {name} | {med:.3f} | {best:.3f} |")


def reference_row(src):
    spec = importlib.util.spec_from_file_location("_ref_aurc", os.path.join(src, "metrics", "aurc.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.RandomState(0)
    confids, risks = rng.rand(131_072).astype(np.float32), (rng.rand(131_072) < 0.1).astype(np.float32)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref.aurc_from_risks_confids(risks, confids)
        t.append((time.perf_counter() - t0) * 1e3)
    print(f"| reference `aurc_from_risks_confids`, 131 072 samples, this CPU (median of 3) | {statistics.median(t):.1f} | {min(t):.1f} |")


if __name__ == "__main__":
    main()
