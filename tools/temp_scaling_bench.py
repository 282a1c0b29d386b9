#!/usr/bin/env python
"""Wall-clock time of the temperature-scaling closure and of a full LBFGS fit at N = 4 x 64 x 2048 rows, C = 20 (DESIGN
"Temperature scaling on the device"), for three ways to evaluate the objective:

  fused        the resident cache and one ``ops.temp_nll`` pass per evaluation (models/temp_scaling.py of this package)
  torch/host   the reference's loop restated with torch ops: the cache in pinned host memory, uploaded in 1 M-row chunks on every
               evaluation, ``x / T`` -> ``cross_entropy(reduction="sum")`` -> ``backward`` per chunk
  torch/device the same loop with the cache already on the device (no upload)

A closure evaluation is timed with a host clock around ``--runs`` evaluations that end in a device synchronise, after a warm-up;
the fit is the stock ``torch.optim.LBFGS`` with the reference's settings, timed the same way (median of ``--fits``).  Prints a
markdown table with the ratios.

    python tools/temp_scaling_bench.py [--rows 524288] [--classes 20] [--runs 50] [--fits 5]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from semanticlidarunc_amd.loss import temp_nll_loss      # noqa: E402

CHUNK = 1_000_000


def make_rows(n, c, gen):
    """log(clamp(p, 1e-12)) rows of an over-confident classifier, a quarter of them wrong."""
    y = torch.randint(0, c, (n,), generator=gen)
    z = torch.randn(n, c, generator=gen)
    hit = torch.where(torch.rand(n, generator=gen) < 0.25, torch.randint(0, c, (n,), generator=gen), y)
    z.scatter_add_(1, hit[:, None], torch.full((n, 1), 2.0))
    return (z * 6.0).softmax(1).clamp_min(1e-12).log().contiguous(), y


def fused_closure(rows, labels, log_t, opt=None):
    n = labels.numel()

    @torch.enable_grad()
    def closure():
        if opt is not None:
            opt.zero_grad(set_to_none=True)
        else:
            log_t.grad = None
        loss, _ = temp_nll_loss(log_t, rows, labels, None, n, CHUNK)
        loss.backward()
        return loss.detach()
    return closure


def torch_closure(rows, labels, log_t, dev, opt=None):
    """The reference's closure: per chunk (upload,) x / T, cross_entropy, backward, the chunk's loss read back."""
    n = labels.numel()

    @torch.enable_grad()
    def closure():
        if opt is not None:
            opt.zero_grad(set_to_none=True)
        else:
            log_t.grad = None
        total = 0.0
        for i in range(0, n, CHUNK):
            j = min(i + CHUNK, n)
            x = rows[i:j].to(dev, non_blocking=True)
            y = labels[i:j].to(dev, non_blocking=True)
            t = log_t.exp().clamp_min(1e-3)
            loss = torch.nn.functional.cross_entropy(x / t, y, reduction="sum") / n
            loss.backward()
            total += float(loss.item())
        return torch.tensor(total, device=dev)
    return closure


def time_closure(closure, runs):
    for _ in range(3):
        closure()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        closure()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / runs * 1e3


def time_fit(make_closure, dtype, dev, fits):
    ms, temps, evals = [], [], []
    for k in range(fits + 1):                              # the first one warms up
        log_t = torch.nn.Parameter(torch.zeros(1, dtype=dtype, device=dev))
        opt = torch.optim.LBFGS([log_t], lr=1.0, max_iter=100, line_search_fn="strong_wolfe", history_size=100, tolerance_grad=1e-10,
                                tolerance_change=1e-12)
        closure = make_closure(log_t, opt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.step(closure)
        temp = float(log_t.exp().item())
        if k:
            ms.append((time.perf_counter() - t0) * 1e3)
            temps.append(temp)
            evals.append(opt.state[log_t]["func_evals"])
    return statistics.median(ms), temps[-1], evals[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4 * 64 * 2048)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--fits", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: this tool measures on the device only")
    dev = torch.device("cuda:0")
    rows, labels = make_rows(args.rows, args.classes, torch.Generator().manual_seed(0))
    rows_d, labels_d = rows.to(dev), labels.to(dev)
    rows_h, labels_h = rows.pin_memory(), labels.pin_memory()
    variants = (
        ("fused (`ops.temp_nll`, resident cache)", torch.float64, lambda lt, opt=None: fused_closure(rows_d, labels_d, lt, opt)),
        ("torch ops, cache in pinned host memory", torch.float32, lambda lt, opt=None: torch_closure(rows_h, labels_h, lt, dev, opt)),
        ("torch ops, cache on the device", torch.float32, lambda lt, opt=None: torch_closure(rows_d, labels_d, lt, dev, opt)),
    )
    out = []
    for name, dtype, make in variants:
        log_t = torch.zeros(1, dtype=dtype, device=dev, requires_grad=True)
        ev = time_closure(make(log_t), args.runs)
        fit, temp, evals = time_fit(make, dtype, dev, args.fits)
        out.append((name, ev, fit, temp, evals))
    print(f"| closure ({torch.cuda.get_device_name(0)}, N = {args.rows}, C = {args.classes}) | one evaluation, ms (mean of {args.runs}) | "
          f"x fused | LBFGS fit, ms (median of {args.fits}) | x fused | evaluations | T |")
    print("|---|---|---|---|---|---|---|")
    for name, ev, fit, temp, evals in out:
        print(f"| {name} | {ev:.3f} | {ev / out[0][1]:.1f} | {fit:.1f} | {fit / out[0][2]:.1f} | {evals} | {temp:.6f} |")


if __name__ == "__main__":
    main()
