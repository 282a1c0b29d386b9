#!/usr/bin/env python
"""Development aid: two builds of the library on the per-pixel loss / metric / uncertainty kernels (csrc/class_column.h), same seeded inputs.

    python tools/class_column_ab.py OLD.so NEW.so [--time] [--only SUBSTR] [--out DIR]

One child process per library and run (the parent process never touches the GPU).  Default: every entry point of the family at
(3, C, 5, 87) for C in 3, 21, 32, at (1, 20, 2, 100) (one block: the fp64 sums have a fixed order there) and at (4, 20, 64, 2048), every
kind / act / mode / form / reduction, three runs per library.  Per-pixel outputs and integer counts are compared by SHA-256; for sums whose
order is not fixed d0 = largest difference among the three OLD runs, d1 = largest of the three NEW-OLD differences, and d1 <= 2 d0 is asked
(d1 = 0 where d0 = 0).  --time: device-event time per entry point at (4, 20, 64, 2048), OLD and NEW alternating, three rounds each; asked:
median(NEW) <= median(OLD) + (max - min)(OLD).  --only: the calls whose name contains SUBSTR.  The `tversky_fwd dyadic` calls feed probabilities
that are multiples of 1/256: every partial sum is then exact, so their outputs must agree bit for bit whatever the order of the atomics.
Exit status 1 if anything asked fails."""
import hashlib
import itertools
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 3, 5, 87), (3, 21, 5, 87), (3, 32, 5, 87), (1, 20, 2, 100), (4, 20, 64, 2048)]
DIR_KINDS = [("nll_dircat", [0.0]), ("digamma_ce", [0.0]), ("brier", [-1.0]), ("brier", [40.0]), ("mse", [0.0]), ("kl_off_uniform", [0.0]),
             ("complement_kl", [1.25, 0.65, 0.15, -1.0, 1.0, 1.0]), ("complement_kl", [1.0, 0.5, 0.1, 30.0, 0.0, 0.0]),
             ("wrong_low_evidence", [2.0, 0.1, 0.05]), ("wrong_low_evidence", [4.0, 0.1, 0.0]), ("kl_off_uniform_weighted", [2.5])]


def calls(shape, t_mc):
    """[(name, thunk -> {output name: tensor})]; names starting with '~' are sums whose order is not fixed (beyond one block)"""
    import torch
    from semanticlidarunc_amd import ops
    from semanticlidarunc_amd.models import probability_helper as ph
    b, c, h, w = shape
    gen, dev = torch.Generator().manual_seed(1000 * c + h * w), torch.device("cuda:0")
    logits = torch.randn(b, c, h, w, generator=gen) * 2.0
    lab = torch.randint(1, c, (b, h, w), generator=gen)                                   # labels as the tests' _labels builds them
    lab[torch.rand((b, h, w), generator=gen) < 0.1] = 0
    lab.reshape(-1)[torch.randperm(b * h * w, generator=gen)[:9]] = torch.tensor([-1, c, 255] * 3)
    head_in = torch.cat([logits, torch.randn(b, 1, h, w, generator=gen) * 3.0 + 3.0], 1)
    head_in[0, c, 0, :3] = 25.0
    mc = (torch.randn(t_mc, 1 if t_mc > 2 else b, c, h, w, generator=gen) * 2.0).to(dev)
    dense, coef = torch.randn(b, c, h, w, generator=gen).to(dev), (torch.rand(2, c, generator=gen) * 1e-3).to(dev)
    logits, lab, head_in = logits.to(dev), lab.to(dev), head_in.to(dev)
    probs, logp, alpha = logits.softmax(1), logits.log_softmax(1), 1.0 + torch.nn.functional.softplus(logits) * 10.0
    by_act, by_mode = {"logits": logits, "probs": probs, "log_probs": logp}, {"logits": logits, "probs": probs, "alpha": alpha}
    gs, one = torch.tensor([0.37], device=dev), b * h * w <= 256
    S = "" if one else "~"
    edges = torch.linspace(0, 1, 16, device=dev)
    out = []
    for kind, x, prm in ((0, logits, 0.0), (1, probs, 1e-8), (2, probs, 1e-8), (3, logp, 0.0)):
        for ign in (0, None):
            out.append((f"nll_fwd k{kind} ign={ign}", lambda x=x, kind=kind, prm=prm, ign=ign: dict(zip((S + "sum", "count"), ops.nll_fwd(x, lab, kind, prm, ign)))))
        out.append((f"nll_bwd k{kind}", lambda x=x, kind=kind, prm=prm: {"grad": ops.nll_bwd(x, lab, kind, prm, 0, gs)}))
    out.append(("softmax_nll", lambda: dict(zip(("probs", S + "sum"), ops.softmax_nll(logits, lab)))))
    out.append(("softmax_loss_bwd", lambda: {"grad": ops.softmax_loss_bwd(probs, lab, dense, 0.5, 1.0, 1e-8, gs)}))
    out.append(("softmax_loss_bwd bare", lambda: {"grad": ops.softmax_loss_bwd(probs)}))
    for act, x in by_act.items():
        for red in ("mean", "sum", "none"):
            out.append((f"tversky_fwd {act} {red}", lambda x=x, act=act, red=red: dict(zip(("~loss", "~coef", "any"), ops.tversky_fwd(x, lab, act, 255, 0.7, 0.3, 1.0, red)))))
        for go in (torch.ones(1, device=dev), torch.linspace(0.5, 1.5, c, device=dev)):
            out.append((f"tversky_bwd {act} go{go.numel()}", lambda x=x, act=act, go=go: {"grad": ops.tversky_bwd(x, lab, act, 255, 0.7, 0.3, coef, go)}))
    dyadic = (probs * 256.0).round() / 256.0       # every partial sum of tversky_sums is then exact in fp32: the order of its atomics cannot show
    for red in ("mean", "sum", "none"):
        out.append((f"tversky_fwd dyadic probs {red}", lambda red=red: dict(zip(("loss", "coef", "any"), ops.tversky_fwd(dyadic, lab, "probs", 255, 0.7, 0.3, 1.0, red)))))
    for kind, prm in DIR_KINDS:
        out.append((f"dirichlet_loss_fwd {kind} {prm}", lambda kind=kind, prm=prm: dict(zip((S + "sums", "count"), ops.dirichlet_loss_fwd_ex(alpha, lab, kind, prm, 1e-12, 0)))))
        out.append((f"dirichlet_loss_bwd {kind} {prm}", lambda kind=kind, prm=prm: {"grad": ops.dirichlet_loss_bwd_ex(alpha, lab, kind, prm, 1e-12, 0, gs)}))
    out.append(("dirichlet_loss_fwd plain mse", lambda: dict(zip((S + "sum", "count"), ops.dirichlet_loss_fwd(alpha, lab, "mse", 0.0, 1e-12, None)))))
    out.append(("dirichlet_loss_bwd plain mse", lambda: {"grad": ops.dirichlet_loss_bwd(alpha, lab, "mse", 0.0, 1e-12, None, gs)}))
    out.append(("dirichlet_head", lambda: dict(zip(("alpha", "p_hat", "H", "AU", "preds"), ph._launch_head(head_in[:, :c], head_in[:, c:], 1.0, 1e-8, True, True, True, True, True)))))
    out.append(("dirichlet_uncertainty", lambda: dict(zip(("H", "AU"), ph._uncertainty(alpha, None, True, True)))))
    for ign in (0, None):
        def ece(ign=ign):
            n, ok, cf = torch.zeros(15, dtype=torch.int64, device=dev), torch.zeros(15, dtype=torch.float64, device=dev), torch.zeros(15, dtype=torch.float64, device=dev)
            ops.ece_update(probs, lab, n, ok, cf, ign)
            return {"count": n, "sum_correct": ok, "~sum_conf": cf}
        out.append((f"ece_update ign={ign}", ece))
        for mode, x in by_mode.items():
            out.append((f"ece_samples {mode} ign={ign}", lambda x=x, mode=mode, ign=ign: dict(zip(("conf", "flag"), ops.ece_samples(x, lab, mode, ign)))))
    conf, flag = ops.ece_samples(probs, lab, "probs", 0)
    u, ok = conf.reshape(-1).contiguous(), (flag.reshape(-1) == 1).to(torch.uint8)
    out.append(("binned_counts", lambda: dict(zip(("count", "n_correct"), ops.binned_counts(u, ok, edges)))))
    out.append(("binned_stats", lambda: dict(zip(("count", "n_correct", "~sum_u"), ops.binned_stats(u, ok, edges)))))
    for (mode, x), score in itertools.product(by_mode.items(), ops.AUROC_SCORES):
        out.append((f"auroc_scores {mode} {score}", lambda x=x, mode=mode, score=score: dict(zip(("score", "flag"), ops.auroc_scores(x, lab, mode, score, 0)))))
    out.append(("auroc_scores override", lambda: dict(zip(("score", "flag"), ops.auroc_scores(probs, lab, "probs", "entropy", None, score_override=conf)))))
    for name, kw in (("maxprob", {"use_max_prob_confidence": True}), ("ent_mc", {"ent_mc": conf}), ("entropy", {})):
        out.append((f"aurc_samples {name}", lambda kw=kw: dict(zip(("conf", "flag"), ops.aurc_samples(probs, lab, 0, **kw)))))
    out.append((f"mc_reduce T={t_mc}", lambda: dict(zip(("p_bar", "H", "MI", "preds"), ops.mc_reduce(mc)))))
    out.append(("softmax_entropy", lambda: dict(zip(("probs", "H", "preds"), ops.softmax_entropy(logits)))))
    preds = logits.argmax(1)

    def confusion():
        cm = torch.zeros(c, c, dtype=torch.int64, device=dev)
        ops.confusion_update(cm, preds, lab)
        return {"cm": cm}
    out.append(("confusion_update", confusion))
    out.append(("ua_samples", lambda: dict(zip(("u", "flag"), ops.ua_samples(lab, preds, conf, (0,))))))
    out.append(("group_by_class", lambda: {"counts": ops.group_by_class(lab.reshape(-1), u, c)[1]}))
    return out


def child(lib, time_it, path, only):
    import torch
    sys.path.insert(0, ROOT)
    from semanticlidarunc_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib)
    res = {}
    for shape in ([SHAPES[-1]] if time_it else SHAPES):
        for t_mc in ((8,) if time_it else (2, 8) if shape == SHAPES[-1] else (2,)):
            for name, fn in calls(shape, t_mc):
                if only not in name or (not time_it and t_mc == 8 and not name.startswith("mc_reduce")):
                    continue
                key = f"{shape} {name}"
                if time_it:
                    def span(n):
                        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(n):
                            fn()
                        z.record()
                        z.synchronize()
                        return a.elapsed_time(z) / n
                    n = max(10, math.ceil(250.0 / max(span(5), 1e-3)))          # 5 warm-up launches, then a window of 0.25 s or more
                    res[key] = span(n)
                else:
                    for k, v in fn().items():
                        v = v.detach().cpu()
                        res[f"{key}: {k}"] = v.double().reshape(-1).tolist() if k.startswith("~") else hashlib.sha256(v.numpy().tobytes()).hexdigest()
    json.dump(res, open(path, "w"))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3] == "time", sys.argv[4], sys.argv[5])
    old, new = sys.argv[1], sys.argv[2]
    time_it = "--time" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "."
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    os.makedirs(out, exist_ok=True)
    runs = {"old": [], "new": []}
    for i, (tag, lib) in itertools.product(range(3), (("old", old), ("new", new))):       # alternating
        path = os.path.join(out, f"{'time' if time_it else 'outputs'}_{tag}{i}.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "time" if time_it else "out", path, only], check=True, timeout=900)
        runs[tag].append(json.load(open(path)))
    bad = 0
    if time_it:
        print("| entry point | OLD ms (3 rounds) | NEW ms (3 rounds) | OLD median + range | NEW median | ok |\n|---|---|---|---|---|---|")
        for k in runs["old"][0]:
            o, n = [r[k] for r in runs["old"]], [r[k] for r in runs["new"]]
            lim, med = statistics.median(o) + max(o) - min(o), statistics.median(n)
            bad += med > lim
            print(f"| {k} | {' '.join(f'{v:.4f}' for v in o)} | {' '.join(f'{v:.4f}' for v in n)} | {lim:.4f} | {med:.4f} | {'yes' if med <= lim else 'NO'} |")
    else:
        diff = lambda a, b: max((0.0 if x != x and y != y else math.inf if x != x or y != y else abs(x - y)) for x, y in zip(a, b))
        exact = [k for k in runs["old"][0] if ": ~" not in k]
        wrong = [k for k in exact if len({r[k] for r in runs["old"] + runs["new"]}) != 1]
        print(f"{len(exact) - len(wrong)} of {len(exact)} per-pixel / integer / one-block outputs have the same bits in all six runs")
        for k in wrong:
            print("DIFFERENT BITS:", k)
        print("| sum | d0 | d1 | ok |\n|---|---|---|---|")
        for k in (k for k in runs["old"][0] if ": ~" in k):
            d0 = max(diff(a[k], b[k]) for a, b in itertools.combinations(runs["old"], 2))
            d1 = max(diff(a[k], b[k]) for a, b in zip(runs["new"], runs["old"]))
            ok = d1 <= 2 * d0
            bad += not ok
            print(f"| {k} | {d0:.3e} | {d1:.3e} | {'yes' if ok else 'NO'} |")
        bad += len(wrong)
    print("FAILED:" if bad else "all accepted;", bad, "not accepted")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
