"""Value-branch cases for the three class-column files that produce the uncertainty numbers (csrc/dirichlet_loss.hip, csrc/dirichlet.hip,
csrc/uncertainty.hip): their control flow depends on the values of a pixel's class column (eps clamps, gates, ties, the number of
digamma recurrence steps, the softplus switch), not on its shape.  This module holds the case tables, the seeded input builders and
the references; no GPU here.  ``tests/test_dirichlet_value_cases_cpu.py`` shows that every input is fair (same decisions in fp32 and
fp64, every branch outcome present, fp32 oracle well inside the bar) and ``tests/test_gpu_dirichlet_value_edges.py`` holds the kernels
to the fp64 results.  Conventions (``Case`` / ``Family`` / the printed comparison line) are those of tests/pixel_edge_cases.py.

A case is one loss (or kernel) x one regime x C in {20, 32} (both slu_class_cap instantiations; C = 3 too where the op starts at three
classes) at [2, C, 1, 67] (134 pixels: a wave plus three lanes per image), and at [1, C, 1, 1] where the regime is one special column.
References: the functions of oracle/dirichlet.py and oracle/uncertainty.py in fp64 (the yardstick) and in fp32 on the same fp32 inputs;
every backward is ``torch.autograd.grad`` of the forward.

Bars.  The coefficients are the project's: loss value 1e-5, loss gradient 2e-5 (weighted KL 3e-5), alpha 2e-6 and p_hat 3e-6 relative,
H and H_norm 1e-5, AU and EU 3e-5, MC p_bar and single-pass probs 1e-6, MI 1e-5, preds exact.  Two scales differ from the older tests:
a loss value is judged relative to |fp64 value| (not max(1, .)), and a gradient per pixel against the largest |fp64 gradient| of that
pixel's own class column.  Where fp32 cannot reach the coefficient (``GAP_BOUND``, an explicit list) the bar is
max(coefficient x scale, 4 x the largest |fp32 oracle - fp64| of that result over the case); elsewhere the coefficient term alone
binds and the fp32 oracle must lie within a quarter of it on every pixel.  Where the bar is 0 the device must return exactly 0.

Labels of a loss case: about 10 % carry the ignore value 0.  None of the oracle's loss functions accepts a label outside [0, C) (its
``gather`` raises), so the tabled cases carry none; the GPU file checks separately that -1, C and 255 count like the ignore value.
The labelled class of a counted pixel is never a zeroed class (psi(0) is infinite).
"""
from __future__ import annotations

import math
import zlib
from typing import Callable, Dict, NamedTuple, Optional

import torch
import torch.nn.functional as F

from oracle import dirichlet as odir
from oracle import uncertainty as ounc
from pixel_edge_cases import Case, Family, case_id  # noqa: F401  (conventions shared with the edge-shape tables)

SHAPE, ONE = (2, 1, 67), (1, 1, 1)          # (B, H, W)
VALUE_COEF = 1e-5

# cases whose first seed failed a CPU condition (conditioning or decision agreement) and the seed offset that replaced it
SALTS: Dict[str, int] = {
    "complement_kl_gated typical C3 2x3x1x67": 2,
    "kl_off_weighted_g1 confident-wrong C32 2x32x1x67": 1,
    "kl_off_weighted_g2.5 confident-wrong C20 2x20x1x67": 1,
    "complement_kl large-evidence C3 2x3x1x67": 2,
    "complement_kl_gated large-evidence C3 2x3x1x67": 18,
    "head randn4 T0.5 C32": 2,
    "head randn4 T1.0 C32": 1,
    "mc_reduce identical passes T7 C20": 1,
    "mc_reduce randn3 T1 C32": 1,
    "mc_reduce offset+1e4 T1 C32": 2,
    "mc_reduce identical passes T2 C32": 3,
    "mc_reduce identical passes T7 C32": 1,
    "softmax_entropy neg-inf class C20": 1,
    "softmax_entropy randn3 C32": 1,
    "softmax_entropy neg-inf class C32": 1,
    "complement_kl sub-one C3 2x3x1x67": 2,
    "complement_kl_gated sub-one C3 2x3x1x67": 18,
    "mse mixed C3 2x3x1x67": 4,
    "complement_kl mixed C3 2x3x1x67": 1,
    "complement_kl_gated mixed C3 2x3x1x67": 4,
}
# ... and the cases that no seed helps, with the exponent range (low, width) that replaced the regime's: with three classes nearly every
# draw of 10^U(-6, 0) or 10^(-3 + 7 U) has pixels where one class holds all but 1e-3 of the mass, which is the confident-right regime
# (gap-bound) by another name
SCALES: Dict[str, tuple] = {
    "complement_kl sub-one C3 2x3x1x67": (-2.0, 2.0),
    "complement_kl_gated sub-one C3 2x3x1x67": (-1.0, 1.0),
    "mse mixed C3 2x3x1x67": (-2.0, 5.0),
    "complement_kl mixed C3 2x3x1x67": (-1.0, 3.0),
    "complement_kl_gated mixed C3 2x3x1x67": (-1.0, 2.0),
}


def gen(case: Case) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(case.id.encode()) + SALTS.get(case.id, 0))


# ---------------------------------------------------------------------------------------------------------------------
# the 13 loss forms: the 11 modules of test_gpu_dirichlet_losses._modules() and the weighted KL at gamma = 1 and 2.5
# ---------------------------------------------------------------------------------------------------------------------
class Loss(NamedTuple):
    kind: str                      # nll | digamma | brier | mse | kl | klw | ckl | wle
    oracle: Callable               # (alpha, labels [B, H, W]) -> scalar
    ignore: Optional[int]
    eps: float
    grad_coef: float
    prm: dict


def _ckl(**kw):
    prm = dict(gamma=2.0, tau=0.55, sigma=0.12, s_target=None, normalize=True, detach_uncert=True)
    prm.update(kw)
    return Loss("ckl", lambda a, l: odir.loss_complement_kl(a, l, 0, eps=1e-8, **prm), 0, 1e-8, 2e-5, prm)


def _wle(ignore, **kw):
    prm = dict(s_low=0.0, margin=0.05, soft_margin_k=0.08)
    prm.update(kw)
    return Loss("wle", lambda a, l: odir.loss_wrong_low_evidence(a, l, ignore, eps=1e-8, **prm), ignore, 1e-8, 2e-5, prm)


def _klw(gamma):
    return Loss("klw", lambda a, l: odir.loss_kl_off_uniform(a, l, 0, with_conf_weighting=True, gamma=gamma), 0, 1e-8, 3e-5, dict(gamma=gamma))


LOSSES: Dict[str, Loss] = {
    "nll_dircat": Loss("nll", lambda a, l: odir.loss_nll_dircat(a, l, 0), 0, 1e-12, 2e-5, {}),
    "digamma_ce": Loss("digamma", lambda a, l: odir.loss_digamma_ce(a, l, 0), 0, 1e-8, 2e-5, {}),
    "brier": Loss("brier", lambda a, l: odir.loss_brier(a, l, 0), 0, 1e-12, 2e-5, {}),
    "brier_sref40": Loss("brier", lambda a, l: odir.loss_brier(a, l, 0, 40.0), 0, 1e-12, 2e-5, dict(s_ref=40.0)),
    "mse": Loss("mse", lambda a, l: odir.loss_mse(a, l, 0), 0, 1e-8, 2e-5, {}),
    "kl_off_uniform": Loss("kl", lambda a, l: odir.loss_kl_off_uniform(a, l, 0), 0, 1e-8, 2e-5, {}),
    "kl_off_weighted_g1": _klw(1.0),
    "kl_off_weighted_g2.5": _klw(2.5),
    "complement_kl": _ckl(gamma=1.25, tau=0.65, sigma=0.15),
    "complement_kl_gated": _ckl(s_target=30.0, normalize=False, detach_uncert=False),
    "wrong_low_evidence": _wle(0),
    "wrong_low_evidence_hard": _wle(0, s_low=4.0, margin=0.1, soft_margin_k=0.0),
    "wrong_low_evidence_nomargin": _wle(None, margin=0.0),
}
WLE = [n for n, l in LOSSES.items() if l.kind == "wle"]
FROM_THREE = ["mse", "complement_kl", "complement_kl_gated"]          # the ops whose kernels start at C = 3

# regime -> (the losses it is for, also as one column: for all of them, none, or the listed ones).  docs/why: the table of profiles/r25/README.md
EVERY = list(LOSSES)
REGIMES = {
    "typical": (EVERY, False),               # control: 1 + 10 softplus(2 randn), the one distribution the older tests draw from
    "evidence-free": (EVERY, True),          # alpha = 1: (alpha~ - 1) = 0, lgamma(1), tie of all classes -> pred 0, hinge exactly 0
    "sub-one": (EVERY, False),               # 10^U(-6, 0): sixth step of digamma_pos / trigamma_pos, lgammaf of small arguments
    "clamped": (EVERY, False),               # 1 + U(0, 1), 4 classes exactly 0: fmaxf(., eps), tl < eps, live = false
    "clamped-tiny": (EVERY, False),          # the same with 1e-10 (< eps = 1e-8) in those classes
    "all-zero": (["nll_dircat", "brier", "brier_sref40", "mse"] + WLE, True),          # a0 < eps, the pmax = -1 start, zero gradient
    "confident-right": (EVERY, False),       # alpha_y = 1e4 (1 + U), rest 1: pred == y; sum of the weights < 1 -> host clamp
    "saturated": (EVERY, True),              # alpha_y = 1e12, rest 1: den_raw < eps (fp64 too: (C - 1) / 1e12 < 1e-8)
    "saturated-hard": (["kl_off_weighted_g1", "kl_off_weighted_g2.5"], True),          # alpha_y = 1e20: (1 - p_y)^gamma is 0 in fp64 too
    "confident-wrong": (EVERY, False),       # alpha_k = 10^U(2, 4) for one k != y, rest 1 + U: gate fully on, large hinge, small p_y
    "confident-wrong-tiny": (EVERY, ["complement_kl", "complement_kl_gated"]),          # alpha_y = 1e-10 beside alpha_k = 1e3: py_raw < eps
    "margin-sides": (WLE, False),            # p_max - p_y = margin + {0.01, -0.01, 0.2, -0.2}: both sides of the soft and the hard margin
    "tie-label-lower": (WLE, True),          # top two classes bit-equal, the label is the lower index: first maximum = y, gate 0
    "tie-label-higher": (WLE, True),         # the label is the higher index: wrong with gap 0: gate 1 / sigmoid(-margin / k) / 0
    "wrong-low-total": (WLE, False),         # wrong with a gap of 0.6 but alpha0 = C / 2 <= C + s_low: h == 0 on a gated pixel
    "large-evidence": (EVERY, False),        # 10^(3 + 2 U) in every class: lgamma / digamma cancellation at S up to 2e6
    "mixed": (EVERY, False),                 # 10^(-3 + 7 U): magnitudes that differ by pixel and by class within a pixel
}

# Where the fp32 evaluation of the reference's own formula cannot meet the coefficient: (loss kind, regime) -> (results, reason).
# An explicit list (the CPU test asserts that nothing else needs it); the figures are in profiles/r25/README.md.
_RESIDUE = "gradient entries are cancellation residues whose fp32 error exceeds their fp64 magnitude"
GAP_BOUND: Dict[tuple, tuple] = {}
_KL, _ALL = ("kl", "klw"), ("value", "grad")


def _gap(kinds, regimes, results, reason):
    for k in kinds:
        for r in regimes:
            GAP_BOUND[(k, r)] = (results, reason)


_gap(_KL, ["large-evidence"], _ALL, "lgamma(S) - sum lgamma(alpha~) and the digamma differences cancel at S up to 2e6")
_gap(("ckl",), ["evidence-free", "confident-right", "saturated"], _ALL, "1 - p_y and sum tl log tl + ln(C - 1) are residues of fp32 rounding; the " + _RESIDUE)
_gap(_KL, ["evidence-free", "confident-right"], ("grad",), "(alpha~ - 1) trigamma(alpha~) - trigamma(S) sum(alpha~ - 1) is 0 at alpha~ = 1: the " + _RESIDUE)
_gap(("kl",), ["saturated"], ("grad",), "as evidence-free: every alpha~ is 1")
_gap(("klw",), ["saturated"], _ALL, "the weight 1 - p_y = 1.9e-11 is 0 in fp32")
_gap(("nll", "digamma"), ["confident-right", "saturated"], ("value",), "the value is alpha0 - alpha_y = C - 1 over alpha0, below an ulp of alpha0 at 1e12 and a few ulps at 1e4")
_gap(("brier", "mse"), ["confident-right", "saturated"], _ALL, "the value and its gradient are of order (C - 1) / alpha0, sums of terms of order 1 that cancel")


def gap_bound(case: Case, result: str) -> bool:
    if case.family != "loss":
        return False
    entry = GAP_BOUND.get((LOSSES[case.p["loss"]].kind, case.p["regime"]))
    return entry is not None and result in entry[0]


def _loss_cases():
    cs = []
    for regime, (names, column) in REGIMES.items():
        for name in names:
            for c in (3, 20, 32):
                if c == 3 and name not in FROM_THREE:
                    continue
                for shape in ((SHAPE, ONE) if column is True or (column and name in column) else (SHAPE,)):
                    cs.append(Case("loss", f"{name} {regime} C{c} {'column' if shape == ONE else 'x'.join(map(str, (shape[0], c) + shape[1:]))}",
                                   dict(loss=name, regime=regime, c=c, shape=shape)))
    return cs


def _labels(shape, c, g):
    lab = torch.randint(1, c, shape, generator=g)
    if lab.numel() > 1:
        lab[torch.rand(shape, generator=g) < 0.1] = 0
    return lab


def _set(alpha, idx, value):
    """alpha[b, idx[b, h, w], h, w] = value"""
    value = value if torch.is_tensor(value) else torch.full(idx.shape, float(value))
    return alpha.scatter(1, idx.unsqueeze(1), value.unsqueeze(1).to(alpha.dtype))


def _other_class(lab, c, g):
    """one class k != label per pixel"""
    return (lab + 1 + torch.randint(0, c - 1, lab.shape, generator=g)) % c


def _zeroed(alpha, lab, c, g, value):
    """min(4, C - 2) classes per pixel, never the labelled one, set to `value`"""
    score = _set(torch.rand(alpha.shape, generator=g), lab, 2.0)
    idx = score.topk(min(4, c - 2), dim=1, largest=False).indices
    return alpha.scatter(1, idx, value)


def _loss_build(case: Case):
    g, p = gen(case), case.p
    c, (b, h, w), regime, loss = p["c"], p["shape"], p["regime"], LOSSES[p["loss"]]
    lab = _labels(p["shape"], c, g)
    full = (b, c, h, w)
    rand = lambda *s: torch.rand(s or full, generator=g)          # noqa: E731
    if regime == "typical":
        alpha = 1.0 + F.softplus(torch.randn(full, generator=g) * 2.0) * 10.0
    elif regime == "evidence-free":
        alpha = torch.ones(full)
    elif regime == "sub-one":
        lo, width = SCALES.get(case.id, (-6.0, 6.0))
        alpha = 10.0 ** (lo + width * rand())
    elif regime in ("clamped", "clamped-tiny"):
        alpha = _zeroed(1.0 + rand(), lab, c, g, 0.0 if regime == "clamped" else 1e-10)
    elif regime == "all-zero":
        alpha = torch.zeros(full)
    elif regime == "confident-right":
        alpha = _set(torch.ones(full), lab, 1e4 * (1.0 + rand(b, h, w)))
    elif regime in ("saturated", "saturated-hard"):
        alpha = _set(torch.ones(full), lab, 1e12 if regime == "saturated" else 1e20)
    elif regime == "confident-wrong":
        alpha = _set(1.0 + rand(), _other_class(lab, c, g), 10.0 ** (2.0 + 2.0 * rand(b, h, w)))
    elif regime == "confident-wrong-tiny":
        alpha = _set(_set(1.0 + rand(), lab, 1e-10), _other_class(lab, c, g), 1e3)
    elif regime == "margin-sides":
        # a two-class contest: the classes k and y share 0.9, the others 0.1; p_k - p_y = margin + delta (negative: y is the maximum)
        margin = loss.prm["margin"] or 0.05
        delta = torch.tensor([0.01, -0.01, 0.2, -0.2])[torch.arange(b * h * w) % 4].reshape(b, h, w)
        d = margin + delta
        prob = _set(_set(torch.full(full, 0.1 / (c - 2)), lab, (0.9 - d) / 2), _other_class(lab, c, g), (0.9 + d) / 2)
        alpha = prob * (c * 10.0 ** (1.0 + 2.0 * rand(b, 1, h, w)))
    elif regime in ("tie-label-lower", "tie-label-higher"):
        lo = torch.randint(1, c - 1, (b, h, w), generator=g)
        hi = lo + 1 + (torch.rand((b, h, w), generator=g) * (c - 1 - lo).float()).long().clamp_max(c - 2 - lo)
        top = 3.0 + 10.0 ** (1.0 + rand(b, h, w))
        alpha = _set(_set(1.0 + rand(), lo, top), hi, top)
        keep = (lab == 0) if loss.ignore == 0 else torch.zeros_like(lab, dtype=torch.bool)          # the ignored pixels stay ignored
        lab = torch.where(keep, lab, lo if regime == "tie-label-lower" else hi)
    elif regime == "wrong-low-total":
        prob = _set(_set(torch.full(full, 0.2 / (c - 2)), lab, 0.1), _other_class(lab, c, g), 0.7)
        alpha = prob * (0.5 * c)
    elif regime == "large-evidence":
        alpha = 10.0 ** (3.0 + 2.0 * rand())
    elif regime == "mixed":
        lo, width = SCALES.get(case.id, (-3.0, 7.0))
        alpha = 10.0 ** (lo + width * rand())
    else:
        raise ValueError(regime)
    return dict(alpha=alpha.float().contiguous(), labels=lab)


def _loss_ref(case: Case, i, dt):
    a = i["alpha"].detach().to(dt).requires_grad_(True)
    v = LOSSES[case.p["loss"]].oracle(a, i["labels"])
    (g,) = torch.autograd.grad(v, a)
    return dict(value=v.detach(), grad=g.detach())


# ---------------------------------------------------------------------------------------------------------------------
# the branch predicates of dirichlet_loss_kernel, evaluated with torch in `dt` over the counted pixels (rows of [n, C])
# ---------------------------------------------------------------------------------------------------------------------
def _steps(x, most):
    """how many of the `most` recurrence steps slu_digamma_steps / trigamma_pos take at x"""
    n = torch.zeros_like(x, dtype=torch.int64)
    for _ in range(most):
        take = x < 6.0
        n += take
        x = torch.where(take, x + 1.0, x)
    return n


def counted_rows(i, loss: Loss):
    """(alpha rows [n, C] fp32, labels [n], mask [B, H, W]) of the counted pixels"""
    a, lab = i["alpha"], i["labels"]
    mask = torch.ones_like(lab, dtype=torch.bool) if loss.ignore is None else lab != loss.ignore
    rows = a.permute(0, 2, 3, 1).reshape(-1, a.shape[1])[mask.reshape(-1)]
    return rows, lab.reshape(-1)[mask.reshape(-1)], mask


def loss_decisions(case: Case, i, dt):
    """name -> tensor (bool or int64) with one row per counted pixel; the scalars of the host side have one row"""
    loss = LOSSES[case.p["loss"]]
    rows, y, _ = counted_rows(i, loss)
    a = rows.to(dt)
    n, c = a.shape
    eps = torch.tensor(loss.eps, dtype=dt)
    hot = torch.zeros(n, c, dtype=torch.bool).scatter_(1, y[:, None], True)
    a0, ay = a.sum(1), a.gather(1, y[:, None])[:, 0]
    out = {}
    if loss.kind == "digamma":
        out["sixth step"] = torch.stack([_steps(a0, 6), _steps(ay, 6)], 1) == 6
    elif loss.kind in ("kl", "klw"):
        at = torch.where(hot, torch.ones_like(a), a).clamp_min(eps)
        out["live"] = (a >= eps) & ~hot
        out["sixth step"] = (_steps(at, 6) == 6) & ~hot
        out["steps of S"] = _steps(at.sum(1), 6)
        if loss.kind == "klw":
            om = (1.0 - ay / (a0 + eps)).clamp(0.0, 1.0)
            out["sum of weights < 1"] = ((om ** loss.prm["gamma"]).sum() < 1.0).reshape(1)
    elif loss.kind == "ckl":
        d = a0 + eps
        py_raw = ay / d
        den_raw = 1.0 - py_raw.clamp_min(eps)
        tl = (a / d[:, None]) / den_raw.clamp_min(eps)[:, None]
        out["py_raw < eps"], out["den_raw < eps"], out["tl < eps"] = py_raw < eps, den_raw < eps, (tl < eps) & ~hot
    elif loss.kind == "wle":
        d = a0.clamp_min(eps)
        p = a / d[:, None]
        top, pred = p.max(1)
        gap = top.clamp_min(eps) - (ay / d).clamp_min(eps)
        margin, k = loss.prm["margin"], loss.prm["soft_margin_k"]
        gate = (pred != y).to(dt)
        if margin > 0.0:
            gate = gate * (torch.sigmoid((gap - margin) / k) if k > 0.0 else (gap > margin).to(dt))
            if k == 0.0:
                out["m > margin"] = gap > margin
        h = torch.relu(d.log() - math.log(c + loss.prm["s_low"] + loss.eps))
        out["a0 >= eps"], out["pred"], out["pred != y"], out["h > 0"] = a0 >= eps, pred, pred != y, h > 0
        out["gated with h == 0"] = (gate > 0) & (h == 0)
        out["sum of gates < 1"] = (gate.sum() < 1.0).reshape(1)
        out["sum of gates == 0"] = (gate.sum() == 0.0).reshape(1)
    return out


def zero_gradient_mask(case: Case, i):
    """entries whose reference gradient is exactly 0 by construction: ignored pixels; the true class and the clamped entries of the KL
    kinds; every entry of a WrongLowEvidence pixel with pred == y"""
    loss = LOSSES[case.p["loss"]]
    a, lab = i["alpha"], i["labels"]
    _, _, counted = counted_rows(i, loss)
    mask = (~counted).unsqueeze(1).expand_as(a).clone()
    if loss.kind in ("kl", "klw"):
        mask |= torch.zeros_like(mask).scatter_(1, lab.unsqueeze(1), True) | (a < loss.eps)
    if loss.kind == "wle":
        mask |= (a.double().argmax(1) == lab).unsqueeze(1)
    return mask


# ---------------------------------------------------------------------------------------------------------------------
# the Dirichlet head from logits (dirichlet_kernel<., true>) and the measures of a given alpha (<., false>)
# ---------------------------------------------------------------------------------------------------------------------
SCALE_LOGITS = [-100.0, -20.0, 0.0, 19.999, 20.0, 20.001, 25.0, 80.0, 1e4]          # on, beside and far from the softplus switch at 20
TEMPERATURES = [0.5, 1.0, 4.0]
ALPHA_PLUS_ONE = [2.0, 2.5, 3.2, 4.3, 5.999, 6.0, 6.001, 1e3, 1e6]                  # every step count of digamma_ge1 below five, and none
HEAD_EPS = 1e-8


def _head_cases():
    cs = [Case("head", f"head {kind} T{t} C{c}", dict(kind=kind, t=t, c=c)) for kind in ("randn4", "spread200", "equal") for t in TEMPERATURES for c in (20, 32)]
    return cs


def _head_build(case: Case):
    g, p = gen(case), case.p
    c, (b, h, w) = p["c"], SHAPE
    if p["kind"] == "randn4":
        shape = torch.randn(b, c, h, w, generator=g) * 4.0
    elif p["kind"] == "spread200":          # most classes underflow to alpha = 1 + eps
        shape = torch.rand(b, c, h, w, generator=g) * 200.0
    else:
        shape = torch.randn(b, 1, h, w, generator=g).expand(b, c, h, w)
    scale = torch.tensor(SCALE_LOGITS)[torch.arange(b * h * w) % len(SCALE_LOGITS)].reshape(b, 1, h, w)
    # an evidence-free pixel (softplus(scale / T) below an ulp of 1) has alpha = 1 + eps in every class in fp32 and not quite in fp64:
    # its shape logits are all equal, so that the argmax is 0 in both
    flat = F.softplus(scale / p["t"]) < 1e-4
    shape = torch.where(flat, shape[:, :1].expand_as(shape), shape)
    return dict(outputs=torch.cat([shape, scale], 1).float().contiguous())


def _head_ref(case: Case, i, dt):
    c = case.p["c"]
    alpha, p_hat, h_norm, preds = odir.head(i["outputs"].to(dt), c, case.p["t"], HEAD_EPS)
    return dict(alpha=alpha, p_hat=p_hat, H_norm=h_norm, preds=preds, H=odir.predictive_entropy(alpha, HEAD_EPS),
                AU=odir.aleatoric(alpha, HEAD_EPS), EU=odir.epistemic(alpha, HEAD_EPS))


def head_decisions(case: Case, i, dt):
    c = case.p["c"]
    o = i["outputs"].to(dt)
    alpha = odir.alpha_from_shape_and_scale(o[:, :c], o[:, c:c + 1], case.p["t"], HEAD_EPS)
    return {"softplus argument > 20": (o[:, c] / case.p["t"] > 20.0).reshape(-1), "argmax": alpha.argmax(1).reshape(-1),
            "steps of alpha + 1": _steps(alpha + 1.0, 5).permute(0, 2, 3, 1).reshape(-1, c)}


def _alpha_cases():
    return [Case("alpha", f"alpha {kind} C{c}", dict(kind=kind, c=c)) for kind in ("ones", "steps", "mixed") for c in (20, 32)]


def _alpha_build(case: Case):
    g, p = gen(case), case.p
    c, (b, h, w) = p["c"], SHAPE
    if p["kind"] == "ones":
        alpha = torch.ones(b, c, h, w)
    elif p["kind"] == "steps":
        pick = (torch.arange(b * h * w)[:, None] * 3 + torch.arange(c)[None]) % len(ALPHA_PLUS_ONE)
        alpha = (torch.tensor(ALPHA_PLUS_ONE)[pick] - 1.0).reshape(b, h, w, c).permute(0, 3, 1, 2)
    else:          # below 1 too: the fifth step of digamma_ge1 (alpha + 1 < 2)
        alpha = 10.0 ** (-3.0 + 7.0 * torch.rand(b, c, h, w, generator=g))
    return dict(alpha=alpha.float().contiguous())


def _alpha_ref(case: Case, i, dt):
    a = i["alpha"].to(dt)
    return dict(H=odir.predictive_entropy(a, HEAD_EPS), H_norm=odir.predictive_entropy_norm(a, HEAD_EPS), AU=odir.aleatoric(a, HEAD_EPS),
                EU=odir.epistemic(a, HEAD_EPS))


def alpha_decisions(case: Case, i, dt):
    a = i["alpha"].to(dt)
    a0 = a.sum(1) + torch.tensor(HEAD_EPS, dtype=dt)
    return {"steps of alpha + 1": _steps(a + 1.0, 5).permute(0, 2, 3, 1).reshape(-1, a.shape[1]), "steps of alpha0 + 1": _steps(a0 + 1.0, 5).reshape(-1)}


# ---------------------------------------------------------------------------------------------------------------------
# MC reduction (mc_reduce_kernel, eps 1e-12) and the single pass (softmax_entropy_kernel, eps 1e-8)
# ---------------------------------------------------------------------------------------------------------------------
MC_EPS, SINGLE_EPS = 1e-12, 1e-8
LOGIT_KINDS = ("randn3", "spread40", "offset+1e4", "offset-1e4", "neg-inf class", "equal", "top-two equal")


def _mc_cases():
    cs = []
    for c in (20, 32):
        for t in (1, 2, 7):
            # bit-equal logits at T <= 2 only: a + b has one rounding, while torch's own sum of seven passes takes another order in the
            # tail of a vector loop than in its body, so the reference's p_bar would not tie in every pixel
            cs += [Case("mc", f"mc_reduce {kind} T{t} C{c}", dict(kind=kind, t=t, c=c)) for kind in LOGIT_KINDS if t <= 2 or kind != "top-two equal"]
            if t > 1:
                cs.append(Case("mc", f"mc_reduce identical passes T{t} C{c}", dict(kind="identical", t=t, c=c)))
        cs.append(Case("mc", f"mc_reduce swapped top two T2 C{c}", dict(kind="swap", t=2, c=c)))
    return cs


def _single_cases():
    return [Case("single", f"softmax_entropy {kind} C{c}", dict(kind=kind, t=1, c=c)) for c in (20, 32) for kind in LOGIT_KINDS]


def _logits(case: Case):
    g, p = gen(case), case.p
    t, c, (b, h, w), kind = p["t"], p["c"], SHAPE, p["kind"]
    full = (t, b, c, h, w)
    if kind == "spread40":          # p down to e^-40: below both eps values (1e-12 is 27.6 nats, 1e-8 is 18.4)
        x = (torch.rand(full, generator=g) - 0.5) * 40.0
    elif kind == "equal":
        x = (torch.randn(t, b, 1, h, w, generator=g) * 3.0).expand(full)
    elif kind == "identical":
        x = (torch.randn(1, b, c, h, w, generator=g) * 3.0).expand(full)
    else:
        x = torch.randn(full, generator=g) * 3.0
    x = x.clone()
    if kind.startswith("offset"):
        x += 1e4 if kind == "offset+1e4" else -1e4
    if kind == "neg-inf class":
        x.scatter_(2, torch.randint(0, c, (t, b, 1, h, w), generator=g), float("-inf"))
    if kind == "top-two equal":          # the two largest logits of every pass are bit-equal at classes lo < hi: p is too, the lower index wins
        lo = torch.randint(0, c - 1, (1, b, 1, h, w), generator=g).expand(t, b, 1, h, w)
        hi = lo + 1 + (torch.rand((1, b, 1, h, w), generator=g) * (c - 1 - lo[:1]).float()).long().clamp_max(c - 2 - lo[:1]).expand(t, b, 1, h, w)
        top = x.amax(2, keepdim=True) + 1.0
        x.scatter_(2, lo, top).scatter_(2, hi, top)
    if kind == "swap":
        # p_bar ties exactly where two passes hold the same column with classes 0 and 1 exchanged: (0 + e0) + e1 = (0 + e1) + e0, so
        # both passes have the same sum, and p0 + p1 is the same sum in either order
        x = torch.randn(1, b, c, h, w, generator=g)
        x[:, :, 0] = 5.0 + torch.rand(1, b, h, w, generator=g)
        x[:, :, 1] = 4.0 + torch.rand(1, b, h, w, generator=g)
        x = torch.cat([x, torch.cat([x[:, :, 1:2], x[:, :, 0:1], x[:, :, 2:]], 2)], 0)
    return x.float().contiguous()


def _mc_build(case: Case):
    return dict(logits=_logits(case))


def _mc_ref(case: Case, i, dt):
    p_bar, h_norm, mi, preds = ounc.mc_reduce(i["logits"].to(dt), MC_EPS)
    return dict(p_bar=p_bar, H_norm=h_norm, MI=mi, preds=preds)


def mc_decisions(case: Case, i, dt):
    c = case.p["c"]
    probs = F.log_softmax(i["logits"].to(dt), dim=2).exp()
    p_bar = probs.mean(0)
    eps = torch.tensor(MC_EPS, dtype=dt)
    return {"p < eps": (probs < eps).permute(0, 1, 3, 4, 2).reshape(-1, c), "p_bar < eps": (p_bar < eps).permute(0, 2, 3, 1).reshape(-1, c),
            "argmax": p_bar.argmax(1).reshape(-1), "tie of the top two": (p_bar.topk(2, dim=1).values.diff(dim=1) == 0).reshape(-1)}


def _single_build(case: Case):
    return dict(logits=_logits(case)[0].contiguous())


def _single_ref(case: Case, i, dt):
    probs, h_norm, preds = ounc.single_pass(i["logits"].to(dt), SINGLE_EPS)
    return dict(probs=probs, H_norm=h_norm, preds=preds)


def single_decisions(case: Case, i, dt):
    c = case.p["c"]
    probs = F.log_softmax(i["logits"].to(dt), dim=1).exp()
    return {"p < eps": (probs < torch.tensor(SINGLE_EPS, dtype=dt)).permute(0, 2, 3, 1).reshape(-1, c), "argmax": probs.argmax(1).reshape(-1),
            "tie of the top two": (probs.topk(2, dim=1).values.diff(dim=1) == 0).reshape(-1)}


# ---------------------------------------------------------------------------------------------------------------------
# bars and comparison
# ---------------------------------------------------------------------------------------------------------------------
def _loss_bars(case: Case):
    return dict(value=(VALUE_COEF, "value"), grad=(LOSSES[case.p["loss"]].grad_coef, "column"))


def _const(bars):
    return lambda c: bars


_MEASURES = dict(H=(1e-5, "abs"), H_norm=(1e-5, "abs"), AU=(3e-5, "abs"), EU=(3e-5, "abs"))
FAMILIES: Dict[str, Family] = {
    "loss": Family(_loss_cases(), _loss_build, _loss_ref, _loss_bars),
    "head": Family(_head_cases(), _head_build, _head_ref, _const(dict(alpha=(2e-6, "relative"), p_hat=(3e-6, "relative"), preds=(None, "exact"), **_MEASURES))),
    "alpha": Family(_alpha_cases(), _alpha_build, _alpha_ref, _const(_MEASURES)),
    "mc": Family(_mc_cases(), _mc_build, _mc_ref, _const(dict(p_bar=(1e-6, "abs"), H_norm=(1e-5, "abs"), MI=(1e-5, "abs"), preds=(None, "exact")))),
    "single": Family(_single_cases(), _single_build, _single_ref, _const(dict(probs=(1e-6, "abs"), H_norm=(1e-5, "abs"), preds=(None, "exact")))),
}
DECISIONS = dict(loss=loss_decisions, head=head_decisions, alpha=alpha_decisions, mc=mc_decisions, single=single_decisions)
ALL_CASES = [c for fam in FAMILIES.values() for c in fam.cases]
assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)


def evaluate(case: Case):
    """(inputs, fp64 results, fp32 results)"""
    fam = FAMILIES[case.family]
    inputs = fam.build(case)
    with torch.enable_grad():
        return inputs, fam.ref(case, inputs, torch.float64), fam.ref(case, inputs, torch.float32)


def bar_of(case: Case, key, spec, want64, want32):
    """(bar tensor shaped like the result, unit each difference is divided by) of one result that is not exact"""
    coef, mode = spec
    w64 = want64.double()
    unit = torch.ones_like(w64)
    if mode == "abs":
        bar = torch.full_like(w64, coef)
    elif mode == "relative":          # of each element: the differences are divided by |want|
        bar, unit = torch.full_like(w64, coef), w64.abs()
    elif mode == "value":
        bar = coef * w64.abs()
    elif mode == "column":          # of the largest |gradient| of the pixel's own class column
        bar = (coef * w64.abs().amax(1, keepdim=True)).expand_as(w64)
    else:
        raise ValueError(mode)
    if gap_bound(case, key):
        bar = bar.clamp_min(4.0 * float((want32.double() - w64).abs().max()))
    return bar, unit


def compare(tag, got, want64, want32, bar, unit, conditioned=True):
    """cmp of tests/pixel_edge_cases.py with a bar per element: prints device-fp64, fp32 oracle-fp64 and the bar at the element that
    comes closest to its bar, asserts the conditioning rule (unless the bar is gap-bound) and the bar; a bar of 0 asks for exactly 0"""
    w64 = want64.detach().double().cpu()
    unit = unit.clamp_min(1e-300)
    diff, gap = (got.detach().double().cpu() - w64).abs() / unit, (want32.detach().double().cpu() - w64).abs() / unit
    assert bool(torch.isfinite(diff).all()), f"{tag}: not finite"

    def worst(d):
        ratio = torch.where(bar > 0, d / bar.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d))).reshape(-1)
        k = int(ratio.argmax()) if ratio.numel() else 0
        return float(ratio[k]), float(d.reshape(-1)[k]), float(bar.reshape(-1)[k])

    (rd, d, b), (rg, gp, _) = worst(diff), worst(gap)
    print(f"{tag}: device-fp64 {d:.3e}, fp32 oracle-fp64 {gp:.3e}, bar {b:.3e}{'' if conditioned else ' (gap-bound)'}")
    if conditioned:
        assert rg <= 0.25, f"{tag}: the inputs are ill-conditioned for this bar (fp32 oracle is {gp:.3e} from fp64, {rg:.2f} of the bar)"
    assert rd <= 1.0, f"{tag}: {d:.3e} > {b:.3e}"


def check(case: Case, got: Dict[str, torch.Tensor], want64, want32):
    """Every result of `got` against the references.  A key ``name@variant`` of `got` is held to reference ``name``."""
    seen = set()
    for key, spec in FAMILIES[case.family].bars(case).items():
        for gkey, g in got.items():
            if gkey.split("@")[0] != key:
                continue
            seen.add(gkey)
            tag = f"{case.id} {gkey}"
            w64, w32 = want64[key], want32[key]
            g = g.detach().cpu()
            assert tuple(g.shape) == tuple(w64.shape), f"{tag}: shape {tuple(g.shape)}, expected {tuple(w64.shape)}"
            if spec[1] == "exact":
                same = torch.equal(g, w64)
                print(f"{tag}: exact {'ok' if same else 'DIFFERS'}")
                assert same, f"{tag}: differs from the reference in {int((g != w64).sum())} of {g.numel()} elements"
                continue
            bar, unit = bar_of(case, key, spec, w64, w32)
            compare(tag, g, w64, w32, bar, unit, conditioned=not gap_bound(case, key))
    assert seen == set(got), f"{case.id}: results without a bar: {sorted(set(got) - seen)}"


def conditioning(case: Case, want64, want32):
    """[(result, worst fp32 oracle - fp64 as a fraction of the coefficient's bar, that gap, the bar there, gap-bound)] of the results that
    are not exact; the exact ones must agree between the two dtypes"""
    out = []
    for key, spec in FAMILIES[case.family].bars(case).items():
        w64, w32 = want64[key], want32[key]
        assert bool(torch.isfinite(w64).all()) and bool(torch.isfinite(w32).all()), f"{case.id} {key}: reference not finite"
        if spec[1] == "exact":
            assert torch.equal(w32, w64), f"{case.id} {key}: exact result differs between the fp32 and the fp64 oracle"
            continue
        assert w64.dtype == torch.float64 and w32.dtype == torch.float32, f"{case.id} {key}: reference dtypes"
        coef, mode = spec
        gap = (w32.double() - w64).abs()
        scale = torch.ones_like(w64) if mode == "abs" else (w64.abs().amax(1, keepdim=True).expand_as(w64) if mode == "column" else w64.abs())
        frac = torch.where(scale > 0, gap / (coef * scale).clamp_min(1e-300), torch.where(gap > 0, torch.full_like(gap, float("inf")), torch.zeros_like(gap)))
        k = int(frac.reshape(-1).argmax())
        out.append((key, float(frac.reshape(-1)[k]), float(gap.max()), float((coef * scale).reshape(-1)[k]), gap_bound(case, key)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# branch census: (family, branch, outcome, which cases) -> every one of those cases has a counted pixel (or entry) with that outcome
# ---------------------------------------------------------------------------------------------------------------------
def _kinds(*kinds):
    return lambda p: LOSSES[p["loss"]].kind in kinds


def _in(regimes, pred=lambda p: True):
    return lambda p: p["regime"] in regimes and pred(p)


_HARD = lambda p: p["loss"] == "wrong_low_evidence_hard"          # noqa: E731
_GATED = lambda p: p["loss"] != "wrong_low_evidence_hard"         # noqa: E731  (the hard margin closes the gate at a gap of 0)
CENSUS = [
    # ComplementKLUniform: the three eps clamps and the switches that zero their gradient terms
    ("loss", "py_raw < eps", True, _kinds("ckl"), _in(["confident-wrong-tiny"])),
    ("loss", "py_raw < eps", False, _kinds("ckl"), _in(["typical", "confident-wrong", "clamped"])),
    ("loss", "den_raw < eps", True, _kinds("ckl"), _in(["saturated"])),
    ("loss", "den_raw < eps", False, _kinds("ckl"), _in(["typical", "confident-right"])),
    ("loss", "tl < eps", True, _kinds("ckl"), _in(["clamped", "clamped-tiny"])),
    ("loss", "tl < eps", False, _kinds("ckl"), _in(["typical", "clamped", "clamped-tiny", "saturated"])),
    # the two KL kinds: liveness, the sixth recurrence step, the host clamp of the weights' sum
    ("loss", "live", False, _kinds("kl", "klw"), _in(["clamped", "clamped-tiny"])),
    ("loss", "live", True, _kinds("kl", "klw"), _in(["typical", "clamped", "clamped-tiny"])),
    ("loss", "sixth step", True, _kinds("kl", "klw", "digamma"), _in(["sub-one", "clamped", "clamped-tiny", "mixed"], lambda p: p["regime"] in ("sub-one", "mixed") or
                                                                          LOSSES[p["loss"]].kind != "digamma")),
    ("loss", "sixth step", False, _kinds("kl", "klw", "digamma"), _in(["typical", "large-evidence"])),
    ("loss", "sum of weights < 1", True, _kinds("klw"), _in(["confident-right", "saturated", "saturated-hard"])),
    ("loss", "sum of weights < 1", False, _kinds("klw"), _in(["typical"])),
    # WrongLowEvidence
    ("loss", "a0 >= eps", False, _kinds("wle"), _in(["all-zero"])),
    ("loss", "a0 >= eps", True, _kinds("wle"), _in(["typical"])),
    ("loss", "pred", 0, _kinds("wle"), _in(["all-zero", "evidence-free"])),          # the pmax = -1 start, the tie of all classes
    ("loss", "pred != y", False, _kinds("wle"), _in(["confident-right", "tie-label-lower", "margin-sides"])),
    ("loss", "pred != y", True, _kinds("wle"), _in(["confident-wrong", "tie-label-higher", "margin-sides", "evidence-free"])),
    ("loss", "m > margin", True, _kinds("wle"), _in(["margin-sides", "confident-wrong"], _HARD)),
    ("loss", "m > margin", False, _kinds("wle"), _in(["margin-sides", "tie-label-higher"], _HARD)),
    ("loss", "h > 0", True, _kinds("wle"), _in(["confident-wrong", "margin-sides"])),
    ("loss", "gated with h == 0", True, _kinds("wle"), _in(["wrong-low-total", "evidence-free"], _GATED)),
    ("loss", "sum of gates < 1", True, _kinds("wle"), _in(["confident-right", "tie-label-lower"])),
    ("loss", "sum of gates == 0", True, _kinds("wle"), _in(["confident-right", "tie-label-lower"])),
    ("loss", "sum of gates == 0", True, _kinds("wle"), _in(["tie-label-higher"], _HARD)),
    ("loss", "sum of gates < 1", False, _kinds("wle"), _in(["confident-wrong"])),
    # head: both sides of the softplus switch, every step count of digamma_ge1, the tie of all classes
    ("head", "softplus argument > 20", True, None, None),
    ("head", "softplus argument > 20", False, None, None),
    ("head", "argmax", 0, None, lambda p: p["kind"] == "equal"),
] + [("alpha", "steps of alpha + 1", n, None, lambda p: p["kind"] == "mixed") for n in range(6)] + [
    ("alpha", "steps of alpha + 1", n, None, lambda p: p["kind"] == "steps") for n in (0, 1, 2, 3, 4)] + [
    ("alpha", "steps of alpha0 + 1", 0, None, None),
    # MC and single pass: a probability below eps (and exactly 0), none below, ties
    ("mc", "p < eps", True, None, lambda p: p["kind"] in ("spread40", "neg-inf class")),
    ("mc", "p_bar < eps", True, None, lambda p: p["kind"] in ("spread40", "neg-inf class") and p["t"] == 1),
    ("mc", "p < eps", False, None, None),
    ("mc", "tie of the top two", True, None, lambda p: p["kind"] in ("swap", "top-two equal", "equal")),
    ("mc", "tie of the top two", False, None, lambda p: p["kind"] == "randn3"),
    ("single", "p < eps", True, None, lambda p: p["kind"] in ("spread40", "neg-inf class")),
    ("single", "p < eps", False, None, None),
    ("single", "tie of the top two", True, None, lambda p: p["kind"] in ("top-two equal", "equal")),
]


def census_cases(entry):
    family, _, _, first, second = entry
    return [c for c in FAMILIES[family].cases if (first is None or first(c.p)) and (second is None or second(c.p))]
