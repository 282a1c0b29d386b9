"""The three class-column files that produce the uncertainty numbers (csrc/dirichlet_loss.hip, csrc/dirichlet.hip, csrc/uncertainty.hip),
driven through their public surfaces onto the branches that depend on the values of a pixel's class column, and compared with the fp64
references of tests/dirichlet_value_cases.py: the eps clamps of ComplementKLUniform and the switches that zero their gradient terms, the
liveness test of the KL kinds, a0 < eps and the pmax start of WrongLowEvidence, both sides of its soft and hard margin, a tie of the top
two classes with the label on either side, pred == y, a hinge of exactly 0 on a gated pixel, (1 - p_y)^gamma = 0, the host-side clamp of
a gate sum below 1, the sixth recurrence step of digamma_pos / trigamma_pos; every step count of digamma_ge1, the softplus switch at
exactly 20 and the all-equal column in the head; probabilities below eps, a -inf logit, T = 1, identical passes and an exact tie of
p_bar in the MC reduction and the single pass.

One test per case.  Bars: the project's coefficients (the cases module lists them), a loss value relative to |fp64 value| and a gradient
per pixel against the largest |fp64 gradient| of that pixel's class column; the gap-bound cases max(that, 4 x the fp32 oracle's own
distance from fp64); a bar of 0 asks for exactly 0, and so do the gradient entries that are 0 by construction.  Every comparison prints
device-fp64, fp32 oracle-fp64 and the bar.  tests/test_dirichlet_value_cases_cpu.py shows beforehand that the inputs are fair.  Not
covered: NaN inputs, a column of -inf only."""
import pytest
import torch

import dirichlet_value_cases as dv
from semanticlidarunc_amd import ops
from semanticlidarunc_amd.losses.regularizers import KL_offClasses_to_uniform
from semanticlidarunc_amd.models import probability_helper as ph
from test_gpu_dirichlet_losses import _modules

pytestmark = pytest.mark.gpu

MODULES = dict(_modules())
MODULES.update({f"kl_off_weighted_g{g}": KL_offClasses_to_uniform(ignore_index=0, with_conf_weighting=True, gamma=float(g)) for g in ("1", "2.5")})
assert set(MODULES) == set(dv.LOSSES)


def _run(cuda, case, fn):
    inputs, want64, want32 = dv.evaluate(case)
    got = fn(case, {k: v.to(cuda) for k, v in inputs.items()})
    torch.cuda.synchronize()
    dv.check(case, got, want64, want32)
    return inputs, got, want64


def _cases(family):
    return pytest.mark.parametrize("case", dv.FAMILIES[family].cases, ids=dv.case_id)


def _loss_and_grad(name, alpha, labels):
    a = alpha.detach().clone().requires_grad_(True)
    loss = MODULES[name](a, labels[:, None] if name == "mse" else labels)
    (g,) = torch.autograd.grad(loss, a)
    return loss.detach(), g


@_cases("loss")
def test_dirichlet_loss(cuda, case):
    def fn(c, d):
        value, grad = _loss_and_grad(c.p["loss"], d["alpha"], d["labels"])
        return dict(value=value, grad=grad)
    inputs, got, _ = _run(cuda, case, fn)
    mask = dv.zero_gradient_mask(case, inputs)
    nonzero = int((got["grad"].cpu()[mask] != 0).sum())
    print(f"{case.id}: {int(mask.sum())} gradient entries that are 0 by construction, {nonzero} of them not 0 on the device")
    assert nonzero == 0


@pytest.mark.parametrize("name", [n for n, l in dv.LOSSES.items() if l.ignore is not None])
def test_labels_out_of_range_count_like_the_ignore_value(cuda, name):
    """-1, C and 255 (the oracle's gather refuses them, so no tabled case carries them): the value and every gradient bit are those of the
    same input with the ignore value at these three pixels, and their gradient is 0"""
    case = next(c for c in dv.FAMILIES["loss"].cases if c.p == dict(loss=name, regime="typical", c=20, shape=dv.SHAPE))
    inputs = dv.FAMILIES["loss"].build(case)
    alpha, lab = inputs["alpha"].to(cuda), inputs["labels"]
    pos = torch.randperm(lab.numel(), generator=dv.gen(case))[:3]
    ignored, out = lab.clone(), lab.clone()
    ignored.reshape(-1)[pos] = dv.LOSSES[name].ignore
    out.reshape(-1)[pos] = torch.tensor([-1, 20, 255])
    (v0, g0), (v1, g1) = _loss_and_grad(name, alpha, ignored.to(cuda)), _loss_and_grad(name, alpha, out.to(cuda))
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    assert not g1.permute(0, 2, 3, 1).reshape(-1, 20)[pos.to(cuda)].any()


@_cases("head")
def test_dirichlet_head(cuda, case):
    def fn(c, d):
        n, t = c.p["c"], c.p["t"]
        alpha, p_hat, h_norm, preds = ph.dirichlet_head(d["outputs"], n, T=t, eps=dv.HEAD_EPS)
        alone = ph.to_alpha_concentrations_from_shape_and_scale(d["outputs"][:, :n], d["outputs"][:, n:n + 1], T=t, eps=dv.HEAD_EPS)
        assert torch.equal(alone, alpha), f"{c.id}: to_alpha_concentrations_from_shape_and_scale differs from the head's alpha"
        # the alpha-based measures of the device's alpha, as the reference calls them
        return {"alpha": alpha, "p_hat": p_hat, "H_norm": h_norm, "preds": preds, "H": ph.get_predictive_entropy(alpha, dv.HEAD_EPS),
                "H_norm@from alpha": ph.get_predictive_entropy_norm(alpha, dv.HEAD_EPS), "AU": ph.get_aleatoric_uncertainty(alpha, dv.HEAD_EPS),
                "EU": ph.get_epistemic_uncertainty(alpha, dv.HEAD_EPS)}
    _run(cuda, case, fn)


@_cases("alpha")
def test_dirichlet_measures_of_a_given_alpha(cuda, case):
    def fn(c, d):
        a = d["alpha"]
        return dict(H=ph.get_predictive_entropy(a, dv.HEAD_EPS), H_norm=ph.get_predictive_entropy_norm(a, dv.HEAD_EPS),
                    AU=ph.get_aleatoric_uncertainty(a, dv.HEAD_EPS), EU=ph.get_epistemic_uncertainty(a, dv.HEAD_EPS))
    _run(cuda, case, fn)


@_cases("mc")
def test_mc_reduce(cuda, case):
    def fn(c, d):
        p_bar, h_norm, mi, preds = ops.mc_reduce(d["logits"], dv.MC_EPS)
        return dict(p_bar=p_bar, H_norm=h_norm, MI=mi, preds=preds)
    _, got, _ = _run(cuda, case, fn)
    assert float(got["MI"].min()) >= 0.0          # identical passes: a cancellation residue that fmaxf(., 0) catches


@_cases("single")
def test_softmax_entropy(cuda, case):
    def fn(c, d):
        probs, h_norm, preds = ops.softmax_entropy(d["logits"], dv.SINGLE_EPS)
        return dict(probs=probs, H_norm=h_norm, preds=preds)
    _run(cuda, case, fn)
