"""GPU: the per-pixel loss and metric kernels at the class counts and pixel counts the other tests leave out.  Every one of them is
compiled twice, <20> and <32> class registers, dispatched on C <= 20; the other tests use C = 20 or 2 and pixel counts that are
multiples of 256.  Here: C in {3, 21, 32} (21 and 32 launch the <32> instantiations of nll_fwd / nll_bwd / softmax_loss_bwd /
softmax_nll / tversky_sums / tversky_bwd / dirichlet_loss fwd and bwd / ece / ece_samples / auroc_score) at 1 pixel, 258 pixels
(one block and 2) and 1305 = 5 * 256 + 25 pixels (a last wave of 25 lanes), where `if (pix >= npix) return` and the grid-stride
`continue` in front of the wave reductions have a partial wave to get wrong.  Labels carry the ignore value and, where the
reference accepts them, values outside [0, C) (-1, C, 255).

Reference: the oracle (or plain torch) on the same fp32 inputs converted to fp64.  Bars are the ones the project's tests of each
op already use (named at each test); before the device result is looked at, the fp32 oracle must be within a quarter of the bar
of the fp64 reference on the same inputs (`_cmp` asserts it), so that the bar measures the kernel and not the conditioning of
the inputs.  Each comparison prints its two figures."""
import math

import numpy as np
import pytest
import torch

from oracle import dirichlet as odir
from oracle import losses as olosses
from oracle import metrics as ometrics
from oracle import uncertainty as ounc
from semanticlidarunc_amd import ops
from semanticlidarunc_amd.loss import salsanext_loss
from semanticlidarunc_amd.losses.regularizers import KL_offClasses_to_uniform
from semanticlidarunc_amd.metrics.ece import ECEAggregator
from semanticlidarunc_amd.models.evaluator import IoUEvaluator
from semanticlidarunc_amd.models import probability_helper as ph
from semanticlidarunc_amd.models.losses import CrossEntropyLoss, TverskyLoss
from test_gpu_dirichlet_losses import _modules

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 3, 43), (3, 5, 87)]
CLASSES = [3, 21, 32]
_ids = lambda v: str(v).replace(" ", "")


def _gen(c, shape, salt=0):
    return torch.Generator().manual_seed(100000 * salt + 1000 * c + shape[1] * shape[2])


def _labels(shape, c, gen, ignore=None, out_of_range=False):
    """in-range labels; ~10 % at `ignore`; three each of -1, C and 255 where the shape has room; a single pixel gets a valid label"""
    b, h, w = shape
    lab = torch.randint(1 if ignore == 0 else 0, c, shape, generator=gen)
    n = b * h * w
    if n == 1:
        return lab
    if ignore is not None:
        lab[torch.rand(shape, generator=gen) < 0.1] = ignore
    if out_of_range:
        pos = torch.randperm(n, generator=gen)[:9]
        lab.reshape(-1)[pos] = torch.tensor([-1, c, 255] * 3)
    return lab


def _cmp(tag, got, want64, want32, bar):
    """got: device result; want64 / want32: the reference in fp64 and the oracle in fp32 on the same inputs (None: not asked)"""
    want64 = torch.as_tensor(want64).detach().double().cpu()
    gap = None if want32 is None else float((torch.as_tensor(want32).detach().double().cpu() - want64).abs().max())
    diff = float((torch.as_tensor(got).detach().double().cpu() - want64).abs().max())
    print(f"{tag}: device-fp64 {diff:.3e}, fp32 oracle-fp64 {'n/a' if gap is None else format(gap, '.3e')}, bar {bar:.3e}")
    if gap is not None:
        assert gap <= bar / 4, f"{tag}: the inputs are ill-conditioned for this bar (fp32 oracle is {gap:.3e} from fp64, bar {bar:.3e})"
    assert diff <= bar, f"{tag}: {diff:.3e} > {bar:.3e}"


def _both(fn, x, *args):
    """fn(x, *args) -> loss, differentiated, once in fp64 and once in fp32: [(loss, grad)] * 2"""
    out = []
    for dt in (torch.float64, torch.float32):
        xc = x.detach().clone().to(dt).requires_grad_(True)
        loss = fn(xc, *args)
        (loss if loss.dim() == 0 else loss.sum()).backward()
        out.append((loss.detach(), xc.grad))
    return out


# ---- CrossEntropyLoss: nll_fwd_kernel / nll_bwd_kernel, three kinds -----------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("c", CLASSES)
def test_cross_entropy(cuda, c, shape):
    """Value 1e-5 (test_gpu_loss).  Gradient 1e-5 of its scale, the bar of that test's probs / log_probs branches; its logits
    branch uses 1e-7 absolute at a scale of 1/900, i.e. 9e-5 of the scale, so this is the tighter of the two at every shape."""
    gen = _gen(c, shape, 1)
    logits = torch.randn(shape[0], c, shape[1], shape[2], generator=gen) * 2.0
    lab = _labels(shape, c, gen, ignore=0, out_of_range=True)
    for act, x in (("logits", logits), ("probs", logits.softmax(1)), ("log_probs", logits.log_softmax(1))):
        (l64, g64), (l32, g32) = _both(lambda t: olosses.cross_entropy(t, lab, 0, act), x)
        xd = x.to(cuda).requires_grad_(True)
        got = CrossEntropyLoss(0)(xd, lab.to(cuda), c, act)
        got.backward()
        _cmp(f"ce {act} C={c} {shape} value", got, l64, l32, 1e-5)
        _cmp(f"ce {act} C={c} {shape} grad", xd.grad, g64, g32, 1e-5 * float(g64.abs().max()))


@pytest.mark.parametrize("c", CLASSES)
def test_cross_entropy_all_ignored(cuda, c):
    """No counted pixel (every label the ignore value or out of range): the mean over nothing is NaN in the reference and here,
    and no gradient reaches the input."""
    shape = (2, 3, 43)
    gen = _gen(c, shape, 2)
    logits = torch.randn(shape[0], c, shape[1], shape[2], generator=gen)
    lab = torch.zeros(shape, dtype=torch.int64)
    lab.reshape(-1)[:3] = torch.tensor([-1, c, 255])
    for act, x in (("logits", logits), ("probs", logits.softmax(1)), ("log_probs", logits.log_softmax(1))):
        assert math.isnan(float(olosses.cross_entropy(x.double(), lab, 0, act)))
        xd = x.to(cuda).requires_grad_(True)
        got = CrossEntropyLoss(0)(xd, lab.to(cuda), c, act)
        assert math.isnan(float(got.detach()))
        got.backward()
        assert not xd.grad.cpu().any()


# ---- salsanext_loss: softmax_nll_kernel, the Lovasz kernels, softmax_loss_bwd_kernel --------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("c", CLASSES)
def test_salsanext_loss(cuda, c, shape):
    """Bars of test_gpu_loss: nll and lovasz 1e-5, total 2e-5, gradient 1e-6 absolute, softmax 1e-6."""
    gen = _gen(c, shape, 3)
    logits = torch.randn(shape[0], c, shape[1], shape[2], generator=gen)      # unit scale: at twice that the CPU's own fp32 softmax is 3.2e-7 off
    lab = _labels(shape, c, gen)
    ref = []
    for dt in (torch.float64, torch.float32):
        z = logits.clone().to(dt).requires_grad_(True)
        tot, nll, ls = olosses.salsanext_loss(z, lab)
        tot.backward()
        ref.append((tot.detach(), nll.detach(), ls.detach(), z.grad))
    zd = logits.to(cuda).requires_grad_(True)
    total, nll, ls = salsanext_loss(zd, lab.to(cuda), 1.0, 1.0, 0)
    total.backward()
    tag = f"salsanext C={c} {shape}"
    _cmp(tag + " nll", nll, ref[0][1], ref[1][1], 1e-5)
    _cmp(tag + " lovasz", ls, ref[0][2], ref[1][2], 1e-5)
    _cmp(tag + " total", total, ref[0][0], ref[1][0], 2e-5)
    _cmp(tag + " grad", zd.grad, ref[0][3], ref[1][3], 1e-6)
    probs, acc = ops.softmax_nll(logits.to(cuda), lab.to(cuda))
    _cmp(tag + " softmax", probs, logits.double().softmax(1), logits.softmax(1), 1e-6)
    _cmp(tag + " nll sum / n", acc / lab.numel(), ref[0][1], ref[1][1], 1e-5)


def test_salsanext_terms_are_not_differentiable(cuda):
    """The backward of SalsaNextLossFn is that of `total`; its nll and lovasz outputs are values for logging.  Differentiating
    through one of them raises (it used to return zeros silently) and the gradient of `total` is what it was."""
    shape, c = (2, 3, 43), 21
    gen = _gen(c, shape, 4)
    logits = torch.randn(shape[0], c, shape[1], shape[2], generator=gen) * 2.0
    lab = _labels(shape, c, gen)
    zd = logits.to(cuda).requires_grad_(True)
    total, nll, ls = salsanext_loss(zd, lab.to(cuda), 0.5, 2.0, 0)
    assert total.requires_grad and not nll.requires_grad and not ls.requires_grad
    for term in (nll, ls):
        with pytest.raises(RuntimeError):
            torch.autograd.grad(term, zd, retain_graph=True)
    (g,) = torch.autograd.grad(total + 3.0 * nll.detach(), zd)
    z = logits.double().requires_grad_(True)
    olosses.salsanext_loss(z, lab, 0.5, 2.0)[0].backward()
    z32 = logits.clone().requires_grad_(True)
    olosses.salsanext_loss(z32, lab, 0.5, 2.0)[0].backward()
    _cmp("salsanext weighted grad", g, z.grad, z32.grad, 2e-6)           # 1e-6 per unit of weight on the Lovasz term (w_ls = 2)


# ---- TverskyLoss: tversky_sums_kernel / tversky_bwd_kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("c", CLASSES)
def test_tversky(cuda, c, shape):
    """Bars of test_gpu_tversky: loss 1e-5 relative, gradient 1e-5 of its scale (+ 1e-9)."""
    gen = _gen(c, shape, 5)
    logits = torch.randn(shape[0], c, shape[1], shape[2], generator=gen)
    lab = _labels(shape, c, gen, ignore=255, out_of_range=True)
    wgt = torch.linspace(0.5, 1.5, c)
    for act, x in (("logits", logits), ("probs", logits.softmax(1)), ("log_probs", logits.log_softmax(1))):
        for red in ("mean", "sum", "none"):
            def ref(t):
                loss = olosses.tversky(t, lab, c, act, 0.7, 0.3, 1.0, 255, red)
                return loss, ((loss * wgt.to(t.dtype)).sum() if red == "none" else loss)
            r = []
            for dt in (torch.float64, torch.float32):
                xc = x.clone().to(dt).requires_grad_(True)
                loss, scalar = ref(xc)
                scalar.backward()
                r.append((loss.detach(), xc.grad))
            xd = x.to(cuda).requires_grad_(True)
            got = TverskyLoss(alpha=0.7, beta=0.3, smooth=1.0, ignore_index=255, reduction=red)(xd, lab.to(cuda), c, act)
            ((got * wgt.to(cuda)).sum() if red == "none" else got).backward()
            tag = f"tversky {act}|{red} C={c} {shape}"
            _cmp(tag + " value", got, r[0][0], r[1][0], 1e-5 * max(1.0, float(r[0][0].abs().max())))
            _cmp(tag + " grad", xd.grad, r[0][1], r[1][1], 1e-5 * float(r[0][1].abs().max()) + 1e-9)


# ---- Dirichlet losses: dirichlet_loss_kernel forward and backward ----------------------------------------------------------------------
def _dirichlet_oracles(lab):
    return {"nll_dircat": lambda a: odir.loss_nll_dircat(a, lab, 0), "digamma_ce": lambda a: odir.loss_digamma_ce(a, lab, 0),
            "brier": lambda a: odir.loss_brier(a, lab, 0), "brier_sref40": lambda a: odir.loss_brier(a, lab, 0, 40.0),
            "mse": lambda a: odir.loss_mse(a, lab, 0), "kl_off_uniform": lambda a: odir.loss_kl_off_uniform(a, lab, 0),
            "complement_kl": lambda a: odir.loss_complement_kl(a, lab, 0, 1.25, 0.65, 0.15),
            "complement_kl_gated": lambda a: odir.loss_complement_kl(a, lab, 0, s_target=30.0, normalize=False, detach_uncert=False),
            "wrong_low_evidence": lambda a: odir.loss_wrong_low_evidence(a, lab, 0),
            "wrong_low_evidence_hard": lambda a: odir.loss_wrong_low_evidence(a, lab, 0, 4.0, 0.1, 0.0),
            "wrong_low_evidence_nomargin": lambda a: odir.loss_wrong_low_evidence(a, lab, None, margin=0.0)}


def _alpha(shape, c, gen):
    return 1.0 + torch.nn.functional.softplus(torch.randn(shape[0], c, shape[1], shape[2], generator=gen) * 2.0) * 10.0


def _check_dirichlet(cuda, name, mod, oracle, alpha, lab, tag, grad_bar=2e-5):
    (l64, g64), (l32, g32) = _both(oracle, alpha)
    a = alpha.to(cuda).requires_grad_(True)
    loss = mod(a, lab.to(cuda)[:, None] if name == "mse" else lab.to(cuda))
    loss.backward()
    _cmp(f"dirichlet {name} {tag} value", loss, l64, l32, 1e-5 * max(1.0, abs(float(l64))))
    _cmp(f"dirichlet {name} {tag} grad", a.grad, g64, g32, grad_bar * float(g64.abs().max()) + 1e-9)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("c", [21, 32])
def test_dirichlet_losses(cuda, c, shape):
    """Bars of test_gpu_dirichlet_losses: value 1e-5 relative (1e-5 absolute below 1), gradient 2e-5 of its scale; the
    confidence-weighted KL 3e-5 of its gradient scale, as there."""
    gen = _gen(c, shape, 6)
    lab = _labels(shape, c, gen, ignore=0)
    alpha = _alpha(shape, c, gen)
    oracles = _dirichlet_oracles(lab)
    for name, mod in _modules().items():
        _check_dirichlet(cuda, name, mod, oracles[name], alpha, lab, f"C={c} {shape}")
    for gamma in (1.0, 2.5):
        _check_dirichlet(cuda, f"kl_off_weighted gamma={gamma}", KL_offClasses_to_uniform(ignore_index=0, with_conf_weighting=True, gamma=gamma),
                         lambda a: odir.loss_kl_off_uniform(a, lab, 0, with_conf_weighting=True, gamma=gamma), alpha, lab, f"C={c} {shape}", 3e-5)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dirichlet_two_and_three_classes(cuda, shape):
    """DirichletMSELoss and ComplementKLUniform return 0 for C <= 2 (there is no off-class distribution to speak of); C = 3 is the
    first class count that runs their kernels."""
    mods = {k: v for k, v in _modules().items() if k in ("mse", "complement_kl", "complement_kl_gated")}
    gen = _gen(2, shape, 7)
    lab = _labels(shape, 2, gen, ignore=0)
    for name, mod in mods.items():
        a = _alpha(shape, 2, gen).to(cuda).requires_grad_(True)
        loss = mod(a, lab.to(cuda)[:, None] if name == "mse" else lab.to(cuda))
        assert float(loss.detach()) == 0.0
        if loss.requires_grad:
            loss.backward()
            assert not a.grad.cpu().any()
    gen = _gen(3, shape, 7)
    lab = _labels(shape, 3, gen, ignore=0)
    alpha = _alpha(shape, 3, gen)
    oracles = _dirichlet_oracles(lab)
    for name, mod in mods.items():
        _check_dirichlet(cuda, name, mod, oracles[name], alpha, lab, f"C=3 {shape}")


# ---- ECE: ece_kernel (bin form) and ece_samples_kernel -----------------------------------------------------------------------------------
def _probs_by_mode(x, mode, eps=1e-12):
    if mode == "logits":
        return x.softmax(1)
    if mode == "alpha":
        return x / (x.sum(1, keepdim=True) + eps)
    p = x.clamp_min(0)
    return p / p.sum(1, keepdim=True).clamp_min(eps)


def _mode_inputs(shape, c, gen):
    logits = torch.randn(shape[0], c, shape[1], shape[2], generator=gen) * 3.0
    return {"logits": logits, "alpha": torch.nn.functional.softplus(logits) + 1.0, "probs": logits.softmax(1)}


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("c", CLASSES)
def test_ece_bins(cuda, c, shape):
    """The bin form of ECEAggregator (test_gpu_uncertainty): bin counts exact, ECE and MCE 1e-5.  The counts are integers, so their
    reference is the oracle's fp32 top-label confidence, which rounds the class sum as the reference project does.  ECE and MCE are
    compared with the same bins summed in fp64; the oracle's own two figures are not asked to be near them, because it sums its
    float32 weights with a float32 cumsum (up to 1.7e-5 off at 1305 samples), which is what the 1e-5 of the existing test allows
    for, and the device sums in fp64."""
    gen = _gen(c, shape, 8)
    inputs = _mode_inputs(shape, c, gen)
    lab = _labels(shape, c, gen, ignore=0, out_of_range=True)
    edges = np.linspace(0.0, 1.0, 16, dtype=np.float32)
    edges[0], edges[-1] = 0.0, 1.0
    for mode in ("probs", "alpha"):
        agg = ECEAggregator(n_bins=15, mode=mode, ignore_index=0)
        agg.update(inputs[mode].to(cuda), lab.to(cuda))
        (e, m), stats, _ = agg.compute()
        conf, ok = ometrics.top_label(inputs[mode].numpy(), lab.numpy(), 0, mode)
        n = ometrics.ece_bins(conf, ok, 15)[0]
        assert np.array_equal(stats["n"].to_numpy(), n), (mode, stats["n"].to_numpy(), n)
        acc64 = np.histogram(conf, bins=edges, weights=ok.astype(np.float64))[0]
        conf64 = np.histogram(conf, bins=edges, weights=conf.astype(np.float64))[0]
        e64, m64 = ometrics.ece_from_bins(n, acc64, conf64)
        _cmp(f"ece bins {mode} C={c} {shape} ece", e, e64, None, 1e-5)
        _cmp(f"ece bins {mode} C={c} {shape} mce", m, m64, None, 1e-5)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("c", CLASSES)
def test_ece_samples(cuda, c, shape):
    """Confidence 2e-6: it is 1 - (the '1-maxprob' AUROC score), the same normalised maximum, and that is the bar test_gpu_auroc
    sets for it; the flags are exact (the fp32 oracle's own flags must equal the fp64 ones, i.e. no near-tie of the top two)."""
    gen = _gen(c, shape, 9)
    inputs = _mode_inputs(shape, c, gen)
    lab = _labels(shape, c, gen, ignore=0, out_of_range=True)
    for mode, x in inputs.items():
        conf, flag = ops.ece_samples(x.to(cuda), lab.to(cuda), mode, ignore_index=0)
        r = []
        for dt in (torch.float64, torch.float32):
            cf, pred = _probs_by_mode(x.to(dt), mode).max(1)
            r.append((cf.clamp(0, 1), torch.where(lab == 0, torch.full_like(lab, 2), (pred == lab).long())))
        assert torch.equal(r[0][1], r[1][1])
        assert torch.equal(flag.cpu().long(), r[0][1]), mode
        _cmp(f"ece samples {mode} C={c} {shape} conf", conf, r[0][0], r[1][0], 2e-6)


# ---- AUROC scores: auroc_score_kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("c", CLASSES)
def test_auroc_scores(cuda, c, shape):
    """Bars of test_gpu_auroc: score 2e-6, 3e-5 for mi_norm; flags exact (the fp32 oracle's must equal the fp64 ones)."""
    gen = _gen(c, shape, 10)
    inputs = _mode_inputs(shape, c, gen)
    lab = _labels(shape, c, gen, ignore=0, out_of_range=True)
    for mode, score in (("logits", "entropy_norm"), ("alpha", "mi_norm"), ("probs", "1-maxprob")):
        s, f = ops.auroc_scores(inputs[mode].to(cuda), lab.to(cuda), mode, score, ignore_index=0)
        s64, e64 = ometrics.auroc_samples(inputs[mode].double(), lab, mode, score, 0)
        s32, e32 = ometrics.auroc_samples(inputs[mode], lab, mode, score, 0)
        valid = lab != 0
        assert torch.equal((f != 2).cpu(), valid)
        assert np.array_equal(e64, e32)
        assert np.array_equal(f.cpu()[valid].numpy(), e64), (mode, score)
        _cmp(f"auroc {mode}|{score} C={c} {shape} score", s.cpu()[valid], s64, s32, 3e-5 if score == "mi_norm" else 2e-6)


# ---- confusion matrix --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("c", CLASSES)
def test_confusion_matrix(cuda, c, shape):
    """Exact; predictions and labels outside [0, C) are dropped, over two updates."""
    gen = _gen(c, shape, 11)
    ev = IoUEvaluator(c)
    want = np.zeros((c, c), dtype=np.int64)
    for _ in range(2):
        p = torch.randint(-1, c + 2, shape, generator=gen)
        t = torch.randint(-1, c + 2, shape, generator=gen)
        p[torch.rand(shape, generator=gen) < 0.05] = 255
        t[torch.rand(shape, generator=gen) < 0.05] = 255
        ev.update(p.to(cuda), t.to(cuda))
        want += ometrics.confusion_matrix(p.numpy(), t.numpy(), c)
    assert np.array_equal(ev.confmat.cpu().numpy(), want)


# ---- single-pass softmax / entropy map: softmax_entropy_kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("c", CLASSES)
def test_softmax_entropy(cuda, c, shape):
    """Bars of test_gpu_uncertainty's test_single_pass_golden: probs 1e-6, H 1e-5, argmax exact (the fp32 oracle's must equal the
    fp64 one).  Unit-scale logits: at twice that the fp32 oracle's own probabilities are 3.0e-7 from fp64, over a quarter of the bar."""
    gen = _gen(c, shape, 12)
    logits = torch.randn(shape[0], c, shape[1], shape[2], generator=gen)
    p64, h64, a64 = ounc.single_pass(logits.double())
    p32, h32, a32 = ounc.single_pass(logits)
    probs, h, preds = ops.softmax_entropy(logits.to(cuda))
    assert torch.equal(a64, a32)
    assert torch.equal(preds.cpu(), a64)
    _cmp(f"softmax_entropy C={c} {shape} probs", probs, p64, p32, 1e-6)
    _cmp(f"softmax_entropy C={c} {shape} H", h, h64, h32, 1e-5)


# ---- Dirichlet head and alpha-based measures: dirichlet_kernel<., true> and <., false> -----------------------------------------------------
def _rel(t, want64):
    return torch.as_tensor(t).detach().double().cpu() / want64


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("c", CLASSES)
def test_dirichlet_head(cuda, c, shape):
    """Bars of test_gpu_dirichlet: alpha 2e-6 and p_hat 3e-6 relative, H_norm 1e-5, AU and EU 3e-5, argmax exact (the fp32 oracle's
    must equal the fp64 one).  The scale logit is centred at 3 so that no pixel is evidence-free (alpha = 1 + eps in every class ties
    the argmax); three pixels carry 25, past the softplus threshold of 20, where the shape has room."""
    gen = _gen(c, shape, 13)
    outs = torch.randn(shape[0], c + 1, shape[1], shape[2], generator=gen) * 2.0
    outs[:, c] = torch.randn(shape, generator=gen) * 3.0 + 3.0
    if outs[:, c].numel() > 1:
        pos = torch.randperm(outs[:, c].numel(), generator=gen)[:3]
        scale = outs[:, c].reshape(-1)
        scale[pos] = 25.0
        outs[:, c] = scale.reshape(shape)
    a64, p64, hn64, pr64 = odir.head(outs.double(), c)
    a32, p32, hn32, pr32 = odir.head(outs, c)
    assert torch.equal(pr64, pr32)
    tag = f"dirichlet head C={c} {shape}"
    alpha, p_hat, h_norm, preds = ph.dirichlet_head(outs.to(cuda), c)
    assert torch.equal(preds.cpu(), pr64)
    one = torch.ones_like(a64)
    _cmp(tag + " alpha (relative)", _rel(alpha, a64), one, _rel(a32, a64), 2e-6)
    _cmp(tag + " p_hat (relative)", _rel(p_hat, p64), one, _rel(p32, p64), 3e-6)
    _cmp(tag + " H_norm", h_norm, hn64, hn32, 1e-5)
    # dirichlet_uncertainty: the alpha-based measures of the device's alpha, as the reference calls them
    _cmp(tag + " H_norm from alpha", ph.get_predictive_entropy_norm(alpha), hn64, hn32, 1e-5)
    _cmp(tag + " AU", ph.get_aleatoric_uncertainty(alpha), odir.aleatoric(a64), odir.aleatoric(a32), 3e-5)
    _cmp(tag + " EU", ph.get_epistemic_uncertainty(alpha), odir.epistemic(a64), odir.epistemic(a32), 3e-5)
