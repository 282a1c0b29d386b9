"""CPU: the oracle reproduces every committed golden vector (which tools/gen_golden.py produced by
running the reference itself) and a few hand-derived known answers."""
import json
import math
import os

import numpy as np
import torch

from conftest import GOLDEN, golden
from oracle import losses as olosses, metrics as ometrics, salsanext as osalsa, uncertainty as ounc
from semanticlidarunc_amd.salsanext import SalsaNext
from semanticlidarunc_amd.testing import seeded_model


def _t(a):
    return torch.from_numpy(np.asarray(a))


# The goldens hold the reference's float32 results computed on one host.  Their last bits depend on the CPU that computed them: which
# vectorised transcendental kernels, MKL / oneDNN code paths and thread partitions torch picks there.  On another x86 host the same
# operations land a few float32 roundings away (at most 6 measured), so the oracle is held to the golden within F32_ULPS roundings.
F32_EPS = float(np.finfo(np.float32).eps)
F32_ULPS = 8
AUROC_PAIRS = 8


def _max_ulps(got, want):
    """max over elements of |got - want| in float32 roundings of max(1, |want|)."""
    got = np.asarray(got.detach() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (F32_EPS * np.maximum(1.0, np.abs(want)))).max())


def _max_ulps_of_scale(got, want):
    """max |got - want| in float32 roundings of max |want|: for gradients, whose elements are sums of terms that cancel -- a rounding of a
    term is measured against the gradient's scale, not against the small element it cancels down to."""
    got = np.asarray(got.detach() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / (F32_EPS * max(float(np.abs(want).max()), np.finfo(np.float32).tiny)))


def _sd():
    return seeded_model(SalsaNext).state_dict()


def test_seeded_weights_match_reference_digest():
    g = golden("salsanext_eval_1x5x16x64")
    sd = _sd()
    s = sum(float(v.double().sum()) for v in sd.values())
    a = sum(float(v.double().abs().sum()) for v in sd.values())
    assert np.allclose([s, a], g["sd_digest"], rtol=1e-12)


def test_salsanext_eval_matches_reference_logits():
    g = golden("salsanext_eval_1x5x16x64")
    with torch.no_grad():
        y = osalsa.salsanext_forward(_sd(), _t(g["x"]))
    assert float((y - _t(g["logits"])).abs().max()) <= 1e-5


def test_salsanext_dropout_multipliers_match_reference_logits():
    g = golden("salsanext_mc_2x5x32x64")
    scales = {k[len("scale:"):]: _t(g[k])[:, :, None, None] for k in g.files if k.startswith("scale:")}
    assert set(scales) == {n for n, _ in osalsa.DROPOUT_SITES}
    with torch.no_grad():
        y = osalsa.salsanext_forward(_sd(), _t(g["x"]), scales)
    assert float((y - _t(g["logits"])).abs().max()) <= 1e-5


def test_mc_reduce_golden_and_known_answers():
    g = golden("mc_reduce_T4_1x20x4x64")
    p_bar, h, mi, preds = ounc.mc_reduce(_t(g["logits"]))
    assert float((p_bar - _t(g["p_bar"])).abs().max()) <= 1e-7
    assert float((h - _t(g["h_norm"])).abs().max()) <= 1e-6
    assert float((mi - _t(g["mi_norm"])).abs().max()) <= 1e-6
    assert torch.equal(preds, _t(g["preds"]))
    # identical passes: MI = 0, uniform logits: H_norm = 1
    z = torch.zeros(3, 1, 20, 2, 4)
    p_bar, h, mi, _ = ounc.mc_reduce(z)
    assert torch.allclose(p_bar, torch.full_like(p_bar, 0.05)) and torch.allclose(h, torch.ones_like(h), atol=1e-6)
    assert float(mi.abs().max()) <= 1e-6
    # two passes, two classes, opposite certain predictions: p_bar = (.5,.5): H = ln2/ln2 = 1, E[H_t] ~ 0 -> MI ~ 1
    lg = torch.tensor([[30.0, -30.0], [-30.0, 30.0]]).reshape(2, 1, 2, 1, 1)
    _, h, mi, _ = ounc.mc_reduce(lg)
    assert abs(float(h) - 1.0) < 1e-6 and abs(float(mi) - 1.0) < 1e-5


def test_single_pass_golden():
    g = golden("single_pass_1x20x4x64")
    probs, h, preds = ounc.single_pass(_t(g["logits"]))
    assert float((probs - _t(g["probs"])).abs().max()) <= 1e-7
    assert float((h - _t(g["h_norm"])).abs().max()) <= 1e-6
    assert torch.equal(preds, _t(g["preds"]))


def test_loss_golden_and_hand_derived():
    g = golden("loss_2x20x8x64")
    lg = _t(g["logits"]).clone().requires_grad_(True)
    lab = _t(g["labels"])
    tot, nll, ls = olosses.salsanext_loss(lg, lab)
    assert abs(float(nll) - float(g["nll"])) <= 1e-6
    assert abs(float(ls) - float(g["lovasz"])) <= 1e-6
    tot.backward()
    assert float((lg.grad - _t(g["grad_logits"])).abs().max()) <= 1e-6
    pr = torch.softmax(lg.detach(), 1)
    assert abs(float(olosses.lovasz_softmax(pr, lab, None)) - float(g["lovasz_noignore"])) <= 1e-6
    assert abs(float(olosses.cross_entropy(lg.detach(), lab, 0, "logits")) - float(g["ce_ignore0"])) <= 1e-6
    # 4 pixels / 2 classes, derived by hand: class 0 -> 0.8/3 + 0.7/3 + 0.4/12 + 0.1/4, class 1 -> 0.65
    k = golden("kat_4px_2cls")
    hand = 0.5 * ((0.8 / 3 + 0.7 / 3 + 0.4 / 12 + 0.1 / 4) + (0.8 * 0.5 + 0.7 / 6 + 0.4 / 3))
    assert abs(float(k["lovasz_none"]) - hand) < 1e-6
    assert abs(float(olosses.lovasz_softmax(_t(k["probs"]), _t(k["labels"]), None)) - hand) < 1e-6
    assert abs(float(olosses.lovasz_softmax(_t(k["probs"]), _t(k["labels"]), 0)) - float(k["lovasz_ign0"])) < 1e-6
    hand_nll = -(math.log(0.9) + math.log(0.6) + math.log(0.3) + math.log(0.2)) / 4
    assert abs(float(k["nll"]) - hand_nll) < 1e-6
    assert abs(float(olosses.nll_on_probs(_t(k["probs"]), _t(k["labels"]))) - hand_nll) < 1e-6
    # empty / all-ignored input
    assert float(olosses.lovasz_softmax(_t(k["probs"]), torch.zeros(1, 1, 4, dtype=torch.long), 0)) == 0.0
    # classes='all' / a list of ids (lovasz.py:66-69), from the reference's own class (tools/gen_golden_r03.py lovasz_classes)
    gc = golden("lovasz_classes_2x20x8x64")
    for tag, ign, classes in (("all_ign0", 0, "all"), ("all_none", None, "all"), ("list_ign0", 0, [1, 3, 19]), ("present_ign0", 0, "present")):
        p = torch.softmax(_t(gc["logits"]), 1).requires_grad_(True)
        loss = olosses.lovasz_softmax(p, _t(gc["labels"]), ign, classes)
        assert abs(float(loss) - float(gc["loss_" + tag])) <= 1e-6
        loss.backward()
        assert float((p.grad - _t(gc["grad_" + tag])).abs().max()) <= 1e-6


def test_iou_golden():
    g = golden("iou_2x16x64")
    cm = ometrics.confusion_matrix(g["preds"], g["labels"], 20)
    assert np.array_equal(cm, g["confmat"])
    miou, iou = ometrics.iou_from_confusion(cm, [0] + [1] * 19, [0])
    assert abs(miou - float(g["miou"])) < 1e-12
    assert np.allclose(iou, g["iou"], equal_nan=True)
    # out-of-range pairs are dropped
    cm2 = ometrics.confusion_matrix(np.array([0, 25, 3, -1]), np.array([0, 1, 99, 2]), 20)
    assert cm2.sum() == 1 and cm2[0, 0] == 1


def test_ece_golden():
    g = golden("ece_2x20x16x64")
    conf, corr = ometrics.top_label(g["probs"], g["labels"], ignore_index=0)
    n, acc_s, conf_s = ometrics.ece_bins(conf, corr, 15)
    assert np.array_equal(n, g["n"])
    e, m = ometrics.ece_from_bins(n, acc_s, conf_s)
    assert abs(e - float(g["ece"])) < 1e-7 and abs(m - float(g["mce"])) < 1e-7
    # confidence exactly 1.0 lands in the last (closed) bin; 0.2 = edge of bin 3 goes up
    n, _, _ = ometrics.ece_bins(np.array([1.0, np.float32(0.2), 0.0], np.float32), np.array([1, 0, 1]), 15)
    assert n[14] == 1 and n[0] == 1 and n.sum() == 3


def test_fixture_files_present():
    with open(os.path.join(GOLDEN, "salsanext_state_dict_keys.json")) as f:
        assert len(json.load(f)) == 51 * 2 + 42 * 5


def test_dirichlet_head_matches_reference_golden():
    """oracle.dirichlet against the vectors tools/gen_golden.py took from the reference's probability_helper."""
    from oracle import dirichlet as odir
    g = golden("dirichlet_head_2x21x8x64")
    outs = torch.from_numpy(g["outputs"])
    alpha, p_hat, h_norm, preds = odir.head(outs, 20)
    assert _max_ulps(alpha, g["alpha"]) <= F32_ULPS
    assert _max_ulps(p_hat, g["p_hat"]) <= F32_ULPS
    assert _max_ulps(h_norm, g["H_norm"]) <= F32_ULPS
    assert torch.equal(preds, torch.from_numpy(g["preds"]))
    assert _max_ulps(odir.aleatoric(alpha), g["AU"]) <= F32_ULPS
    assert _max_ulps(odir.epistemic(alpha), g["EU"]) <= F32_ULPS
    a2 = odir.alpha_from_shape_and_scale(outs[:, :20], outs[:, 20:21], 2.5, 1e-6)
    assert _max_ulps(a2, g["alpha_T2p5_eps1em6"]) <= F32_ULPS
    # known answers: zero evidence (scale -> -inf) gives alpha = 1 + eps, the uniform p_hat and H_norm = 1
    flat = torch.zeros(1, 21, 2, 2)
    flat[:, 20] = -100.0
    a, p, hn, _ = odir.head(flat, 20)
    assert float((a - (1.0 + 1e-8)).abs().max()) < 1e-7 and float((p - 0.05).abs().max()) < 1e-7 and float((hn - 1.0).abs().max()) < 1e-6


def test_auroc_golden_and_known_answers():
    """oracle.metrics.auroc_* against the values tools/gen_golden.py took from the reference's AUROCAggregator."""
    g = golden("auroc_2x20x16x64")
    labs = torch.from_numpy(g["labels"])
    inputs = {"logits": torch.from_numpy(g["logits"]), "alpha": torch.from_numpy(g["alpha"]), "probs": torch.from_numpy(g["logits"]).softmax(1)}
    for key in g.files:
        if not key.startswith("auroc:") or key == "auroc:capped1500":
            continue
        mode, score, src = key[len("auroc:"):].split("|")
        ov = torch.from_numpy(g["override"]) if src == "override" else None
        s1, e1 = ometrics.auroc_samples(inputs[mode], labs, mode, score, 0, 1e-12, ov)
        s2, e2 = ometrics.auroc_samples(inputs[mode].flip(0), labs.flip(0), mode, score, 0, 1e-12, None if ov is None else ov.flip(0))
        err = np.concatenate([e1, e2])
        a = ometrics.auroc_from_samples(np.concatenate([s1, s2]), err)
        # one (error, correct) pair whose near-equal scores swap order under another CPU's last-bit rounding moves the AUROC by
        # 1 / (errors x correct): at most AUROC_PAIRS such swaps
        pairs = float(err.sum()) * float(err.size - err.sum())
        assert abs(a - float(g[key])) <= AUROC_PAIRS / pairs and s1.size + s2.size == int(g["nsamples:" + key[len("auroc:"):]])
    # hand-derived: perfectly separated scores give 1, reversed 0, one inversion among 2 x 2 gives 3/4
    assert ometrics.auroc_from_samples(np.array([0.9, 0.8, 0.2, 0.1]), np.array([1, 1, 0, 0])) == 1.0
    assert ometrics.auroc_from_samples(np.array([0.9, 0.8, 0.2, 0.1]), np.array([0, 0, 1, 1])) == 0.0
    assert ometrics.auroc_from_samples(np.array([0.9, 0.2, 0.8, 0.1]), np.array([1, 1, 0, 0])) == 0.75
    assert np.isnan(ometrics.auroc_from_samples(np.array([0.3, 0.2]), np.array([1, 1])))


def test_accuracy_vs_uncertainty_bins_golden():
    """oracle.metrics.ua_* against the counts / accuracies the reference's UncertaintyAccuracyAggregator produced."""
    g = golden("ua_bins_2x16x64")
    lab, prd, unc = (torch.from_numpy(g[k]) for k in ("labels", "preds", "uncertainty"))
    u1, c1 = ometrics.ua_samples(lab, prd, unc, (0, 7))
    u2, c2 = ometrics.ua_samples(lab.flip(0), prd.flip(0), unc.flip(0))
    u, c = np.concatenate([u1, u2]), np.concatenate([c1, c2])
    assert float(u.min()) >= 0.0 and float(u.max()) <= 1.0
    for tag, kw in (("bins10", {}), ("width0.05", {"bin_width": 0.05}), ("bins64", {"num_bins": 64}),
                    ("custom", {"bin_edges": np.array([0.0, 0.05, 0.3, 0.31, 0.8, 1.0], dtype=np.float32)})):
        edges = ometrics.ua_make_bins(kw.get("num_bins", 10), kw.get("bin_width"), kw.get("bin_edges"))
        assert np.array_equal(edges, g["edges:" + tag])
        n, acc, pct = ometrics.ua_binned(u, c, edges)
        assert np.array_equal(n, g["n:" + tag]) and np.allclose(acc, g["accuracy:" + tag], equal_nan=True, rtol=0, atol=0)
        assert abs(float(pct.sum()) - 100.0) < 1e-9
    # known answers: values on an interior edge go right, the last bin is closed
    n, acc, _ = ometrics.ua_binned(np.array([0.0, 0.5, 0.5, 1.0], np.float32), np.array([1, 0, 1, 1]), ometrics.ua_make_bins(2))
    assert n.tolist() == [1, 3] and acc.tolist() == [1.0, 2.0 / 3.0]


def test_tversky_golden():
    """oracle.losses.tversky against the reference's TverskyLoss values and gradients."""
    g = golden("tversky_2x20x8x64")
    lab, logits = torch.from_numpy(g["labels"]), torch.from_numpy(g["logits"])
    inputs = {"logits": logits, "probs": logits.softmax(1), "log_probs": logits.log_softmax(1)}
    wgt = torch.linspace(0.5, 1.5, 20)
    for act, inp in inputs.items():
        for red in ("mean", "sum", "none"):
            x = inp.clone().requires_grad_(True)
            lo = olosses.tversky(x, lab, 20, act, 0.7, 0.3, 1.0, 255, red)
            ((lo * wgt).sum() if red == "none" else lo).backward()
            assert _max_ulps(lo, g[f"loss:{act}|{red}"]) <= F32_ULPS
            assert _max_ulps_of_scale(x.grad, g[f"grad:{act}|{red}"]) <= F32_ULPS
    assert float(olosses.tversky(logits, torch.full((2, 8, 64), 255), 20, "logits")) == float(g["loss:all_ignored"]) == 0.0


def test_per_class_samples_golden():
    """oracle.metrics.PerClassSamples against the lists the reference's UncertaintyPerClassAggregator held (unlimited and capped)."""
    g = golden("per_class_uncertainty_3x2x16x64")
    for tag, cap in (("all", None), ("cap300", 300)):
        agg = ometrics.PerClassSamples(6, cap, seed=5)
        for b in range(3):
            agg.update(g["labels"][b], g["uncertainty"][b])
        assert np.array_equal(np.concatenate(agg.values), g["values:" + tag])
        assert [v.size for v in agg.values] == g["sizes:" + tag].tolist() and agg.seen == g["seen:" + tag].tolist()
    # known answer: scan order inside a class, labels outside [0, C) dropped
    agg = ometrics.PerClassSamples(2)
    agg.update(np.array([[1, 0, 5], [1, 1, 0]]), np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]], dtype=np.float32))
    assert np.allclose(agg.values[0], [0.2, 0.6]) and np.allclose(agg.values[1], [0.1, 0.4, 0.5]) and agg.seen == [2, 3]


def test_dirichlet_losses_golden():
    """oracle.dirichlet.loss_* against the reference's Dirichlet loss modules (values and gradients)."""
    from oracle import dirichlet as odir
    g = golden("dirichlet_losses_2x20x8x64")
    lab, alpha = torch.from_numpy(g["labels"]), torch.from_numpy(g["alpha"])
    fns = {"nll_dircat": lambda a: odir.loss_nll_dircat(a, lab, 0), "digamma_ce": lambda a: odir.loss_digamma_ce(a, lab, 0),
           "brier": lambda a: odir.loss_brier(a, lab, 0), "brier_sref40": lambda a: odir.loss_brier(a, lab, 0, 40.0),
           "mse": lambda a: odir.loss_mse(a, lab, 0), "kl_off_uniform": lambda a: odir.loss_kl_off_uniform(a, lab, 0),
           "complement_kl": lambda a: odir.loss_complement_kl(a, lab, 0, 1.25, 0.65, 0.15),
           "complement_kl_gated": lambda a: odir.loss_complement_kl(a, lab, 0, s_target=30.0, normalize=False, detach_uncert=False),
           "wrong_low_evidence": lambda a: odir.loss_wrong_low_evidence(a, lab, 0),
           "wrong_low_evidence_hard": lambda a: odir.loss_wrong_low_evidence(a, lab, 0, 4.0, 0.1, 0.0),
           "wrong_low_evidence_nomargin": lambda a: odir.loss_wrong_low_evidence(a, lab, None, margin=0.0)}
    for name, fn in fns.items():
        a = alpha.clone().requires_grad_(True)
        lo = fn(a)
        lo.backward()
        assert _max_ulps(lo, g["loss:" + name]) <= F32_ULPS
        assert _max_ulps_of_scale(a.grad, g["grad:" + name]) <= F32_ULPS
    # known answers at the uniform prior alpha = 1 (C = 4): NLL = ln 4; digamma-CE = psi(4) - psi(1) = 1 + 1/2 + 1/3
    one = torch.ones(1, 4, 1, 2)
    y = torch.tensor([[[1, 3]]])
    assert abs(float(odir.loss_nll_dircat(one, y)) - math.log(4.0)) < 1e-6
    assert abs(float(odir.loss_digamma_ce(one, y)) - (1.0 + 0.5 + 1.0 / 3.0)) < 1e-6
    # complement-KL: off-class mass spread evenly -> 0; all of it on one off class -> ln(C-1) (1 when normalised), times the gate
    even = torch.tensor([5.0, 1.0, 1.0, 1.0]).view(1, 4, 1, 1)
    peak = torch.tensor([5.0, 3.0, 1e-9, 1e-9]).view(1, 4, 1, 1)
    y0 = torch.zeros(1, 1, 1, dtype=torch.int64)
    assert abs(float(odir.loss_complement_kl(even, y0, None))) < 1e-6
    py = 5.0 / 8.0
    gate = (1.0 - py) ** 2.0 / (1.0 + math.exp(-(0.55 - py) / 0.12))
    assert abs(float(odir.loss_complement_kl(peak, y0, None)) - gate) < 1e-5
    # wrong-low-evidence: a confidently wrong pixel with alpha0 = 2 C pays ln(2)^2 (hard margin: the gate is 1); a right one pays 0
    wrong = torch.tensor([1.0, 7.0]).view(1, 2, 1, 1).repeat(1, 1, 1, 2) * torch.tensor([1.0, 0.5]).view(1, 1, 1, 2)
    yw = torch.tensor([[[0, 1]]])
    assert abs(float(odir.loss_wrong_low_evidence(wrong[..., :1] * 0.5, yw[..., :1], None, 0.0, 0.1, 0.0)) - math.log(2.0) ** 2) < 1e-5
    assert float(odir.loss_wrong_low_evidence(wrong[..., 1:], yw[..., 1:], None, 0.0, 0.1, 0.0)) == 0.0


def test_normals_known_answers():
    """oracle.normals (Scharr restated from OpenCV's definition; parity unpinned, see its header): planes, a sphere, the border rule."""
    from oracle import normals as onorm
    h, w = 12, 40
    j, i = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    # Scharr of a ramp: (3 + 10 + 3) * 2 * slope * scale in the interior, 0 on the reflected border
    assert np.allclose(onorm.scharr(2.0 * j, 1, 0, 4.0)[1:-1, 1:-1], 16 * 2 * 2.0 * 4.0) and np.all(onorm.scharr(2.0 * j, 1, 0)[:, 0] == 0)
    assert np.all(onorm.scharr(2.0 * j, 0, 1) == 0) and np.allclose(onorm.scharr(3.0 * i, 0, 1)[1:-1], 16 * 2 * 3.0)
    # a plane z = 0.1 col + 0.2 row: n = -(d/dcol x d/drow) = (0.1, 0.2, -1) / |.|
    n = onorm.build_normal_xyz(np.dstack([j, i, 0.1 * j + 0.2 * i]))
    want = np.array([0.1, 0.2, -1.0]) / np.linalg.norm([0.1, 0.2, -1.0])
    assert n.dtype == np.float32 and np.allclose(n[1:-1, 1:-1], want, atol=1e-6) and np.all(n[0, 0] == 0)
    # a sphere sampled on an (elevation, azimuth) grid like a range image: the normal is radial up to sign and discretisation
    el, az = np.meshgrid(np.linspace(0.4, -0.4, 32), np.linspace(np.pi, -np.pi, 256, endpoint=False), indexing="ij")
    p = 10.0 * np.dstack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    n = onorm.build_normal_xyz(p)[1:-1, 1:-1]
    radial = (p / 10.0)[1:-1, 1:-1]
    assert np.abs(np.abs((n * radial).sum(-1)) - 1.0).max() < 1e-3 and np.allclose(np.linalg.norm(n, axis=-1), 1.0, atol=1e-5)


def test_spherical_projection_golden_and_known_answers():
    """oracle.projection against the image the reference's dataset.utils.spherical_projection produced."""
    from oracle import projection as oproj
    g = golden("spherical_projection_30000x5_32x256")
    for tag, tr in (("data_range", None), ("fixed_range", [-np.pi / 8, np.pi / 8])):
        img, alpha, th, ph = oproj.spherical_projection(g["cloud"], 32, 256, theta_range=tr)
        assert np.array_equal(img, g["img:" + tag]) and np.array_equal(np.asarray(th, dtype=np.float64), g["theta_range:" + tag])
        assert alpha.shape == (32, 256) and ph == (-np.pi, np.pi)
    # two points in one pixel: the nearer one survives; a point on the +x axis (phi = 0) lands in the middle column
    pts = np.array([[10.0, 0.0, 0.0, 0.5, 3.0], [5.0, 0.0, 0.0, 0.9, 7.0], [0.0, -8.0, 1.0, 0.1, 2.0]])
    img, _, _, _ = oproj.spherical_projection(pts, 4, 8, theta_range=[-0.5, 0.5])
    assert np.count_nonzero(img[..., 0] != 0) + np.count_nonzero(img[..., 1] != 0) == 2
    assert float(img[..., 3].max()) == np.float32(0.9) and 7.0 in img[..., 4] and 3.0 not in img[..., 4]


def _ece_batches(x, lab):
    return [(x, lab), (np.flip(x, 0), np.flip(lab, 0)), (np.roll(x, 1, 3), np.roll(lab, 1, 2)), (np.flip(x, 3), np.flip(lab, 2))]


def test_ece_reservoir_and_adaptive_binning_match_reference():
    """metrics/ece.py:93-128 (golden: tools/gen_golden_r02.py): buffers after the seeded reservoir, equal-mass edges, bins, ECE / MCE."""
    g = golden("ece_capped_adaptive_2x20x16x64")
    for mode in ("probs", "logits", "alpha"):
        for cap, binning in ((3000, "uniform"), (None, "adaptive"), (2500, "adaptive")):
            tag = f"{mode}|{cap}|{binning}"
            buf = ometrics.ECESamples(cap, seed=0)
            for xb, lb in _ece_batches(g[mode], g["labels"]):
                buf.update(*ometrics.top_label(np.ascontiguousarray(xb), np.ascontiguousarray(lb), 0, mode))
            assert buf.seen == int(g["seen:" + tag]) and buf.conf.size == int(g["kept:" + tag])
            assert np.array_equal(np.sort(buf.conf), g["conf_sorted:" + tag]) and int(buf.correct.sum()) == int(g["ncorrect:" + tag])
            edges = ometrics.ece_edges(buf.conf, 15, binning)
            assert np.array_equal(edges, g["edges:" + tag])
            n, acc_s, conf_s = ometrics.ece_bins_over(buf.conf, buf.correct, edges)
            assert np.array_equal(n, g["n:" + tag])
            e, m = ometrics.ece_from_bins(n, acc_s, conf_s)
            assert abs(e - float(g["ece:" + tag])) <= 1e-7 and abs(m - float(g["mce:" + tag])) <= 1e-7
    c, _ = ometrics.top_label(g["onehot_probs"], g["onehot_labels"], 0, "probs")
    assert np.array_equal(ometrics.ece_edges(c, 15, "adaptive"), np.linspace(0, 1, 16, dtype=np.float32))   # duplicate quantiles -> uniform


def test_kitti_sample_and_projection_options_match_reference():
    """f-3 (golden: tools/gen_golden_r02.py kitti, produced by the reference's SemanticKitti.__getitem__ / spherical_projection):
    decode + id_map + rotate + projection + flip + range, and the sort_largest_first / bins_h options of the projection."""
    from oracle import kitti as okitti, projection as oproj
    g = golden("kitti_sample_16000_32x256")
    id_map = {int(k): int(v) for k, v in zip(g["id_map_keys"], g["id_map_values"])}
    for tag, flip in (("plain", False), ("rot", False), ("flip", True), ("rotflip", True)):
        angle = None if np.isnan(float(g[f"{tag}:angle"])) else float(g[f"{tag}:angle"])
        got = okitti.sample(g["xyzi"].tobytes(), g["label"].tobytes(), id_map, (32, 256), angle, flip)
        for name, arr in zip(("range", "reflectivity", "xyz", "normals", "semantics"), got):
            assert np.array_equal(arr, g[f"{tag}:{name}"]), (tag, name)
    cloud = okitti.decode(g["xyzi"].tobytes(), g["label"].tobytes(), id_map)
    beams = g["beams"]
    for tag, kw in (("farthest", dict(sort_largest_first=True)), ("bins_h", dict(bins_h=beams)), ("bins_h_increasing", dict(bins_h=beams[::-1].copy())),
                    ("farthest_bins_h_range", dict(sort_largest_first=True, bins_h=beams, theta_range=(-0.45, 0.05)))):
        img, _, th, _ = oproj.spherical_projection(cloud, 32, 256, **kw)
        assert np.array_equal(img, g[f"proj:{tag}:img"]) and np.allclose(th, g[f"proj:{tag}:theta"], rtol=0, atol=0)


def test_fpn_resnet50_oracle_matches_reference_golden():
    """a3 widened to the Bottleneck backbone (golden: tools/gen_golden_r02.py fpn_resnet50 -- the reference's own semanticFCN wiring on this
    repo's state_dict, through the stub torchvision that serves oracle.fpn's restated ResNet)."""
    from oracle import fpn as ofpn
    from semanticlidarunc_amd.fpn import SemanticNetworkWithFPN
    from semanticlidarunc_amd.testing import randomize_bn_
    g = golden("fpn_resnet50_m3_c5")
    torch.manual_seed(0)
    model = randomize_bn_(SemanticNetworkWithFPN(backbone="resnet50", input_channels=2, meta_channel_dim=3, num_classes=5), 3).eval()
    sd = model.state_dict()
    fl = [v for v in sd.values() if v.is_floating_point()]
    assert np.allclose([sum(float(v.double().sum()) for v in fl), sum(float(v.double().abs().sum()) for v in fl)], g["sd_digest"], rtol=1e-10)
    assert sd["backbone.layer4.2.conv3.weight"].shape == (2048, 512, 1, 1) and sd["fpn_block4.0.weight"].shape == (1024, 2048, 3, 3)
    with torch.no_grad():
        y = ofpn.fpn_forward(sd, _t(g["x"]), _t(g["meta"]), "resnet50", True, True)
    # 50 float32 layers over randomised BatchNorm: the golden host's conv kernels and thread partitions leave 2e-5 .. 8e-5 of the output
    # scale of rounding noise (measured over hosts and thread counts), so the bound is 2e-4 of it where the shallower backbones keep 1e-5
    assert float((y - _t(g["out"])).abs().max()) <= 2e-4 * max(1.0, float(np.abs(g["out"]).max()))


def test_fpn_opt_oracle_matches_reference_golden():
    """f-4 (golden: tools/gen_golden_r02.py fpn_opt, the reference's own semanticFCN_opt head wiring on this repo's state_dict)."""
    from oracle import fpn_opt as ofpo
    from semanticlidarunc_amd.fpn_opt import SemanticNetworkWithFPN
    from semanticlidarunc_amd.testing import randomize_bn_
    for tag, kw in (("resnet18_m6_c20", dict(backbone="resnet18", input_channels=2, meta_channel_dim=6, num_classes=20)),
                    ("resnet34_m3_c21_noatt", dict(backbone="resnet34", input_channels=2, meta_channel_dim=3, num_classes=21, attention=False,
                                                   multi_scale_meta=False)),
                    ("resnet50_m3_c5", dict(backbone="resnet50", input_channels=2, meta_channel_dim=3, num_classes=5))):
        g = golden("fpn_opt_" + tag)
        torch.manual_seed(0)
        m = randomize_bn_(SemanticNetworkWithFPN(**kw), 3).eval()
        with torch.no_grad():
            gg = torch.Generator().manual_seed(9)
            for mod in m.modules():
                if isinstance(mod, torch.nn.GroupNorm):
                    mod.weight.copy_(torch.rand(mod.num_channels, generator=gg) + 0.5)
                    mod.bias.copy_(torch.randn(mod.num_channels, generator=gg) * 0.1)
        sd = m.state_dict()
        dig = [sum(float(v.double().sum()) for v in sd.values() if v.is_floating_point()), sum(float(v.double().abs().sum()) for v in sd.values() if v.is_floating_point())]
        assert np.allclose(dig, g["sd_digest"], rtol=1e-12)
        with torch.no_grad():
            y = ofpo.fpn_opt_forward(sd, _t(g["x"]), _t(g["meta"]), kw["backbone"], kw.get("attention", True), kw.get("multi_scale_meta", True))
            yd = ofpo.fpn_opt_forward(sd, _t(g["x"]), _t(g["meta"]), kw["backbone"], kw.get("attention", True), kw.get("multi_scale_meta", True),
                                      dropout_scale=_t(g["dropout_scale"]))
        assert float((y - _t(g["out"])).abs().max()) <= 1e-5 and float((yd - _t(g["out_dropout"])).abs().max()) <= 1e-5
    keys = json.load(open(os.path.join(GOLDEN, "fpn_opt_resnet18_state_dict_keys.json")))
    torch.manual_seed(0)
    mine = SemanticNetworkWithFPN("resnet18", 2, 6, num_classes=20).state_dict()
    assert list(mine.keys()) == list(keys.keys()) and all(list(v.shape) == keys[k] for k, v in mine.items())


def test_confidence_weighted_kl_oracle_matches_reference_golden():
    from oracle import dirichlet as odir
    g = golden("kl_off_weighted_2x20x8x64")
    for gamma in (1.0, 2.5):
        a = _t(g["alpha"]).clone().requires_grad_(True)
        loss = odir.loss_kl_off_uniform(a, _t(g["labels"]), 0, with_conf_weighting=True, gamma=gamma)
        loss.backward()
        assert float(loss.detach()) == float(g[f"loss:gamma{gamma}"]) and float((a.grad - _t(g[f"grad:gamma{gamma}"])).abs().max()) == 0.0
