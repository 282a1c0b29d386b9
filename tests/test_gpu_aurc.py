"""GPU: AURC / E-AURC (DESIGN "AURC on the device") -- the post-sort kernels against the fp64 restatement that test_aurc_cpu.py
pins to the reference, the per-pixel sample kernel against torch on the CPU, and the drop-in aggregator / batch function against
the reference's golden values.

Bounds.  Counts (E, m, s_m, recall numerators) are exact.  AURC, AURC_opt and EAURC are fp64 sums of <= 6e5 non-negative terms
whose sum is <= 1; device and numpy differ in summation order only, which is bounded by n 2^-53 ~ 7e-11: 1e-9 absolute.  Curve
points are single correctly rounded fp64 quotients of exact integers: 1e-15.  Against the golden values the confidences carry the
last-bit logf differences of the entropy, which can swap neighbours in the ranking: 1e-5 absolute on AURC / EAURC, the bar
test_gpu_auroc.py uses for the same cause.  Largest differences observed on an MI355X: OBSERVED below and the docstrings of the golden tests."""
import numpy as np
import pytest
import torch

from aurc_restatement import KS, restate
from conftest import golden
from semanticlidarunc_amd import ops
from semanticlidarunc_amd._lib import SluError
from semanticlidarunc_amd.metrics import aurc as maurc

pytestmark = pytest.mark.gpu

# maxima as printed by the tests below on an MI355X
OBSERVED = ("against the restatement: |AURC| 2.1e-15, |AURC_opt| 6.9e-18 (n = 600 011); sample kernel: |conf - cpu| 3.0e-7 (entropy form, "
            "0 for the other two); against the golden values: |AURC| = |EAURC| = 4.4e-7 (one batch, entropy form), 2.2e-7 (two batches), "
            "<= 1.2e-16 for the max-prob and ent_mc forms and the reservoir; kept confidences 1.8e-7 (entropy form), 0 otherwise")

SIZES = (1, 2, 3, 2047, 2048, 2049, 4097, 600_011)        # around the 2048-key sort tile; the last one is 293 tiles (> 256: the scans loop)
KINDS = ("tiefree", "ties8", "allequal", "zeros", "E0", "En")


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _inputs(n, kind):
    gen = torch.Generator().manual_seed(1000 + n % 997 + 7 * KINDS.index(kind))
    if kind == "ties8":                                   # 8 values, both signs: groups cross tile boundaries
        conf = torch.randint(0, 8, (n,), generator=gen).float() / 8 - 0.4
    elif kind == "allequal":
        conf = torch.full((n,), 0.25)
    elif kind == "zeros":                                 # +0.0 and -0.0 are one group
        conf = torch.where(torch.rand(n, generator=gen) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    else:                                                 # distinct values of both signs
        conf = torch.randperm(n, generator=gen).float() / n - 0.3
    if kind == "E0":
        err = torch.zeros(n, dtype=torch.uint8)
    elif kind == "En":
        err = torch.ones(n, dtype=torch.uint8)
    else:
        err = (torch.rand(n, generator=gen) < 0.3).to(torch.uint8)
    return conf, err


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_post_sort_kernels_against_restatement(cuda, n, kind):
    conf, err = _inputs(n, kind)
    if kind in ("tiefree", "E0", "En"):
        assert torch.unique(conf).numel() == n
    want = restate(conf.numpy(), err.numpy())
    got = ops.aurc_from_samples(conf.to(cuda), err.to(cuda), want_curve=True, want_sorted=True)
    again = ops.aurc_from_samples(conf.to(cuda), err.to(cuda))
    print(f"n={n} {kind}: dAURC {abs(got.aurc - want['AURC']):.3e} dOpt {abs(got.aurc_opt - want['AURC_opt']):.3e} m {got.num_points}")
    assert (got.num_errors, got.num_points, got.last_start) == (want["E"], want["m"], want["s_m"])
    assert abs(got.aurc - want["AURC"]) <= 1e-9 and abs(got.aurc_opt - want["AURC_opt"]) <= 1e-9 and abs(got.eaurc - want["EAURC"]) <= 1e-9
    den = max(want["E"], 1)
    assert got.recalls == [num / den for num in want["recall_num"]]                  # exact numerators, one fp64 division
    assert got.coverages.shape == (want["m"] + 1,) and got.rc_risks.shape == (want["m"] + 1,)
    assert float((got.coverages.cpu() - _t(want["cov"])).abs().max()) <= 1e-15
    assert float((got.rc_risks.cpu() - _t(want["risk"])).abs().max()) <= 1e-15
    sc, order = torch.sort(conf, stable=True)
    assert torch.equal(got.sorted_confids.cpu(), sc) and torch.equal(got.sorted_is_error.cpu(), err[order])
    assert again[:7] == got[:7]                                                      # bit-identical scalars run to run


def _cpu_samples(probs, labels, ent_mc, ignore, maxprob):
    """torch on the CPU, fp32: the reference's formulas (metrics/aurc.py _flatten_batch) before the valid-pixel selection."""
    pred = probs.argmax(1)
    if maxprob:
        conf = probs.max(1).values
    else:
        ent = maurc.entropy_from_probs(probs) if ent_mc is None else ent_mc
        conf = 1.0 - ent.clamp(0, 1)
    return conf, (pred != labels), labels != ignore


@pytest.mark.parametrize("ignored", (True, False))
@pytest.mark.parametrize("form", ("maxprob", "ent_mc", "entropy"))
@pytest.mark.parametrize("shape", ((2, 20, 16, 64), (1, 32, 4, 100)))
def test_sample_kernel_against_torch_cpu(cuda, shape, form, ignored):
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(sum(shape) + len(form))
    probs = (torch.randn(shape, generator=gen) * 2).softmax(1)
    if c == 32:
        probs = probs * 0.9                                # not normalised: the kernel takes the probabilities as given
    probs[0, :, 0, 0] = 0.0                                # an all-zero pixel: first argmax = class 0, entropy through eps
    probs[0, 3, 0, 1] = probs[0, :, 0, 1].max()            # a tied maximum: the first one wins
    probs[0, 1, 0, 1] = probs[0, 3, 0, 1]
    labels = torch.randint(0, c, (b, h, w), generator=gen)
    if ignored:
        labels[torch.rand(b, h, w, generator=gen) < 0.2] = 255
    ent = (torch.rand(b, h, w, generator=gen) * 1.4 - 0.2) if form == "ent_mc" else None      # some outside [0, 1]: clamped
    want_conf, want_err, want_valid = _cpu_samples(probs, labels, ent, 255, form == "maxprob")
    conf, flag = ops.aurc_samples(probs.to(cuda), labels.to(cuda), 255, None if ent is None else ent.to(cuda), form == "maxprob")
    conf, flag = conf.cpu(), flag.cpu()
    valid = flag != 2
    assert torch.equal(valid, want_valid) and bool(valid.all()) == (not ignored)
    d = float((conf - want_conf).abs().max())
    print(f"{shape} {form}: max |conf - cpu| = {d:.3e}")
    assert d <= 2e-6
    assert float((flag[valid] != want_err[valid].to(torch.uint8)).float().mean()) < 1e-5


def _fixture(cuda):
    g = golden("aurc_2x20x16x64")
    return g, _t(g["probs"]).to(cuda), _t(g["labels"])[:, None].to(cuda), _t(g["ent_mc"]).to(cuda)


@pytest.mark.parametrize("form", ("maxprob", "entropy", "ent_mc"))
def test_batch_function_and_two_batch_aggregator_against_golden(cuda, form):
    """Largest differences observed (MI355X): |AURC| = |EAURC| = 4.4e-7 for one batch and 2.2e-7 for two in the entropy form (kept
    confidences within 1.8e-7), <= 1.2e-16 in the max-prob and ent_mc forms, which involve no transcendental; bound 1e-5."""
    g, probs, sem, ent = _fixture(cuda)
    e0 = ent[0] if form == "ent_mc" else None
    tag = "batch:" + form
    res = maurc.compute_batch_uncertainty_metrics(probs, sem, e0, 255, form == "maxprob", KS)
    conf, flag = ops.aurc_samples(probs, sem[:, 0].contiguous(), 255, e0, form == "maxprob")
    kept = torch.sort(conf[flag != 2]).values.cpu()
    d_conf = float((kept - _t(np.sort(g[tag + ":confids"]))).abs().max())
    d = (abs(res["AURC"] - float(g[tag + ":AURC"])), abs(res["EAURC"] - float(g[tag + ":EAURC"])))
    print(f"batch {form}: dAURC {d[0]:.3e} dEAURC {d[1]:.3e} dconf {d_conf:.3e}")
    assert d_conf <= 2e-6 and max(d) <= 1e-5
    assert res["num_pixels"] == int(g[tag + ":num_pixels"]) and res["num_errors"] == int(g[tag + ":num_errors"])
    assert res["valid_mask_shape"] == (2, 16, 64) and tuple(res["ks"]) == KS
    assert res["coverages"].shape == res["rc_risks"].shape and res["coverages"][0] == 1.0
    if form == "maxprob":                                  # no transcendental: the ranking is the reference's
        assert res["coverages"].size == int(g[tag + ":npoints"])
        assert np.abs(res["recalls"] - g[tag + ":recalls"]).max() <= 2.0 ** -24          # the reference divides in fp32
        assert d_conf == 0.0
    agg = maurc.UncertaintyAggregator(ignore_index=255, use_max_prob_confidence=form == "maxprob")
    agg.add_batch(probs, sem, e0)
    agg.add_batch(probs.flip(0), sem.flip(0), None if e0 is None else e0.flip(0))
    fin = agg.finalize(make_plots=False)
    d = (abs(fin["AURC"] - float(g["agg:" + form + ":AURC"])), abs(fin["EAURC"] - float(g["agg:" + form + ":EAURC"])))
    print(f"two-batch {form}: dAURC {d[0]:.3e} dEAURC {d[1]:.3e}")
    assert max(d) <= 1e-5 and fin["num_pixels"] == int(g["agg:" + form + ":num_pixels"])
    assert fin["rc_curve_path"] is None and fin["error_recall_path"] is None


def test_reservoir_against_golden_and_plots(cuda, tmp_path, monkeypatch):
    """Largest differences observed (MI355X): 0 on the kept confidences, on AURC and on EAURC (ent_mc form); bound 2e-6 / 1e-5."""
    g, probs, sem, ent = _fixture(cuda)
    agg = maurc.UncertaintyAggregator(ignore_index=255, reservoir_size=1500, seed=0)
    for k in range(3):
        agg.add_batch(probs, sem, ent[k])
    conf, err = agg._buf.materialize()
    assert conf.is_cuda and conf.numel() == 1500
    d_conf = float((torch.sort(conf).values.cpu() - _t(g["res:kept_sorted"])).abs().max())
    calls = []
    real = ops.aurc_from_samples
    monkeypatch.setattr(ops, "aurc_from_samples", lambda *a, **k: calls.append(k.get("want_curve")) or real(*a, **k))
    fin = agg.finalize(make_plots=False)
    d = (abs(fin["AURC"] - float(g["res:AURC"])), abs(fin["EAURC"] - float(g["res:EAURC"])))
    print(f"reservoir: dAURC {d[0]:.3e} dEAURC {d[1]:.3e} dconf {d_conf:.3e}")
    assert d_conf <= 2e-6 and max(d) <= 1e-5 and fin["num_pixels"] == 1500
    assert calls == [False]                                # no curve buffers without plots
    fin = agg.finalize(make_plots=True, save_dir=str(tmp_path), epoch=3, filename_prefix="val_")
    assert calls == [False, True]
    assert fin["rc_curve_path"].endswith("val_epoch_000003_rc_curve.png") and (tmp_path / "val_epoch_000003_rc_curve.png").stat().st_size > 0
    assert (tmp_path / "val_epoch_000003_uncertainty_error_recall.png").stat().st_size > 0


def test_argument_checks(cuda):
    probs = torch.full((1, 4, 2, 8), 0.25)
    labels = torch.zeros(1, 2, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.aurc_samples(probs, labels, 255)                                          # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        ops.aurc_from_samples(torch.zeros(4), torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        ops.aurc_samples(probs.to(cuda), labels[:, :1].contiguous().to(cuda), 255)    # labels of another shape
    with pytest.raises(RuntimeError):
        ops.aurc_samples(probs.to(cuda), labels.to(cuda), 255, ent_mc=torch.zeros(1, 2, 4, device=cuda))
    with pytest.raises(RuntimeError):
        ops.aurc_from_samples(torch.zeros(4, device=cuda), torch.zeros(5, dtype=torch.uint8, device=cuda))
    with pytest.raises(RuntimeError):
        ops.aurc_from_samples(torch.zeros(4, device=cuda), torch.zeros(4, dtype=torch.uint8, device=cuda), ks=range(17))
    with pytest.raises(SluError, match="code -2"):                                    # C = 33: not instantiated
        ops.aurc_samples(torch.zeros(1, 33, 2, 8, device=cuda), labels.to(cuda), 255)
    with pytest.raises(RuntimeError, match="No batches added"):
        maurc.UncertaintyAggregator().finalize()
    with pytest.raises(RuntimeError, match="No batches added"):
        maurc.UncertaintyAggregator(reservoir_size=10, seed=0).finalize(make_plots=False)
