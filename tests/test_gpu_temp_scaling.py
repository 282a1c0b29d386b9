"""GPU: temperature scaling on the device (DESIGN "Temperature scaling on the device") -- the cache kernel and the fused NLL(T)
closure against the fp64 restatement that test_temp_scaling_cpu.py pins to the reference, the two fits against the fixture's fp64
minimiser and Adam iteration, and the drop-in module end to end.

Bounds.
  calib_rows: order, labels and counts exact; values within 2 ulp of the restatement (the logarithm, in fp64, of the correctly rounded
    fp32 probability): the kernel rounds both the probability and its logarithm from fp64.
  temp_nll: per case 4 x the error of the reference's own fp32 CPU evaluation (CrossEntropyLoss(reduction="sum") on x / T and its
    autograd gradient) against the restatement on the same data, as stored in tests/golden/temp_scaling_nll.npz.  That error is 0 where
    the result is 0 in every arithmetic (C = 1; g under the clamp; a one-row case whose loss underflows to 0), and the kernel must
    return 0 there too.  An fp32 row evaluation misses this bar in about 20 of the 360 cases (the reference's fp32 errors cancel to a
    tenth of their usual size there), which is why the kernel evaluates a row in fp64.
  LBFGS: |T - T64| <= 4 x max over the fixture's chunk sizes of |T_ref32 - T64|.
  Adam: |T - restatement| <= 4 x |T_ref32_adam - restatement| of the fixture, same seed, same permutations.
Largest figures observed on an MI355X: OBSERVED below."""
import numpy as np
import pytest
import torch

import temp_scaling_restatement as rs
from conftest import golden
from semanticlidarunc_amd import ops
from semanticlidarunc_amd._lib import SluError
from semanticlidarunc_amd.loss import temp_nll_loss
from semanticlidarunc_amd.metrics.ece import ECEAggregator
from semanticlidarunc_amd.models import temp_scaling as ts

pytestmark = pytest.mark.gpu

# maxima as printed by the tests below on an MI355X
OBSERVED = ("calib_rows: 0 ulp in all 25 (C, shape) cases; temp_nll: |error| <= 3.7e-9 (on a loss_sum of 2.5e7), at most 1.0e-7 of the bar "
            "where the bar is not 0, exact zeros where it is; LBFGS: |T - T64| 2.8e-7 against a bar of 1.17e-6 (2.7e-6 and 2.0e-7 from the "
            "start values 4 and 9, reach 6.4e-6); Adam: |T - restatement| 7.5e-10 against a bar of 7.0e-8; end to end: ECE 0.4365 at "
            "T = 1, 0.0733 at the fitted T = 4.6109")

CS = (1, 3, 20, 21, 32)
SHAPES = ((1, 1, 1), (1, 1, 63), (2, 3, 67), (3, 2, 257), (1, 4, 1024))
KINDS = ("logits", "probs", "log_probs")
PATTERNS = ("none", "no_ignore_index", "all", "every_other", "block_ends_ignored", "block_ends_valid", "image")
CFG = {"model_settings": {"baseline": "SalsaNext", "reflectivity": 0, "normals": 0}}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _labels(pattern, b, h, w, c, gen):
    lab = torch.randint(0, c, (b, h * w), generator=gen)
    pos = torch.arange(b * h * w).reshape(b, h * w)
    ends = (pos % 256 == 0) | (pos % 256 == 255)
    if pattern == "all":
        lab[:] = 255
    elif pattern == "every_other":
        lab[pos % 2 == 1] = 255
    elif pattern == "block_ends_ignored":
        lab[ends] = 255
    elif pattern == "block_ends_valid":
        lab[~ends] = 255
    elif pattern == "image":
        lab[b - 1] = 255
    return lab.reshape(b, h, w)


def _outputs(b, c, h, w, gen):
    """The same scores in the three output kinds; the probabilities carry exact zeros and values below 1e-12."""
    z = torch.randn(b, c, h, w, generator=gen) * 3.0
    z[:, :, :, ::3] *= 4.0                                         # confident columns: p_max within a few ulp of 1
    p = z.double().softmax(1).float()
    p[torch.rand(p.shape, generator=gen) < 0.05] = 0.0
    p[torch.rand(p.shape, generator=gen) < 0.05] = 3e-13
    return {"logits": z, "probs": p, "log_probs": z.double().log_softmax(1).float()}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", CS)
def test_calib_rows_against_restatement(cuda, c, shape):
    """Observed: 0 ulp in every case; order, labels and counts exact."""
    b, h, w = shape
    gen = torch.Generator().manual_seed(100 * c + b * h * w)
    outs = _outputs(b, c, h, w, gen)
    worst = 0
    for pattern in PATTERNS:
        lab = _labels(pattern, b, h, w, c, gen)
        ignore = None if pattern == "no_ignore_index" else 255
        for kind in KINDS:
            want_rows, want_lab = rs.cache_rows(outs[kind].numpy(), kind, lab.numpy(), ignore)
            cap = b * h * w + 3
            rows = torch.full((cap, c), 7.0, device=cuda)
            row_labels = torch.full((cap,), -7, dtype=torch.int64, device=cuda)
            count = torch.zeros(1, dtype=torch.int64, device=cuda)
            ops.calib_rows(outs[kind].to(cuda), kind, lab.to(cuda), ignore, rows, row_labels, count)
            n = int(count.item())
            assert n == want_lab.size, (pattern, kind)
            assert np.array_equal(row_labels[:n].cpu().numpy(), want_lab), (pattern, kind)
            assert bool((rows[n:] == 7.0).all()) and bool((row_labels[n:] == -7).all()), (pattern, kind)      # nothing past the rows
            d = rs.ulp_distance(rows[:n].cpu().numpy(), want_rows)
            worst = max(worst, d)
            assert d <= 2, (pattern, kind, d)
    print(f"C={c} {shape}: {worst} ulp")


def test_calib_rows_appends_and_respects_the_capacity(cuda):
    gen = torch.Generator().manual_seed(5)
    c, (b, h, w) = 20, (2, 3, 67)
    outs = _outputs(b, c, h, w, gen)
    labs = [_labels("every_other", b, h, w, c, gen), _labels("all", b, h, w, c, gen), _labels("image", b, h, w, c, gen)]
    want = [rs.cache_rows(outs["logits"].numpy(), "logits", l.numpy(), 255) for l in labs]
    want_rows, want_lab = np.concatenate([r for r, _ in want]), np.concatenate([l for _, l in want])
    total = want_lab.size
    assert want[1][1].size == 0 and total == 201 + 201
    for cap in (3 * b * h * w, total, total - 1, 150, 201):       # roomy, exact, one short, full inside the first batch, full at its end
        store = torch.full((cap + 300, c), 7.0, device=cuda)
        store_lab = torch.full((cap + 300,), -7, dtype=torch.int64, device=cuda)
        count = torch.zeros(1, dtype=torch.int64, device=cuda)
        for l in labs:
            ops.calib_rows(outs["logits"].to(cuda), "logits", l.to(cuda), 255, store[:cap], store_lab[:cap], count)
        assert int(count.item()) == total                         # the count runs on: count > cap tells that rows were dropped
        kept = min(cap, total)
        assert np.array_equal(store_lab[:kept].cpu().numpy(), want_lab[:kept])
        assert rs.ulp_distance(store[:kept].cpu().numpy(), want_rows[:kept]) <= 2
        assert bool((store[kept:] == 7.0).all()) and bool((store_lab[kept:] == -7).all())


def test_wrappers_reject_wrong_tensors(cuda):
    out, lab = torch.zeros(1, 3, 2, 4, device=cuda), torch.zeros(1, 2, 4, dtype=torch.int64, device=cuda)
    rows, rl, cnt = torch.zeros(8, 3, device=cuda), torch.zeros(8, dtype=torch.int64, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda)
    lt = torch.zeros(1, device=cuda)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.calib_rows(out.permute(0, 1, 3, 2), "logits", lab, 255, rows, rl, cnt)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.calib_rows(out, "logits", lab.int(), 255, rows, rl, cnt)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.calib_rows(out.double(), "logits", lab, 255, rows, rl, cnt)
    with pytest.raises(RuntimeError, match="expected"):
        ops.calib_rows(out, "logits", lab, 255, torch.zeros(8, 4, device=cuda), rl, cnt)
    with pytest.raises(RuntimeError, match="expected"):
        ops.calib_rows(out, "logits", lab[:, :1], 255, rows, rl, cnt)
    with pytest.raises(ValueError, match="Unknown output kind"):
        ops.calib_rows(out, "alpha", lab, 255, rows, rl, cnt)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.temp_nll(torch.zeros(3, 8, device=cuda).t(), rl, lt)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.temp_nll(rows, rl.int(), lt)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.temp_nll(rows, rl, lt.double())
    with pytest.raises(RuntimeError, match="dtype"):
        ops.temp_nll(rows, rl, lt, torch.zeros(4, dtype=torch.int32, device=cuda))
    with pytest.raises(RuntimeError, match="expected"):
        ops.temp_nll(rows, rl[:4], lt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.temp_nll(rows, rl, torch.zeros(1))
    with pytest.raises(SluError, match="slu_temp_nll"):
        ops.temp_nll(torch.zeros(4, 33, device=cuda), rl[:4], lt)                 # more than 32 classes
    with pytest.raises(SluError, match="slu_calib_rows"):
        ops.calib_rows(torch.zeros(1, 33, 2, 4, device=cuda), "logits", lab, 255, torch.zeros(8, 33, device=cuda), rl, cnt)
    assert int(cnt.item()) == 0


@pytest.fixture(scope="module")
def nll_golden():
    return golden("temp_scaling_nll")


@pytest.mark.parametrize("c", rs.NLL_CS)
@pytest.mark.parametrize("n", rs.NLL_NS)
def test_temp_nll_against_restatement(cuda, nll_golden, n, c):
    """Observed: the largest |error| / bar over the cases with a bar > 0 is printed per (N, C); exact zeros where the bar is 0."""
    g = nll_golden
    i, j = rs.NLL_NS.index(n), rs.NLL_CS.index(c)
    x, y = rs.nll_case(g["rows"], g["labels"], n, c)
    assert n < 64 or c < 3 or (x == np.float32(-27.631021)).any()
    xd, yd = _t(x).to(cuda), _t(y).to(cuda)
    worst = 0.0
    for k, lt in enumerate(rs.NLL_LOG_TS):
        ltd = torch.tensor([float(lt)], dtype=torch.float32, device=cuda)
        for v, variant in enumerate(rs.NLL_VARIANTS):
            idx = rs.nll_index(variant, n)
            idxd = None if idx is None else _t(idx).to(cuda)
            loss, gs, bad = ops.temp_nll(xd, yd, ltd, idxd)
            loss2, gs2, bad2 = ops.temp_nll(xd, yd, ltd, idxd)
            assert torch.equal(loss, loss2) and torch.equal(gs, gs2) and int(bad.item()) == int(bad2.item()) == 0      # the same bits
            want_loss, want_g = rs.nll(x, y, lt, idx)
            el, eg = abs(float(loss.item()) - want_loss), abs(float(gs.item()) - want_g)
            bl, bg = 4.0 * float(g["err_loss"][i, j, k, v]), 4.0 * float(g["err_g"][i, j, k, v])
            print(f"N={n} C={c} log_T={float(lt):+.4f} {variant}: loss {want_loss:.9e} err {el:.2e} bar {bl:.2e}; g {want_g:+.9e} err {eg:.2e} bar {bg:.2e}")
            worst = max(worst, el / bl if bl else 0.0, eg / bg if bg else 0.0)
            assert el <= bl and eg <= bg, (float(lt), variant, el, bl, eg, bg)
            if k == 0:                                             # under the clamp: g == 0 exactly, the loss is the one at T = 1e-3
                assert float(gs.item()) == 0.0
                at = rs.nll(x, y, np.log(np.float64(np.float32(1e-3))), idx, False)[0]
                assert abs(float(loss.item()) - at) <= 1e-12 * max(at, 1.0)
    print(f"N={n} C={c}: largest error / bar {worst:.3g}")


def test_temp_nll_counts_bad_labels_and_indices(cuda, nll_golden):
    x, y = rs.nll_case(nll_golden["rows"], nll_golden["labels"], 257, 20)
    y = y.copy()
    y[[0, 100, 256]] = [20, -1, 255]
    good = np.ones(257, dtype=bool)
    good[[0, 100, 256]] = False
    lt = np.float32(np.log(6.3))
    xd, yd, ltd = _t(x).to(cuda), _t(y).to(cuda), torch.tensor([float(lt)], device=cuda)
    loss, gs, bad = ops.temp_nll(xd, yd, ltd)
    want = rs.nll(x[good], y[good], lt)
    assert int(bad.item()) == 3                                    # they contribute nothing
    assert abs(float(loss.item()) - want[0]) <= 1e-9 * abs(want[0]) and abs(float(gs.item()) - want[1]) <= 1e-9 * np.abs(rs.nll_terms(x[good], y[good], lt)[1]).sum()
    idx = np.array([5, 257, -1, 6, 1 << 40, 0], dtype=np.int64)   # outside [0, N): counted, never read; row 0 carries a bad label
    loss, gs, bad = ops.temp_nll(xd, yd, ltd, _t(idx).to(cuda))
    want = rs.nll(x, y, lt, np.array([5, 6]))
    assert int(bad.item()) == 4 and abs(float(loss.item()) - want[0]) <= 1e-9 * abs(want[0])
    for opt in ("lbfgs", "adam"):
        with pytest.raises(ValueError, match="outside"):
            ts.calibrate_temperature_from_cache(xd, yd, cuda, optimizer_type=opt)


def test_autograd_node_and_chunking(cuda, nll_golden):
    x, y = rs.nll_case(nll_golden["rows"], nll_golden["labels"], 4099, 20)
    xd, yd = _t(x).to(cuda), _t(y).to(cuda)
    want = rs.nll(x, y, np.float32(0.5))
    for dtype in (torch.float32, torch.float64):
        for chunk in (None, 4099, 1000, 64):
            log_t = torch.full((1,), 0.5, dtype=dtype, device=cuda, requires_grad=True)
            loss, bad = temp_nll_loss(log_t, xd, yd, None, 4099, chunk)
            loss.backward()
            assert loss.dtype == torch.float64 and log_t.grad.dtype == dtype and log_t.grad.shape == (1,) and not bad.requires_grad
            assert abs(float(loss.item()) - want[0] / 4099) <= 1e-12 * want[0] and abs(float(log_t.grad.item()) - want[1] / 4099) <= 1e-6 * abs(want[1] / 4099)
    idx = rs.nll_index("repeated", 4099)
    log_t = torch.full((1,), 0.5, dtype=torch.float64, device=cuda, requires_grad=True)
    loss, _ = temp_nll_loss(log_t, xd, yd, _t(idx).to(cuda), None, 1000)
    (2.0 * loss).backward()
    want = rs.nll(x, y, np.float32(0.5), idx)
    assert abs(float(loss.item()) - want[0] / idx.size) <= 1e-12 * want[0] and abs(float(log_t.grad.item()) - 2.0 * want[1] / idx.size) <= 1e-9 * abs(want[1] / idx.size)


@pytest.fixture(scope="module")
def fit_golden():
    return golden("temp_scaling_fit")


@pytest.mark.parametrize("where", ("device", "cpu"))
def test_lbfgs_fit_finds_the_fp64_minimiser(cuda, fit_golden, where, tmp_path):
    """Observed: printed |T - T64| and the bar."""
    g = fit_golden
    t64 = float(g["T64"])
    bar = 4.0 * float(np.abs(g["T_ref32"] - t64).max())
    rows, labels = _t(g["rows"]), _t(g["labels"])
    if where == "device":
        rows, labels = rows.to(cuda), labels.to(cuda)
    for chunk in (1_000_000, 700):
        path = tmp_path / f"T_{chunk}.json"
        t = ts.calibrate_temperature_from_cache(rows, labels, cuda, chunk_size=chunk, save_path=str(path))
        print(f"{where} cache, chunk {chunk}: T {t:.9f} T64 {t64:.9f} |T - T64| {abs(t - t64):.3e} bar {bar:.3e}")
        assert abs(t - t64) <= bar
        assert __import__("json").load(open(path)) == {"temperature": t}
    # other start values: LBFGS ends a run once the mean loss changes by less than tolerance_change = 1e-12, i.e. within
    # sqrt(2e-12 / h) of the minimiser in log T (h: the curvature of the mean loss there) -- 6.4e-6 in T here, whatever the arithmetic
    eps = 1e-4
    h = (rs.nll(g["rows"], g["labels"], np.log(t64) + eps, None, False)[1] - rs.nll(g["rows"], g["labels"], np.log(t64) - eps, None, False)[1]) / (2 * eps) / 3000
    reach = t64 * float(np.sqrt(2e-12 / h))
    for kw in ({"init_T": "auto", "prev_T": 4.0}, {"init_T": 9.0}):
        t = ts.calibrate_temperature_from_cache(rows, labels.int(), cuda, **kw)
        print(f"{where} cache, {kw}: |T - T64| {abs(t - t64):.3e} reach {reach:.3e}")
        assert abs(t - t64) <= reach


def test_adam_fit_follows_the_restatement(cuda, fit_golden):
    """Observed: printed |T - restatement| and the bar."""
    g = fit_golden
    want = float(g["adam:T_restatement"])
    bar = 4.0 * abs(float(g["adam:T_ref32"]) - want)
    for where in ("device", "cpu"):
        rows, labels = _t(g["rows"]), _t(g["labels"])
        if where == "device":
            rows, labels = rows.to(cuda), labels.to(cuda)
        torch.manual_seed(int(g["adam:seed"]))
        t = ts.calibrate_temperature_from_cache(rows, labels, cuda, optimizer_type="adam", lr=float(g["adam:lr"]), epochs=int(g["adam:epochs"]),
                                                chunk_size=int(g["adam:chunk"]))
        print(f"{where} cache: T {t:.10f} restatement {want:.10f} |difference| {abs(t - want):.3e} bar {bar:.3e}")
        assert abs(t - want) <= bar


class _Replay(torch.nn.Module):
    """Returns its stored outputs one after the other; `drop` is a dropout layer in front of a copy, for the MC mode."""

    def __init__(self, outs, p=0.0):
        super().__init__()
        self.outs, self.at = outs, 0
        self.drop = torch.nn.Dropout2d(p)

    def forward(self, x):
        out = self.outs[self.at % len(self.outs)]
        self.at += 1
        reps = x.shape[0] // out.shape[0]                         # stacked MC passes
        return self.drop(out.repeat(reps, 1, 1, 1)) if self.drop.p else out.repeat(reps, 1, 1, 1)


def _loader(labels, h, w):
    z = torch.zeros(labels[0].shape[0], 1, h, w)
    return [(z, z, z.repeat(1, 3, 1, 1), z.repeat(1, 3, 1, 1), lab) for lab in labels]


def _ece(rows, labels, t):
    agg = ECEAggregator(n_bins=15, mode="logits")
    n, c = rows.shape
    agg.update((rows / t).t().reshape(1, c, 1, n).contiguous(), labels.reshape(1, 1, n))
    return agg.compute()[0][0]


def test_end_to_end_cache_fit_and_ece(cuda):
    gen = torch.Generator().manual_seed(11)
    b, c, h, w = 2, 20, 4, 96
    labels, logits = [], []
    for k in range(3):
        lab = torch.randint(0, c, (b, h, w), generator=gen)
        hit = torch.where(torch.rand(b, h, w, generator=gen) < 0.3, torch.randint(0, c, (b, h, w), generator=gen), lab)
        z = torch.randn(b, c, h, w, generator=gen)
        z.scatter_add_(1, hit[:, None], torch.full((b, 1, h, w), 2.0))
        lab[torch.rand(b, h, w, generator=gen) < 0.1] = 255
        labels.append(lab[:, None] if k == 0 else lab)             # [B,1,H,W] is accepted like [B,H,W]
        logits.append((z * 5.0).to(cuda))                         # over-confident
    labels[1][:] = 255                                            # an all-ignored batch contributes nothing
    torch.manual_seed(0)
    rows, row_labels = ts.cache_calib_logits(_Replay(logits), _loader(labels, h, w), cuda, CFG)
    assert rows.is_cuda and row_labels.is_cuda and rows.dtype == torch.float32 and row_labels.dtype == torch.int64
    want = [rs.cache_rows(z.cpu().numpy(), "logits", l.reshape(b, h, w).numpy(), 255) for z, l in zip(logits, labels)]
    want_rows, want_lab = np.concatenate([r for r, _ in want]), np.concatenate([l for _, l in want])
    assert want[1][1].size == 0 and np.array_equal(row_labels.cpu().numpy(), want_lab)
    assert rs.ulp_distance(rows.cpu().numpy(), want_rows) <= 2
    torch.manual_seed(0)
    rows_cpu, labels_cpu = ts.cache_calib_logits(_Replay(logits), _loader(labels, h, w), cuda, CFG, keep_on_device=False)
    assert not rows_cpu.is_cuda and not labels_cpu.is_cuda and torch.equal(rows_cpu, rows.cpu()) and torch.equal(labels_cpu, row_labels.cpu())
    t = ts.calibrate_temperature_from_cache(rows, row_labels, cuda)
    t64 = rs.minimiser(want_rows, want_lab)
    before, after = _ece(rows, row_labels, 1.0), _ece(rows, row_labels, t)
    print(f"T {t:.6f} (fp64 minimiser {t64:.6f}); ECE {before:.4f} at T = 1, {after:.4f} at T")
    assert abs(t - t64) <= 1e-5 * t64 and t > 1.5
    assert after <= before
    with pytest.raises(ValueError, match="No valid pixels found in calibration loader."):
        ts.cache_calib_logits(_Replay(logits), _loader([torch.full((b, h, w), 255)] * 2, h, w), cuda, CFG)
    # MC mode: without active dropout the mean of the passes is the single pass
    torch.manual_seed(0)
    rows_mc, labels_mc = ts.cache_calib_logits(_Replay(logits), _loader(labels, h, w), cuda, CFG, mode="mc", mc_samples=5)
    assert torch.equal(labels_mc, row_labels) and float((rows_mc.exp() - rows.exp()).abs().max()) <= 1e-6
    model = _Replay([z.softmax(1) for z in logits], p=0.5)        # probabilities, whole maps dropped (and the rest doubled) per pass
    torch.manual_seed(0)
    rows_mc, labels_mc = ts.cache_calib_logits(model, _loader(labels, h, w), cuda, CFG, mode="mc", mc_samples=18)
    assert not model.drop.training and torch.equal(labels_mc, row_labels)
    assert bool(torch.isfinite(rows_mc).all()) and float(rows_mc.max()) <= float(np.log(2.0)) + 1e-6 and float(rows_mc.min()) >= -27.64
