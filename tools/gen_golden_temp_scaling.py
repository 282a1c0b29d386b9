#!/usr/bin/env python
"""(Re)generate tests/golden/temp_scaling_{rows,fit,nll}.npz from the reference's models/temp_scaling.py.

Runs ONLY in the build container (needs /root/reference; CPU is enough).  It imports the reference's module read-only, asserts that
the fp64 restatement (tests/temp_scaling_restatement.py) agrees with it and stores data only:

  temp_scaling_rows   two batches of model outputs in the three output kinds (probabilities with exact zeros and values below 1e-12),
                      labels with ignored pixels, and the reference's cache rows / labels for each kind
  temp_scaling_fit    N = 3000 over-confident cache rows (2 % of the entries at the 1e-12 clamp); T64, the fp64 minimiser by bisection on
                      the sign of g; the reference's fp32 CPU LBFGS result at chunk sizes 64 / 700 / 1000 / N; its Adam result for the
                      permutations it drew under a stored seed, and the restatement's for the same permutations
  temp_scaling_nll    [4099, 32] rows (with -27.631 entries) the objective's test cases are cut from, and per case the error of the
                      reference's own fp32 CPU evaluation (CrossEntropyLoss(reduction="sum") on x / T and its autograd gradient) against
                      the restatement on the same data

    python tools/gen_golden_temp_scaling.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(1, REF)

import temp_scaling_restatement as rs      # noqa: E402
from models import temp_scaling as ref     # noqa: E402  (reference)

OUT = os.path.join(ROOT, "tests", "golden")
CFG = {"model_settings": {"baseline": "SalsaNext", "reflectivity": 0, "normals": 0}}
KINDS = ("logits", "probs", "log_probs")
FIT_CHUNKS = (64, 700, 1000, 3000)
ADAM = {"seed": 1234, "chunk": 700, "epochs": 2, "lr": 0.05}


class Replay(torch.nn.Module):
    """Returns the stored outputs one after the other, whatever it is fed."""

    def __init__(self, outs):
        super().__init__()
        self.outs, self.at = outs, 0

    def forward(self, x):
        out = self.outs[self.at % len(self.outs)]
        self.at += 1
        return out


def loader(labels, h, w):
    z = torch.zeros(labels[0].shape[0], 1, h, w)
    return [(z, z, z.repeat(1, 3, 1, 1), z.repeat(1, 3, 1, 1), lab) for lab in labels]


def rows_fixture():
    g = torch.Generator().manual_seed(20)
    b, c, h, w = 2, 20, 3, 67
    out = {}
    logits, labels = [], []
    for k in range(2):
        lab = torch.randint(0, c, (b, h, w), generator=g)
        z = torch.randn(b, c, h, w, generator=g) * 3.0
        z.scatter_add_(1, lab[:, None], torch.full((b, 1, h, w), 4.0))
        lab[torch.rand(b, h, w, generator=g) < 0.2] = 255
        logits.append(z)
        labels.append(lab)
    labels[1][1] = 255                                     # a whole image ignored
    probs = [z.softmax(1) for z in logits]
    for p in probs:                                        # exact zeros and values below the clamp, put where p < 1e-4: the sums stay 1
        flat = p.view(-1)
        small = torch.nonzero(flat < 1e-4).view(-1)
        pick = small[torch.randperm(small.numel(), generator=g)[:120]]
        flat[pick[:60]] = 0.0
        flat[pick[60:]] = torch.rand(60, generator=g) * 1e-13
    logp = [z.log_softmax(1) for z in logits]
    model_out = {"logits": logits, "probs": probs, "log_probs": logp}
    for kind in KINDS:
        torch.manual_seed(0)
        rows, lab = ref.cache_calib_logits(Replay(model_out[kind]), loader(labels, h, w), "cpu", CFG, ignore_index=255)
        # the reference's own fp32 probabilities: the rows are their logarithm
        ref_p = [ref._forward_to_probs(Replay([o]), [o], None) for o in model_out[kind]]
        assert all(k == kind for _, k in ref_p), (kind, [k for _, k in ref_p])
        want_rows, want_lab, end_to_end = [], [], []
        for o, y, (p, _) in zip(model_out[kind], labels, ref_p):
            r, l = rs.rows_from_probs(p.numpy(), y.numpy(), 255)
            want_rows.append(r)
            want_lab.append(l)
            end_to_end.append(rs.cache_rows(o.numpy(), kind, y.numpy(), 255)[0])
            excess = rs.prob_excess(o.numpy(), kind, p.numpy())
            assert excess <= 1.0, (kind, excess)
        want_rows, want_lab = np.concatenate(want_rows), np.concatenate(want_lab)
        assert np.array_equal(lab.numpy(), want_lab), kind
        d = rs.ulp_distance(rows.numpy(), want_rows)
        e2e = np.concatenate(end_to_end)
        far = np.abs(e2e) >= 0.5
        print(f"rows[{kind}]: {rows.shape[0]} rows; from the reference's probabilities the restatement is within {d} ulp of the reference; "
              f"from the model output {rs.ulp_distance(rows.numpy(), e2e)} ulp ({rs.ulp_distance(rows.numpy()[far], e2e[far])} ulp where |row| >= 0.5); "
              f"probabilities at {excess:.2f} of their bound")
        assert d <= 1, (kind, d)
        for k in range(2):
            out[f"{kind}:out{k}"] = model_out[kind][k].numpy()
            out[f"{kind}:ref_probs{k}"] = ref_p[k][0].numpy()
        out[f"{kind}:rows"], out[f"{kind}:labels"] = rows.numpy(), lab.numpy()
    for k in range(2):
        out[f"labels{k}"] = labels[k].numpy()
    return out


def confident_rows(n, c, seed, scale=6.0, wrong=0.25, clamp_fraction=0.02):
    """log(clamp(p, 1e-12)) rows of an over-confident classifier that is wrong on `wrong` of the rows."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, c, (n,), generator=g)
    z = torch.randn(n, c, generator=g)
    hit = torch.where(torch.rand(n, generator=g) < wrong, torch.randint(0, c, (n,), generator=g), y)
    z.scatter_add_(1, hit[:, None], torch.full((n, 1), 2.0))
    p = (z * scale).softmax(1)
    p.view(-1)[torch.randperm(n * c, generator=g)[: int(clamp_fraction * n * c)]] = 0.0
    return p.clamp_min(1e-12).log().numpy(), y.numpy()


def fit_fixture():
    rows, y = confident_rows(3000, 20, seed=7)
    out = {"rows": rows, "labels": y, "chunks": np.asarray(FIT_CHUNKS)}
    t64 = rs.minimiser(rows, y)
    again = rs.minimiser(rows, y, lo=np.log(0.5), hi=np.log(200.0))
    assert abs(t64 - again) <= 1e-9 * t64, (t64, again)
    out["T64"] = np.float64(t64)
    tr, ty = torch.from_numpy(rows), torch.from_numpy(y)
    t32 = [ref.calibrate_temperature_from_cache(tr, ty, "cpu", chunk_size=ch) for ch in FIT_CHUNKS]
    out["T_ref32"] = np.asarray(t32, dtype=np.float64)
    print(f"fit: T64 {t64:.9f}; reference fp32 LBFGS, relative deviation at chunks {FIT_CHUNKS}: " +
          " ".join(f"{abs(t - t64) / t64:.1e}" for t in t32))
    assert max(abs(t - t64) for t in t32) <= 1e-3 * t64
    torch.manual_seed(ADAM["seed"])
    perms = np.stack([torch.randperm(3000).numpy() for _ in range(ADAM["epochs"])])
    torch.manual_seed(ADAM["seed"])
    ta = ref.calibrate_temperature_from_cache(tr, ty, "cpu", optimizer_type="adam", lr=ADAM["lr"], epochs=ADAM["epochs"], chunk_size=ADAM["chunk"])
    tb = rs.adam_fit(rows, y, perms, ADAM["chunk"], lr=ADAM["lr"])
    print(f"fit: Adam reference {ta:.9f}, restatement {tb:.9f}, |difference| {abs(ta - tb):.2e}")
    assert abs(ta - tb) <= 1e-4 * tb
    out.update({"adam:seed": np.int64(ADAM["seed"]), "adam:chunk": np.int64(ADAM["chunk"]), "adam:epochs": np.int64(ADAM["epochs"]),
                "adam:lr": np.float64(ADAM["lr"]), "adam:perms": perms, "adam:T_ref32": np.float64(ta), "adam:T_restatement": np.float64(tb)})
    return out


def reference_nll(rows, y, log_t, idx):
    """(loss_sum, g_sum) of the reference's objective in its own arithmetic: fp32 on the CPU, gradient by autograd."""
    x, lab = torch.from_numpy(rows), torch.from_numpy(y)
    if idx is not None:
        x, lab = x[torch.from_numpy(idx)], lab[torch.from_numpy(idx)]
    lt = torch.nn.Parameter(torch.tensor([float(log_t)], dtype=torch.float32))
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(x / lt.exp().clamp_min(1e-3), lab)
    loss.backward()
    return float(loss.item()), float(lt.grad.item())


def nll_fixture():
    rows, y = confident_rows(4099, 32, seed=11)
    assert np.isclose(rows.min(), np.log(np.float32(1e-12)))
    shape = (len(rs.NLL_NS), len(rs.NLL_CS), len(rs.NLL_LOG_TS), len(rs.NLL_VARIANTS))
    err_loss, err_g = np.zeros(shape), np.zeros(shape)
    for i, n in enumerate(rs.NLL_NS):
        for j, c in enumerate(rs.NLL_CS):
            x, lab = rs.nll_case(rows, y, n, c)
            for k, lt in enumerate(rs.NLL_LOG_TS):
                for v, variant in enumerate(rs.NLL_VARIANTS):
                    idx = rs.nll_index(variant, n)
                    got = reference_nll(x, lab, lt, idx)
                    want = rs.nll(x, lab, lt, idx)
                    err_loss[i, j, k, v], err_g[i, j, k, v] = abs(got[0] - want[0]), abs(got[1] - want[1])
    print(f"nll: reference fp32 error, largest {err_loss.max():.3e} (loss) {err_g.max():.3e} (g); cases with error 0: "
          f"{int((err_loss == 0).sum())} (loss) {int((err_g == 0).sum())} (g) of {err_loss.size}")
    return {"rows": rows, "labels": y.astype(np.int64), "log_T": np.asarray(rs.NLL_LOG_TS, dtype=np.float32), "ns": np.asarray(rs.NLL_NS),
            "cs": np.asarray(rs.NLL_CS), "err_loss": err_loss, "err_g": err_g}


def main():
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    for name, build in (("rows", rows_fixture), ("fit", fit_fixture), ("nll", nll_fixture)):
        path = os.path.join(OUT, f"temp_scaling_{name}.npz")
        np.savez_compressed(path, **build())
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
