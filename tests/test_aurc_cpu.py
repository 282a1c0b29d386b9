"""CPU: the yardstick of the AURC tests and the host side of the reservoir.

The fp64 restatement (tests/aurc_restatement.py) that the GPU tests compare the kernels with is pinned here to the reference's
own results (tests/golden/aurc_2x20x16x64.npz, written by tools/gen_golden_aurc.py from the reference's metrics/aurc.py): fed the
reference's flattened samples it reproduces every golden AURC / EAURC / recall to 1e-12.  The reference forms a recall as the
fp32 quotient of two exactly represented counts, so the restatement's exact numerators, divided the same way, must reproduce the
stored value; the fp64 quotient that the device reports then differs from it by the fp32 rounding alone (2^-24 relative)."""
import numpy as np
import torch

from aurc_restatement import KS, restate
from conftest import golden
from semanticlidarunc_amd._reservoir import MergedReservoir

FORMS = ("maxprob", "entropy", "ent_mc")


def _check(g, tag, want_recalls):
    r = restate(g[tag + ":confids"], g[tag + ":risks"])
    assert abs(r["AURC"] - float(g[tag + ":AURC"])) <= 1e-12, (tag, r["AURC"], float(g[tag + ":AURC"]))
    assert abs(r["EAURC"] - float(g[tag + ":EAURC"])) <= 1e-12, (tag, r["EAURC"], float(g[tag + ":EAURC"]))
    assert r["E"] == int(g[tag + ":risks"].sum())
    if want_recalls:
        ref = g[tag + ":recalls"]
        den = max(r["E"], 1)
        as_ref = np.array([float(np.float32(num) / np.float32(den)) for num in r["recall_num"]])
        assert np.abs(as_ref - ref).max() <= 1e-12, (tag, as_ref, ref)
        assert np.abs(np.array(r["recall_num"]) / den - ref).max() <= 2.0 ** -24
        # number of curve points: point 0, the m group starts, the tail
        n = g[tag + ":confids"].size
        assert 1 + r["m"] + (1 if r["m"] and n - 2 - r["s_m"] > 0 else 0) == int(g[tag + ":npoints"])
        assert r["E"] == int(g[tag + ":num_errors"]) and n == int(g[tag + ":num_pixels"])
    return r


def test_restatement_reproduces_the_reference():
    g = golden("aurc_2x20x16x64")
    assert tuple(g["ks"]) == KS
    for form in FORMS:
        _check(g, "batch:" + form, True)
        _check(g, "agg:" + form, False)           # every confidence twice, both with the same risk: order-free
    r = restate(g["res:kept_confids"], g["res:kept_risks"])
    assert abs(r["AURC"] - float(g["res:AURC"])) <= 1e-12 and abs(r["EAURC"] - float(g["res:EAURC"])) <= 1e-12


def test_restatement_small_cases_by_hand():
    # n = 1: no point but point 0, AURC = 0; AURC_opt = E/n
    r = restate([0.3], [1])
    assert (r["AURC"], r["AURC_opt"], r["m"], r["s_m"]) == (0.0, 1.0, 0, -1)
    # n = 3, all equal: one group start at 0, then the tail:  (R0 + R1)/2 * 1/3 + R1 * 1/3 with R0 = 2/3, R1 = (2 - e_0)/2
    r = restate([0.5, 0.5, 0.5], [1, 0, 1])          # stable: the first sample (an error) leads the group
    assert (r["m"], r["s_m"]) == (1, 0) and abs(r["AURC"] - ((2 / 3 + 0.5) / 2 / 3 + 0.5 / 3)) <= 1e-15
    assert np.allclose(r["cov"], [1.0, 2 / 3]) and np.allclose(r["risk"], [2 / 3, 0.5])
    # -0.0 and +0.0 are one group
    assert restate([0.0, -0.0, 0.0, 1.0], [0, 1, 0, 1])["m"] == 1


def test_merged_reservoir_reproduces_the_reference_kept_set():
    g = golden("aurc_2x20x16x64")
    probs, labs, ent = torch.from_numpy(g["probs"]), torch.from_numpy(g["labels"]), torch.from_numpy(g["ent_mc"])
    valid = labs != 255
    err = ((probs.argmax(1) != labs) & valid)[valid].to(torch.uint8)
    buf = MergedReservoir(1500, seed=0)
    for k in range(3):
        buf.push((1.0 - ent[k].clamp(0, 1))[valid], err)
    conf, risk = buf.materialize()
    assert len(buf) == 1500
    assert np.array_equal(conf.numpy(), g["res:kept_confids"]) and np.array_equal(risk.numpy(), g["res:kept_risks"])
    # without a size everything is kept, in order
    buf = MergedReservoir(None)
    buf.push(err[:5].float(), err[:5])
    buf.push(err[5:9].float(), err[5:9])
    assert len(buf) == 9 and torch.equal(buf.materialize()[1], err[:9])
    # the first chunk alone already exceeds the size: it is down-sampled by the same draw
    buf, rng = MergedReservoir(4, seed=3), np.random.RandomState(3)
    buf.push(torch.arange(10.0), torch.arange(10, dtype=torch.uint8))
    assert np.array_equal(buf.materialize()[0].numpy(), np.arange(10.0)[rng.choice(10, size=4, replace=False)])
