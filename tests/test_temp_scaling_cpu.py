"""CPU: the yardstick of the temperature-scaling tests and the host rules of models/temp_scaling.py.

The fp64 restatement (tests/temp_scaling_restatement.py) that the GPU tests hold the kernels to is pinned here to the reference's own
results (tests/golden/temp_scaling_*.npz, written by tools/gen_golden_temp_scaling.py from the reference's models/temp_scaling.py).

Cache rows.  Order and labels are exactly the reference's.  The values are the logarithm of fp32 probabilities, and log p near 0
magnifies every ulp of p: from the same model output the reference's own fp32 softmax (exp) leaves its rows up to 2052 (1025) ulp
from the restatement's for logits (log-probs), 4 (2) ulp where |row| >= 0.5, while its probabilities are within 0.43 (0.65) of what
fp32 arithmetic allows them.  So the pin has two parts, and each holds at the bar it can be held to: given the reference's own
fp32 probabilities (stored in the fixture) the rows are reproduced within 1 ulp -- observed: 0 -- for every kind, which for the
probabilities kind is the whole path; and the restatement's probabilities agree with the reference's within the fp32 error bound of
the formula (temp_scaling_restatement.prob_excess)."""
import json
import os

import numpy as np
import pytest
import torch

import temp_scaling_restatement as rs
from conftest import golden
from semanticlidarunc_amd import _lib, ops
from semanticlidarunc_amd.models import temp_scaling as ts

KINDS = ("logits", "probs", "log_probs")


def test_restatement_reproduces_the_reference_cache_rows():
    g = golden("temp_scaling_rows")
    labels = [g["labels0"], g["labels1"]]
    assert (labels[1][1] == 255).all() and 0 < (labels[0] == 255).sum() < labels[0].size
    assert (g["probs:out0"] == 0).sum() >= 30 and ((g["probs:out0"] > 0) & (g["probs:out0"] < 1e-12)).sum() >= 30
    for kind in KINDS:
        rows, lab = [], []
        for k in range(2):
            r, l = rs.rows_from_probs(g[f"{kind}:ref_probs{k}"], labels[k], 255)
            e2e, l2 = rs.cache_rows(g[f"{kind}:out{k}"], kind, labels[k], 255)
            assert np.array_equal(l, l2) and e2e.shape == r.shape
            assert rs.prob_excess(g[f"{kind}:out{k}"], kind, g[f"{kind}:ref_probs{k}"]) <= 1.0
            rows.append(r)
            lab.append(l)
        rows, lab = np.concatenate(rows), np.concatenate(lab)
        assert np.array_equal(lab, g[f"{kind}:labels"]), kind                     # order and labels: exact
        assert rows.shape == g[f"{kind}:rows"].shape
        d = rs.ulp_distance(rows, g[f"{kind}:rows"])
        print(f"{kind}: {rows.shape[0]} rows, {d} ulp")
        assert d <= 1, (kind, d)
    # the clamp: exact zeros and values below 1e-12 give log(fp32(1e-12))
    assert np.float32(np.log(np.float64(np.float32(1e-12)))) == g["probs:rows"].min() == np.float32(-27.631021)


def test_restatement_reproduces_the_fp64_minimiser_and_the_adam_loop():
    g = golden("temp_scaling_fit")
    t64 = float(g["T64"])
    assert abs(rs.minimiser(g["rows"], g["labels"]) - t64) <= 1e-9
    assert abs(rs.nll(g["rows"], g["labels"], np.log(t64), None, False)[1]) <= 1e-8 * np.abs(rs.nll_terms(g["rows"], g["labels"], np.log(t64))[1]).sum()
    spread = np.abs(g["T_ref32"] - t64).max()
    assert 0 < spread <= 1e-4 * t64 and tuple(g["chunks"]) == (64, 700, 1000, 3000)
    torch.manual_seed(int(g["adam:seed"]))
    perms = np.stack([torch.randperm(3000).numpy() for _ in range(int(g["adam:epochs"]))])
    assert np.array_equal(perms, g["adam:perms"])                                 # the reference's permutations are redrawn under the seed
    ta = rs.adam_fit(g["rows"], g["labels"], perms, int(g["adam:chunk"]), lr=float(g["adam:lr"]))
    assert abs(ta - float(g["adam:T_restatement"])) <= 1e-12
    assert 0 < abs(float(g["adam:T_ref32"]) - ta) <= 1e-6


def test_restatement_objective_by_hand():
    rows = np.log(np.array([[0.5, 0.25, 0.25], [0.1, 0.8, 0.1]], dtype=np.float32))
    loss, g = rs.nll(rows, [0, 2], np.float32(0.0))
    assert abs(loss - (-np.log(0.5) - np.log(0.1))) <= 1e-6                      # T = 1: -log p_y of normalised rows
    eps = 1e-6
    up, down = rs.nll(rows, [0, 2], eps, None, False)[0], rs.nll(rows, [0, 2], -eps, None, False)[0]
    assert abs((up - down) / (2 * eps) - g) <= 1e-6                               # g is d loss / d log T
    lc, gc = rs.nll(rows, [0, 2], np.float32(np.log(1e-4)))
    assert gc == 0.0 and abs(lc - rs.nll(rows, [0, 2], np.log(np.float64(np.float32(1e-3))), None, False)[0]) <= 1e-9 * lc
    assert rs.nll(rows, [0, 2], 0.3, np.array([1, 1, 0]))[0] == pytest.approx(sum(rs.nll_terms(rows, [0, 2], 0.3)[0][[1, 1, 0]]))


def test_nll_fixture_matches_the_case_table():
    g = golden("temp_scaling_nll")
    assert g["rows"].shape == (4099, 32) and g["rows"].dtype == np.float32 and g["labels"].shape == (4099,)
    assert tuple(g["ns"]) == rs.NLL_NS and tuple(g["cs"]) == rs.NLL_CS and np.array_equal(g["log_T"], np.asarray(rs.NLL_LOG_TS))
    assert g["rows"].min() == np.float32(-27.631021) and (g["rows"] == g["rows"].min()).mean() > 0.01
    shape = (len(rs.NLL_NS), len(rs.NLL_CS), len(rs.NLL_LOG_TS), len(rs.NLL_VARIANTS))
    assert g["err_loss"].shape == shape == g["err_g"].shape
    assert (g["err_g"][:, :, 0] == 0).all() and (g["err_g"][:, 1:, 1:] > 0).all()          # clamped: g = 0 exactly; else the reference errs
    idx = rs.nll_index("repeated", 65)
    assert idx.shape == (72,) and np.unique(idx).size < 65 and np.array_equal(rs.nll_index("reversed", 3), [2, 1, 0])


def test_start_value_rule_and_json_file(tmp_path):
    assert ts._start_temperature("auto", None) == 1.0
    assert ts._start_temperature("auto", 2.5) == 2.5
    assert ts._start_temperature(3, 2.5) == 3.0 and ts._start_temperature("0.5", None) == 0.5
    path = tmp_path / "sub" / "dir" / "T.json"
    ts._save_temperature(str(path), 1.75)
    assert json.load(open(path)) == {"temperature": 1.75}
    ts._save_temperature(None, 1.0)
    import inspect
    sig = inspect.signature(ts.calibrate_temperature_from_cache)
    assert [(k, v.default) for k, v in sig.parameters.items()][3:] == [
        ("init_T", "auto"), ("optimizer_type", "lbfgs"), ("lr", 0.05), ("epochs", 2), ("chunk_size", 1_000_000), ("max_iter_lbfgs", 100),
        ("prev_T", None), ("save_path", None)]
    sig = inspect.signature(ts.cache_calib_logits)
    assert [(k, v.default) for k, v in sig.parameters.items()][4:] == [("ignore_index", 255), ("mode", "default"), ("mc_samples", 30),
                                                                      ("keep_on_device", True)]
    assert sig.parameters["keep_on_device"].kind is inspect.Parameter.KEYWORD_ONLY


def test_empty_loader_raises_the_reference_error():
    with pytest.raises(ValueError, match="No valid pixels found in calibration loader."):
        ts.cache_calib_logits(torch.nn.Identity(), [], "cpu", {"model_settings": {"baseline": "SalsaNext"}})


def test_wrappers_reject_cpu_tensors():
    rows, lab, cnt = torch.zeros(8, 3), torch.zeros(8, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.calib_rows(torch.zeros(1, 3, 2, 4), "logits", torch.zeros(1, 2, 4, dtype=torch.int64), 255, rows, lab, cnt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.temp_nll(rows, lab, torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.calibrate_temperature_from_cache(rows, lab, "cpu")


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 43 and lib.slu_abi_version() == _lib.ABI_VERSION
    p = 4096                                                   # a non-null address that is never dereferenced: every call below is refused
    ok_rows = (p, 0, p, 2, 20, 64, 1, 255, p, p, 128, p, p, 1 << 20, None)
    assert lib.slu_calib_rows(*ok_rows[:3], 2, 33, *ok_rows[5:]) == -2                       # C > 32
    assert lib.slu_calib_rows(*ok_rows[:3], 1 << 16, 20, 1 << 15, *ok_rows[6:]) == -2        # B HW = 2^31
    for i in (0, 2, 8, 9, 11, 12):                             # each pointer
        a = list(ok_rows)
        a[i] = None
        assert lib.slu_calib_rows(*a) == -1, i
    for i, v in ((1, 3), (1, -1), (3, 0), (4, 0), (5, 0), (10, 0), (13, 8)):                 # kind, B, C, HW, cap, a short workspace
        a = list(ok_rows)
        a[i] = v
        assert lib.slu_calib_rows(*a) == -1, (i, v)
    assert lib.slu_calib_rows_workspace_bytes(2, 64) >= 256 + 4 and lib.slu_calib_rows_workspace_bytes(0, 64) == 0
    ok_nll = (p, p, 100, 20, None, 0, p, p, p, p, p, 1 << 20, None)
    a = list(ok_nll)
    a[3] = 33
    assert lib.slu_temp_nll(*a) == -2
    for i in (0, 1, 6, 7, 8, 9, 10):
        a = list(ok_nll)
        a[i] = None
        assert lib.slu_temp_nll(*a) == -1, i
    for i, v in ((2, 0), (3, 0), (11, 8)):
        a = list(ok_nll)
        a[i] = v
        assert lib.slu_temp_nll(*a) == -1, (i, v)
    a = list(ok_nll)
    a[4], a[5] = p, 0                                          # an index without entries
    assert lib.slu_temp_nll(*a) == -1
    assert lib.slu_temp_nll_workspace_bytes(1) > 0 and lib.slu_temp_nll_workspace_bytes(0) == 0


def test_drop_in_import_path_resolves_here_and_reexports_the_rest(tmp_path):
    """With the package directory ahead of a reference-like tree on sys.path, `models.temp_scaling` is this mirror, and a name it does
    not define comes from the shadowed file (hermetic: the other tree is written to tmp_path)."""
    import subprocess
    import sys
    import textwrap
    from conftest import ROOT
    src = tmp_path / "src"
    (src / "models").mkdir(parents=True)
    (src / "models" / "temp_scaling.py").write_text(textwrap.dedent("""
        def cache_calib_logits(*a, **k):
            return 'shadowed: must NOT win over the mirror'
        def only_in_reference():
            return 'reference helper'
    """))
    code = textwrap.dedent("""
        from models.temp_scaling import cache_calib_logits, calibrate_temperature_from_cache, only_in_reference
        import models.temp_scaling as m
        assert 'semanticlidarunc_amd' in m.__file__ and only_in_reference() == 'reference helper'
        try:
            cache_calib_logits(None, [], 'cpu', {})
        except AttributeError:
            pass                                              # the mirror ran: model.eval() on None
        else:
            raise AssertionError('the shadowed function answered')
        print('ok')
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "semanticlidarunc_amd"), str(src)]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
