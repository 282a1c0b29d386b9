"""GPU: gemm1x1_h8_kernel's epilogue with the residual loaded ahead (gemm1x1_h8.hip): whole 16-byte residual records from untracked loads,
the first two M-blocks issued before the last chunk's staging burst and retired by a counted wait, the rest issued at the top of the epilogue.

Reference and bar are those of test_gpu_h8._conv_case: oracle.salsanext.fused_conv on the same fp16-rounded operands,
err <= 2^-10 |want| + 1e-4 max(1, max|want| / 30) (fp32 summation order and one rounding to fp16).  The two epilogue forms (the default and
SLU_GEMM1X1_RES_AHEAD=0, gemm1x1_h8_kernel_v1) run the same arithmetic in the same order, so their raw outputs are equal byte for byte.

Both switches (SLU_GEMM1X1_RES_AHEAD, SLU_H8_GEMM1X1) are read once per process, so each switched path runs in a fresh child process (this
file as a script, under its own timeout); a child that faults, aborts or times out fails the test, which then starts nothing further.

MULTI: N = 17 at 16x256 is 272 tiles of 256 pixels on 256 workgroups, so 16 workgroups walk two tiles and issue the second tile's first
burst before the first tile's residual is retired."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [p for p in (ROOT, HERE) if p not in sys.path]

from oracle import salsanext as osalsa  # noqa: E402
from semanticlidarunc_amd import h8, ops  # noqa: E402
from test_gpu_h8 import _conv_case  # noqa: E402

pytestmark = pytest.mark.gpu

K256, K256_V1, K128, K128_V1 = ("gemm1x1_h8_kernel<4, 4, 2>", "gemm1x1_h8_kernel_v1<4, 4, 2>", "gemm1x1_h8_kernel<2, 4, 3>",
                                "gemm1x1_h8_kernel_v1<2, 4, 3>")
# (parts, cout, residual): 2 chunks, 12 chunks, one chunk (the "last chunk" is the first), and two without residual
MULTI = [([128], 256, True), ([256, 256, 256], 256, True), ([64], 256, True), ([256], 256, False), ([64, 192], 256, False)]
MULTI_SHAPE = (17, 16, 256)
CASE_128 = ([128, 128, 128], 128, True)


def _run(dev, parts, cout, resid, shape, seed):
    """-> (raw h8 output on the device, recorded kernel name, a function giving the fp32 CPU oracle of the same fp16-rounded operands)"""
    n, hh, ww = shape
    g = torch.Generator().manual_seed(seed)
    r16 = lambda t: t.half().float()
    xs = [r16(torch.randn(n, c, hh, ww, generator=g)) for c in parts]
    cin = sum(parts)
    wgt = r16(torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5)
    bias, bn_a, bn_b = torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    res = r16(torch.randn(n, cout, hh, ww, generator=g)) if resid else None
    d = lambda t: t.to(dev).contiguous()
    ops.TIMING, ops.TIMING_TAGS = [], []      # measurement mode records the instantiation slu_conv2d_h8_kernel_name reports
    try:
        got = h8.conv2d_h8([h8.H8Source(h8.to_h8(d(x))) for x in xs], h8.pack_conv_weight_h8(d(wgt)), cin, cout, 1, 1, 0, bias=d(bias), slope=0.01,
                           bn_a=d(bn_a), bn_b=d(bn_b), resid=None if res is None else h8.to_h8(d(res)))
        names = [t[0] for t in ops.TIMING]
    finally:
        ops.TIMING, ops.TIMING_TAGS = None, []
    assert len(names) == 1, names
    return got, names[0], (lambda: osalsa.fused_conv([(x, None, False) for x in xs], wgt, bias, 0, 1, 0.01, bn_a, bn_b, res))


def _raw(got):
    return got.contiguous().view(torch.int16).cpu().numpy().ravel()


def _within_bar(got, cout, want):
    err = (h8.from_h8(got, cout).cpu() - want).abs()
    return bool((err <= 2.0 ** -10 * want.abs() + 1e-4 * max(1.0, float(want.abs().max()) / 30)).all()), float(err.max())


def _run_child(mode, env_add, *args):
    env = dict(os.environ)
    env.update(env_add)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), mode, *args]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"child {mode} exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"


@pytest.fixture(scope="module")
def multi(cuda):
    """The MULTI cases in the default form, once: raw bytes, recorded name and whether the result is within the bar."""
    assert os.environ.get("SLU_GEMM1X1_RES_AHEAD", "1") != "0" and os.environ.get("SLU_H8_GEMM1X1", "1") == "1", "the parent runs the defaults"
    out = []
    for i, (parts, cout, resid) in enumerate(MULTI):
        got, name, oracle = _run(cuda, parts, cout, resid, MULTI_SHAPE, 300 + i)
        ok, worst = _within_bar(got, cout, oracle())
        out.append((_raw(got), name, ok, worst))
    return out


@pytest.mark.parametrize("i", range(len(MULTI)))
def test_workgroups_walk_several_tiles(multi, i):
    raw, name, ok, worst = multi[i]
    assert name == K256, name
    assert ok, (MULTI[i], worst)


@pytest.mark.parametrize("parts,resid", [([256, 256, 256], True), ([64], True), ([128], True), ([256], False)])
def test_fewer_tiles_than_workgroups(cuda, parts, resid):
    """N = 1 at 4x64: one tile, every tensor exactly as large as the kernel's last access."""
    _conv_case(cuda, 1, parts, 256, 4, 64, (1, 1, 0), seed=sum(parts) + 5, resid=resid, expect_kernel=K256)


def test_one_chunk_per_tile_a_few_tiles(cuda):
    _conv_case(cuda, 3, [64], 256, 8, 64, (1, 1, 0), seed=41, resid=True, expect_kernel=K256)


def test_two_epilogue_forms_compute_the_same_bytes(multi):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "v1.npy")
        _run_child("forms", {"SLU_GEMM1X1_RES_AHEAD": "0"}, path, K256_V1)      # first: nothing more is started if the child fails
        theirs = np.load(path)
    pos = 0
    for (parts, cout, resid), (mine, _, _, _) in zip(MULTI, multi):
        assert np.array_equal(mine, theirs[pos:pos + mine.size]), (parts, cout, resid, int((mine != theirs[pos:pos + mine.size]).sum()))
        pos += mine.size
    assert pos == theirs.size


def test_128_output_concat_conv_with_residual_is_dispatched_to_the_gemm(cuda):
    """The gate is narrow: 384 -> 128 from three sources WITH a residual; the same layer without one stays on the streaming kernel."""
    _conv_case(cuda, 3, [128, 128, 128], 128, 16, 64, (1, 1, 0), seed=51, resid=True, expect_kernel=K128)
    _conv_case(cuda, 3, [128, 128, 128], 128, 16, 64, (1, 1, 0), seed=52, resid=False, expect_kernel="conv1x1_h8_kernel<4, 1>")


def test_128_output_instantiation_both_forms(cuda):
    """gemm1x1_h8_kernel<2, 4, 3> (ring of 3: the chunk wait is vmcnt(NPIECE), stricter with the residual loads in between) behind
    SLU_H8_GEMM1X1=2: the bar and the recorded name in the child, and the same bytes from the two epilogue forms."""
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, "ahead.npy"), os.path.join(tmp, "v1.npy")
        _run_child("g128", {"SLU_H8_GEMM1X1": "2"}, a, K128)
        _run_child("g128", {"SLU_H8_GEMM1X1": "2", "SLU_GEMM1X1_RES_AHEAD": "0"}, b, K128_V1)
        mine, theirs = np.load(a), np.load(b)
    assert np.array_equal(mine, theirs), int((mine != theirs).sum())


def _child_forms(dev, path, expect):
    raws = []
    for i, (parts, cout, resid) in enumerate(MULTI):
        got, name, _ = _run(dev, parts, cout, resid, MULTI_SHAPE, 300 + i)
        assert name == expect, name      # the switch took effect
        raws.append(_raw(got))
    np.save(path, np.concatenate(raws))


def _child_g128(dev, path, expect):
    parts, cout, resid = CASE_128
    got, name, oracle = _run(dev, parts, cout, resid, MULTI_SHAPE, 400)
    assert name == expect, name
    ok, worst = _within_bar(got, cout, oracle())
    assert ok, (CASE_128, worst)
    np.save(path, _raw(got))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    device = torch.device("cuda:0")
    if sys.argv[1] == "forms":
        _child_forms(device, sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "g128":
        _child_g128(device, sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(f"unknown mode {sys.argv[1]}")
    torch.cuda.synchronize()
