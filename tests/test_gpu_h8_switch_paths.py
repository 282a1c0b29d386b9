"""GPU: two h8 paths that only an environment switch reaches.  Both switches are read once per process (a `static const` in the launcher),
so each path runs in a fresh child Python process (this file as a script, `subprocess.run` under its own timeout); a child that faults,
aborts or times out fails the test, which then starts nothing further.

SLU_TAIL_V1=1   the round-1 fused tail, tail_h8_kernel (conv_tail_h8.hip): the child runs test_gpu_h8_tail._case -- against the unfused h8
                kernels at 2e-3 and the fp32 CPU oracle at 3e-3 of the output scale -- and checks that the launch names that kernel.
SLU_H8_ORDER=0  conv_h8_kernel's contiguous tile runs (conv_h8_tiled.hip): the two orders deal the same tiles to different workgroups and the
                arithmetic per tile is the same, so the child's raw h8 outputs must equal the parent's (default order) byte for byte; the
                parent's own result is held to the single-kernel bar of test_gpu_h8.py against oracle.salsanext.fused_conv."""
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

pytestmark = pytest.mark.gpu

TAIL_V1_NAMES = {32: "tail_h8_kernel<1, 1, 8, 2, true>", 64: "tail_h8_kernel<2, 1, 8, 1, true>"}
# (n, H, W) x channels of the 3x3 pad-1 convs; the last shape (128 channels only, bytes only) is 288 tiles of 8 rows on 256 workgroups: a
# contiguous run of two tiles in 32 of them, ragged in W
ORDER_SHAPES = [(3, 19, 150), (70, 8, 64)]
ORDER_CASES = [(c, s) for s in ORDER_SHAPES for c in (32, 128)] + [(128, (2, 72, 1000))]


def _order_case(dev, c, shape, seed):
    """-> (raw h8 output on the device, fp32 CPU oracle of the same fp16-rounded operands)"""
    n, hh, ww = shape
    g = torch.Generator().manual_seed(seed)
    r16 = lambda t: t.half().float()
    x = r16(torch.randn(n, c, hh, ww, generator=g))
    wgt = r16(torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5)
    bias, bn_a, bn_b = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    d = lambda t: t.to(dev).contiguous()
    got = h8.conv2d_h8([h8.H8Source(h8.to_h8(d(x)))], h8.pack_conv_weight_h8(d(wgt)), c, c, 3, 1, 1, bias=d(bias), slope=0.01, bn_a=d(bn_a),
                       bn_b=d(bn_b))
    return got, (lambda: osalsa.fused_conv([(x, None, False)], wgt, bias, 1, 1, 0.01, bn_a, bn_b, None))


def _raw(got):
    return got.contiguous().view(torch.int16).cpu().numpy().ravel()


def _child_tail_v1(dev):
    from test_gpu_h8_tail import _case
    for c in (32, 64):
        ops.TIMING, ops.TIMING_TAGS = [], []      # measurement mode records the instantiation slu_conv_tail_h8_kernel_name reports
        try:
            _case(dev, c, 1, 19, 150, True, 3)                                     # partial tiles in both directions, residual
            _case(dev, c, 2, 5, 37, False, 4, slope_a=None, slope_b=None, bn=False)  # tiny, no activation, no BN
            _case(dev, c, 3, 16, 64, False, 2)                                     # one tile column, several images
            names = [t[0] for t in ops.TIMING if "tail" in t[0]]
        finally:
            ops.TIMING, ops.TIMING_TAGS = None, []
        assert names == [TAIL_V1_NAMES[c]] * 3, names                             # the switch took effect


def _child_order0(dev, path):
    np.save(path, np.concatenate([_raw(_order_case(dev, c, s, 100 + i)[0]) for i, (c, s) in enumerate(ORDER_CASES)]))


def _run_child(mode, switch, *args):
    env = dict(os.environ)
    env[switch[0]] = switch[1]
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), mode, *args]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"child {mode} exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"


def test_round1_tail_kernel_behind_its_switch(cuda):
    _run_child("tail_v1", ("SLU_TAIL_V1", "1"))


def test_contiguous_tile_order_computes_the_same_bytes(cuda):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "order0.npy")
        _run_child("order0", ("SLU_H8_ORDER", "0"), path)      # first: nothing more is started if the child fails
        theirs = np.load(path)
    assert os.environ.get("SLU_H8_ORDER", "1") != "0", "the parent must run the default order"
    pos = 0
    for i, (c, shape) in enumerate(ORDER_CASES):
        got, oracle = _order_case(cuda, c, shape, 100 + i)
        mine = _raw(got)
        assert np.array_equal(mine, theirs[pos:pos + mine.size]), (c, shape, int((mine != theirs[pos:pos + mine.size]).sum()))
        pos += mine.size
        if shape in ORDER_SHAPES:      # the bar of test_gpu_h8._conv_case: fp32 summation order + one rounding to fp16
            want = oracle()
            err = (h8.from_h8(got, c).cpu() - want).abs()
            assert bool((err <= 2.0 ** -10 * want.abs() + 1e-4 * max(1.0, float(want.abs().max()) / 30)).all()), (c, shape, float(err.max()))
    assert pos == theirs.size


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    device = torch.device("cuda:0")
    if sys.argv[1] == "tail_v1":
        _child_tail_v1(device)
    elif sys.argv[1] == "order0":
        _child_order0(device, sys.argv[2])
    else:
        raise SystemExit(f"unknown mode {sys.argv[1]}")
    torch.cuda.synchronize()
