"""GPU: the 128-channel member of the counted-wait fused tail, tail2_h8_kernel<4, 2, 3, RES> (csrc/conv_tail128_h8.h), at the smallest shapes at
which it can go wrong.  A launch reaches it from 256 tiles of 8 rows x 64 columns on (one round of the 256 persistent workgroups), so every
case here has at least that many.  Every case checks the name the launch records, the result against the same two layers through the unfused
h8 kernels (2e-3 of the output scale: same fp16 operands and rounding of the intermediate, another fp32 summation order of the 1x1) and
against the CPU oracle's fused_conv on the fp16-rounded operands (3e-3: its output is not rounded to fp16).  128 is a multiple of 8: an h8
tensor of 128 channels has no pad channels, which the cases assert on the output's shape.

The model-level case runs SalsaNext in half precision at 16 passes of 64 x 512, where ResBlock 2 (32 x 256, 16 images: exactly 256 tiles)
reaches the kernel, against a child process with SLU_FUSE_TAIL=0 (every tail as two launches); bar: the 1e-3 of test_gpu_model.py."""
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
C = 128
NAME = "tail2_h8_kernel<4,"


def _ends_its_allocation(t):
    p, nbytes = t.data_ptr(), t.numel() * t.element_size()
    seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= p < s["address"] + s["total_size"]]
    return len(seg) == 1 and seg[0]["address"] + seg[0]["total_size"] == p + nbytes


def _case(dev, n, hh, ww, resid, seed, plain=False, big=False, tight=False):
    """plain: no bias, BN or activation.  big: activations x 30.  tight: a1, a2, the residual and the output each fill a device allocation of
    their own to its last byte (allocated first, from an empty cache)."""
    assert ((ww + 63) // 64) * ((hh + 7) // 8) * n >= 256
    bufs = None
    if tight:
        torch.cuda.empty_cache()
        bufs = [torch.empty(n, C // 8, hh, ww, 8, dtype=torch.float16, device=dev) for _ in range(4)]
        assert all(_ends_its_allocation(b) for b in bufs), "a tensor does not end its allocation"
    g = torch.Generator(device=dev).manual_seed(seed)
    mag = 30.0 if big else 1.0
    a1 = torch.randn(n, C, hh, ww, device=dev, generator=g) * mag
    a2 = torch.randn(n, C, hh, ww, device=dev, generator=g) * mag
    r = torch.randn(n, C, hh, ww, device=dev, generator=g) * mag if resid else None
    w2 = torch.randn(C, C, 2, 2, device=dev, generator=g) / (4 * C) ** 0.5
    w1 = torch.randn(C, 3 * C, 1, 1, device=dev, generator=g) / (3 * C) ** 0.5
    ba = bb = bna = bnb = slope = None
    if not plain:
        slope = 0.01
        ba, bb = torch.randn(C, device=dev, generator=g) * 0.1, torch.randn(C, device=dev, generator=g) * 0.1
        bna = (torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g) * 0.1)
        bnb = (torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g) * 0.1)
    h1, h2, hr = h8.to_h8(a1), h8.to_h8(a2), (None if r is None else h8.to_h8(r))
    out = None
    if tight:
        h1, h2, out = bufs[0].copy_(h1), bufs[1].copy_(h2), bufs[3]
        hr = None if hr is None else bufs[2].copy_(hr)
    p2, p1 = h8.pack_conv_weight_h8(w2), h8.pack_conv_weight_h8(w1)
    ops.TIMING, ops.TIMING_TAGS = [], []      # measurement mode records the instantiation the launch names
    try:
        raw = h8.conv_tail_h8(h1, h2, p2, p1, ba, slope, bna, bb, slope, bnb, resid=hr, out=out)
        names = [t[0] for t in ops.TIMING]
    finally:
        ops.TIMING, ops.TIMING_TAGS = None, []
    assert len(names) == 1 and names[0].startswith(NAME) and names[0].endswith(f", {1 if resid else 0}>"), names
    assert tuple(raw.shape) == (n, C // 8, hh, ww, 8)      # 16 full channel blocks: no pad channel exists
    fused = h8.from_h8(raw, C).cpu()
    kw = lambda pair: dict(bn_a=None if pair is None else pair[0], bn_b=None if pair is None else pair[1])
    h3 = h8.conv2d_h8([h8.H8Source(h2)], p2, C, C, 2, 2, 1, bias=ba, slope=slope, **kw(bna))
    unf = h8.from_h8(h8.conv2d_h8([h8.H8Source(h1), h8.H8Source(h2), h8.H8Source(h3)], p1, 3 * C, C, 1, 1, 0, bias=bb, slope=slope, resid=hr,
                                  **kw(bnb)), C).cpu()
    q = lambda t: t.half().float().cpu()
    cpu = lambda t: None if t is None else t.cpu()
    pair = lambda pr: (None, None) if pr is None else (pr[0].cpu(), pr[1].cpu())
    a3 = osalsa.fused_conv([(q(a2), None, False)], q(w2), cpu(ba), 1, 2, slope, *pair(bna)).half().float()
    ref = osalsa.fused_conv([(q(a1), None, False), (q(a2), None, False), (a3, None, False)], q(w1), cpu(bb), 0, 1, slope, *pair(bnb),
                            resid=None if r is None else q(r))
    scale = float(ref.abs().max())
    assert bool(torch.isfinite(fused).all())
    assert float((fused - unf).abs().max()) <= 2e-3 * scale, (n, hh, ww, float((fused - unf).abs().max()), scale)
    assert float((fused - ref).abs().max()) <= 3e-3 * scale, (n, hh, ww, float((fused - ref).abs().max()), scale)


def test_one_exact_round_with_residual(cuda):
    _case(cuda, 32, 8, 512, True, 21)                       # 8 x 1 x 32 = 256 tiles


def test_ragged_rounds_odd_batch_without_residual(cuda):
    _case(cuda, 33, 13, 500, False, 22)                     # 8 x 2 x 33 = 528 tiles = 2 rounds + 16; 5 rows and 52 columns in the border tiles


def test_fewer_rows_than_a_tile_and_a_ragged_width(cuda):
    _case(cuda, 128, 5, 100, True, 23)                      # 2 x 1 x 128 tiles of 5 rows; 36 columns in the second


def test_no_bias_bn_or_activation(cuda):
    _case(cuda, 64, 8, 200, False, 24, plain=True)          # 4 x 1 x 64


def test_large_magnitudes(cuda):
    _case(cuda, 43, 9, 384, True, 25, big=True)             # 6 x 2 x 43 = 516 tiles


def test_operands_that_end_their_allocations(cuda):
    """Register-direct loads of a1 / a2 / the residual, the stores and the halo DMA of border tiles next to the end of device memory they may
    touch: 128 x 4 x 96 records x 16 channel blocks = 12 MiB a tensor, a whole number of allocator segments."""
    _case(cuda, 128, 4, 96, True, 26, tight=True)           # 2 x 1 x 128 tiles of 4 rows; 32 columns in the second


def test_tile_count_that_is_no_multiple_of_the_grid(cuda):
    _case(cuda, 37, 8, 450, True, 27)                       # 8 x 1 x 37 = 296 tiles on 256 workgroups: 40 of them run a second tile


# ---- model level ----
def _logits(dev):
    from semanticlidarunc_amd import salsanext as sn
    from semanticlidarunc_amd.testing import seeded_model, synthetic_scan
    from semanticlidarunc_amd.utils.mc_dropout import mc_forward
    sn.set_conv_precision("f16")
    try:
        model = seeded_model(sn.SalsaNext).to(dev)
        x, _ = synthetic_scan(2, 64, 512, seed=77)
        torch.manual_seed(5)
        ops.TIMING, ops.TIMING_TAGS = [], []
        try:
            with torch.no_grad():
                out = mc_forward(model, [x.to(dev)], T=8)
            names = [t[0] for t in ops.TIMING]
        finally:
            ops.TIMING, ops.TIMING_TAGS = None, []
    finally:
        sn.set_conv_precision("fp32")
    return out.float().cpu().numpy(), names


def test_salsanext_f16_with_the_kernel_equals_two_launches(cuda):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "unfused.npy")
        env = dict(os.environ, SLU_FUSE_TAIL="0")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), path]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)      # first: nothing more is started if the child fails
        assert r.returncode == 0, f"child exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
        theirs = np.load(path)
    assert os.environ.get("SLU_FUSE_TAIL", "1") != "0", "the parent must run the fused tails"
    mine, names = _logits(cuda)
    assert any(n.startswith(NAME) for n in names), names      # ResBlock 2 reached the kernel
    assert mine.shape == theirs.shape and np.isfinite(mine).all()
    err = float(np.abs(mine - theirs).max())
    assert err <= 1e-3, err


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    got, launched = _logits(torch.device("cuda:0"))
    assert not any("tail" in n for n in launched), launched      # the switch took effect
    np.save(sys.argv[1], got)
    torch.cuda.synchronize()
