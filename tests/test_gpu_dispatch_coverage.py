"""GPU: one oracle case for every conv kernel instantiation the benchmark and the training step launch, at a shape that
selects it, and a coverage test that keeps that true as the dispatch rules change.

The dispatchers (choose_h8 in csrc/conv_h8_tiled.hip, choose_cfg in csrc/conv_common.h, launch_h8_m128) choose the tile from the
launch size, so the configurations of the full-size runs (>= 256 / 512 / 3 072 workgroups) are never reached by the small shapes of
test_gpu_h8.py / test_gpu_conv.py / test_gpu_f16x3.py.  Each row of the tables below names the instantiation its shape must select
(read back from ops.TIMING, i.e. slu_conv2d_h8_kernel_name / slu_conv2d_kernel_name: the launch's own dispatch with a leaf that
prints its template arguments instead of launching, so the name is the launched one by construction; test_dispatch_names_cpu.py asks
the same rows for their names without a GPU) and checks every output element at the bar of its precision:
  h8     2^-10 |y| + 1e-4 max(1, max|y| / 30) against the oracle fed the same fp16-rounded operands; pad channels exactly 0
  fp32   1e-4 abs on O(1) outputs (fused BatchNorm statistics: as test_gpu_backward.test_fused_bn_statistics)
  f16x3  1e-4 scale against the oracle, 2e-5 scale against the fp32 kernel
Ragged rows (H not a multiple of the tile height, W not a multiple of 64, Cout not a multiple of the workgroup's channel group,
a half-empty last K-step, odd N, no bias / BatchNorm / activation / residual, large magnitudes) still select the same form."""
import pytest
import torch

from oracle import salsanext as osalsa
from semanticlidarunc_amd import ops, salsanext as sn
from semanticlidarunc_amd.testing import seeded_model, synthetic_scan

pytestmark = pytest.mark.gpu
K1, K3, K3D2, K2D2 = (1, 1, 0), (3, 1, 1), (3, 2, 2), (2, 2, 1)


# (instantiation the shape must select, family, source channel counts, Cout, N, H, W, options)
H8_CASES = [
    # M128_TH8, one plain source: the ONE / OPT = 15 form of launch_h8_m128 (every 128 / 256-channel layer of the bench headline)
    ("conv_h8_kernel<3, 1, 1, 2, 2, 4, 2, false, false, false, 1, 15, true>", K3, [64], 128, 2, 64, 1024, {}),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 4, 2, false, false, false, 1, 15, true>", K3, [128], 256, 2, 32, 1024, {}),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 4, 2, false, false, false, 1, 15, true>", K3, [136], 160, 1, 61, 1000, {"resid": False}),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 4, 2, false, false, false, 1, 15, true>", K3, [128], 224, 3, 24, 1000,
     {"bias": False, "bn": False, "act": False, "big": True}),
    ("conv_h8_kernel<3, 2, 2, 2, 2, 4, 2, false, false, false, 1, 15, true>", K3D2, [128], 128, 2, 64, 1024, {}),
    ("conv_h8_kernel<3, 2, 2, 2, 2, 4, 2, false, false, false, 1, 15, true>", K3D2, [128], 128, 3, 45, 1000, {"resid": False, "big": True}),
    ("conv_h8_kernel<3, 2, 2, 2, 2, 4, 2, false, false, false, 1, 15, true>", K3D2, [136], 160, 1, 64, 1000, {"bias": False, "bn": False, "act": False}),
    ("conv_h8_kernel<2, 2, 1, 2, 2, 4, 2, false, false, false, 1, 15, true>", K2D2, [128], 128, 2, 64, 1024, {}),
    ("conv_h8_kernel<2, 2, 1, 2, 2, 4, 2, false, false, false, 1, 15, true>", K2D2, [136], 160, 1, 61, 1000, {"resid": False}),
    ("conv_h8_kernel<2, 2, 1, 2, 2, 4, 2, false, false, false, 1, 15, true>", K2D2, [128], 224, 3, 45, 1000,
     {"bias": False, "bn": False, "act": False, "big": True}),
    # M128_TH8 with dropout multipliers (UpBlock.conv1 of the 128-channel levels)
    ("conv_h8_kernel<3, 1, 1, 2, 2, 4, 2, true, false, false, 1, 0, false>", K3, [64, 64], 128, 2, 64, 1024, {"scales": True}),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 4, 2, true, false, false, 1, 0, false>", K3, [64, 72], 160, 3, 24, 1000, {"scales": True, "resid": False, "big": True}),
    # M128_TH4 (the 4x128 level of the headline, the 16x512 level of the B = 1 stream)
    ("conv_h8_kernel<3, 1, 1, 2, 2, 2, 2, false, false, false, 1, 0, false>", K3, [128], 128, 64, 4, 256, {}),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 2, 2, false, false, false, 1, 0, false>", K3, [136], 160, 64, 6, 250, {"resid": False, "big": True}),
    ("conv_h8_kernel<3, 2, 2, 2, 2, 2, 2, false, false, false, 1, 0, false>", K3D2, [128], 128, 64, 4, 256, {}),
    ("conv_h8_kernel<3, 2, 2, 2, 2, 2, 2, false, false, false, 1, 0, false>", K3D2, [136], 224, 65, 7, 130, {"bias": False, "bn": False, "act": False}),
    ("conv_h8_kernel<3, 2, 2, 2, 2, 2, 2, false, false, false, 1, 0, false>", K3D2, [128], 128, 8, 16, 512, {}),
    ("conv_h8_kernel<2, 2, 1, 2, 2, 2, 2, false, false, false, 1, 0, false>", K2D2, [128], 128, 64, 4, 256, {}),
    ("conv_h8_kernel<2, 2, 1, 2, 2, 2, 2, false, false, false, 1, 0, false>", K2D2, [136], 160, 65, 7, 250, {"resid": False}),
    ("conv_h8_kernel<2, 2, 1, 2, 2, 2, 2, false, false, false, 1, 0, false>", K2D2, [128], 128, 8, 16, 512, {}),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 2, 2, true, false, false, 1, 0, false>", K3, [64, 64], 128, 64, 4, 256, {"scales": True}),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 2, 2, true, false, false, 1, 0, false>", K3, [64, 72], 160, 65, 6, 250, {"scales": True, "resid": False}),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 2, 2, true, false, false, 1, 0, false>", K3, [32, 256], 128, 8, 16, 512, {"scales": True}),
    # M64_TH16, with multipliers as launched (160 -> 64 at 32x1024) and plain
    ("conv_h8_kernel<3, 1, 1, 2, 1, 8, 2, true, false, false, 1, 0, false>", K3, [32, 32], 64, 4, 64, 1024, {"scales": True}),
    ("conv_h8_kernel<3, 1, 1, 2, 1, 8, 2, true, false, false, 1, 0, false>", K3, [32, 40], 40, 3, 96, 1000, {"scales": True, "resid": False, "big": True}),
    ("conv_h8_kernel<3, 1, 1, 2, 1, 8, 2, false, false, false, 1, 0, false>", K3, [64], 64, 4, 64, 1024, {}),
    ("conv_h8_kernel<3, 1, 1, 2, 1, 8, 2, false, false, false, 1, 0, false>", K3, [72], 48, 5, 61, 1000, {"bias": False, "bn": False, "act": False}),
    # M32_TH16: the shared-prefix UpBlock.conv1 (skip shared by the stacked passes)
    ("conv_h8_kernel<3, 1, 1, 1, 1, 8, 2, false, false, false, 1, 0, false>", K3, [16, 64], 32, 4, 64, 1024, {"nbatch_last": 2}),
    ("conv_h8_kernel<3, 1, 1, 1, 1, 8, 2, false, false, false, 1, 0, false>", K3, [16, 64], 20, 5, 61, 1000,
     {"nbatch_last": 1, "resid": False, "big": True}),
    # M32_TH8 (resident and streamed weights) / M64_TH8
    ("conv_h8_kernel<3, 1, 1, 1, 1, 4, 2, false, true, false, 1, 0, false>", K3, [32], 32, 2, 64, 1024, {}),
    ("conv_h8_kernel<3, 1, 1, 1, 1, 4, 2, false, false, false, 1, 0, false>", K3, [40], 24, 3, 45, 1000,
     {"bias": False, "bn": False, "act": False, "big": True}),
    ("conv_h8_kernel<3, 1, 1, 2, 1, 4, 2, false, false, false, 1, 0, false>", K3, [32], 64, 2, 64, 1024, {}),
    ("conv_h8_kernel<3, 1, 1, 2, 1, 4, 2, false, false, false, 1, 0, false>", K3, [40], 48, 3, 45, 1000, {"resid": False}),
    # M64_TH4 / M32_TH4 (the B = 1 stream's lower levels)
    ("conv_h8_kernel<3, 1, 1, 2, 1, 4, 1, false, false, false, 1, 0, false>", K3, [256], 256, 8, 8, 256, {}),
    ("conv_h8_kernel<3, 2, 2, 2, 1, 4, 1, false, false, false, 1, 0, false>", K3D2, [256], 256, 8, 8, 256, {}),
    ("conv_h8_kernel<2, 2, 1, 2, 1, 4, 1, false, false, false, 1, 0, false>", K2D2, [256], 256, 8, 8, 256, {}),
    ("conv_h8_kernel<3, 1, 1, 1, 1, 4, 1, false, false, false, 1, 0, false>", K3, [256], 256, 8, 4, 128, {}),
    ("conv_h8_kernel<3, 1, 1, 1, 1, 4, 1, false, false, false, 1, 0, false>", K3, [136], 160, 9, 6, 250, {"resid": False}),
    ("conv_h8_kernel<3, 1, 1, 1, 1, 4, 1, false, false, false, 1, 0, false>", K3, [136], 224, 3, 7, 130,
     {"bias": False, "bn": False, "act": False, "big": True}),
    ("conv_h8_kernel<3, 2, 2, 1, 1, 4, 1, false, false, false, 1, 0, false>", K3D2, [128], 128, 8, 8, 256, {}),
    ("conv_h8_kernel<2, 2, 1, 1, 1, 4, 1, false, false, false, 1, 0, false>", K2D2, [128], 128, 8, 8, 256, {}),
    ("conv_h8_kernel<3, 1, 1, 1, 1, 4, 1, true, false, false, 1, 0, false>", K3, [64, 256], 128, 8, 8, 256, {"scales": True}),
    # the streaming 1x1 kernel: 384 -> 128 concat conv, 64 -> 128 shortcut
    ("conv1x1_h8_kernel<4, 1>", K1, [128, 128, 128], 128, 2, 16, 256, {"resid": False}),
    ("conv1x1_h8_kernel<4, 1>", K1, [64], 128, 2, 32, 256, {}),
    ("conv1x1_h8_kernel<4, 1>", K1, [136], 112, 3, 8, 96, {"bias": False, "bn": False, "act": False}),
]

FP32_CASES = [
    # M32_TH8 (>= 3 072 eight-row tiles: inference batches)
    ("conv_fwd_kernel<1, 1, 0, 16, 1, 1, 4, 2, false>", K1, [8], 32, 12, 64, 2048, {}),
    ("conv_fwd_kernel<3, 1, 1, 8, 1, 1, 4, 2, false>", K3, [8], 32, 12, 64, 2048, {}),
    ("conv_fwd_kernel<3, 2, 2, 8, 1, 1, 4, 2, false>", K3D2, [8], 32, 12, 64, 2048, {}),
    ("conv_fwd_kernel<2, 2, 1, 8, 1, 1, 4, 2, false>", K2D2, [8], 32, 12, 64, 2048, {}),
    ("conv_fwd_kernel<3, 1, 1, 8, 1, 1, 4, 2, true>", K3, [8, 8], 32, 12, 64, 2048, {"scales": True}),
    ("conv_fwd_kernel<3, 1, 1, 8, 1, 1, 4, 2, true>", K3, [5], 20, 13, 61, 1950, {"resid": False, "bias": False, "bn": False, "act": False, "big": True}),
    # M64_TH8 (the training step's 64-channel layers at 64x2048, fused BatchNorm statistics)
    ("conv_fwd_kernel<1, 1, 0, 16, 2, 1, 4, 2, false>", K1, [32], 64, 4, 64, 1024, {}),
    ("conv_fwd_kernel<3, 1, 1, 8, 2, 1, 4, 2, false>", K3, [32], 64, 4, 64, 1024, {"stats": True}),
    ("conv_fwd_kernel<3, 1, 1, 8, 2, 1, 4, 2, false>", K3, [21], 40, 5, 61, 1000, {"resid": False, "stats": True, "big": True}),
    ("conv_fwd_kernel<3, 2, 2, 8, 2, 1, 4, 2, false>", K3D2, [64], 64, 4, 64, 1024, {"stats": True}),
    ("conv_fwd_kernel<3, 2, 2, 8, 2, 1, 4, 2, false>", K3D2, [19], 48, 5, 61, 1000, {"bias": False, "bn": False, "act": False}),
    ("conv_fwd_kernel<2, 2, 1, 8, 2, 1, 4, 2, false>", K2D2, [64], 64, 4, 64, 1024, {"stats": True}),
    ("conv_fwd_kernel<3, 1, 1, 8, 2, 1, 4, 2, true>", K3, [32, 32], 64, 4, 64, 1024, {"scales": True}),
    # M128_TH4 (>= 512 four-row tiles of 128 channels: the training step's 32x1024 level)
    ("conv_fwd_kernel<1, 1, 0, 16, 2, 2, 2, 2, false>", K1, [64], 128, 4, 32, 1024, {}),
    ("conv_fwd_kernel<3, 1, 1, 8, 2, 2, 2, 2, false>", K3, [64], 128, 4, 32, 1024, {"stats": True}),
    ("conv_fwd_kernel<3, 1, 1, 8, 2, 2, 2, 2, false>", K3, [37], 160, 5, 29, 500, {"resid": False, "stats": True, "big": True}),
    ("conv_fwd_kernel<3, 2, 2, 8, 2, 2, 2, 2, false>", K3D2, [64], 128, 4, 32, 1024, {"stats": True}),
    ("conv_fwd_kernel<2, 2, 1, 8, 2, 2, 2, 2, false>", K2D2, [128], 128, 4, 32, 1024, {"stats": True}),
    ("conv_fwd_kernel<2, 2, 1, 8, 2, 2, 2, 2, false>", K2D2, [37], 224, 5, 29, 500, {"bias": False, "bn": False, "act": False}),
    ("conv_fwd_kernel<3, 1, 1, 8, 2, 2, 2, 2, true>", K3, [32, 32], 128, 4, 32, 1024, {"scales": True}),
    # M64_TH4
    ("conv_fwd_kernel<1, 1, 0, 16, 2, 1, 4, 1, false>", K1, [64], 128, 4, 32, 512, {}),
    ("conv_fwd_kernel<3, 1, 1, 8, 2, 1, 4, 1, false>", K3, [64], 128, 4, 32, 512, {"stats": True}),
    ("conv_fwd_kernel<3, 1, 1, 8, 2, 1, 4, 1, false>", K3, [37], 72, 5, 29, 500, {"resid": False, "big": True}),
    ("conv_fwd_kernel<3, 2, 2, 8, 2, 1, 4, 1, false>", K3D2, [64], 128, 4, 32, 512, {}),
    ("conv_fwd_kernel<2, 2, 1, 8, 2, 1, 4, 1, false>", K2D2, [64], 128, 4, 32, 512, {}),
    ("conv_fwd_kernel<3, 1, 1, 8, 2, 1, 4, 1, true>", K3, [32, 32], 128, 4, 32, 512, {"scales": True}),
    # M32_TH4 (the training step's 32-channel layers, the small maps)
    ("conv_fwd_kernel<1, 1, 0, 16, 1, 1, 4, 1, false>", K1, [32], 32, 4, 64, 512, {}),
    ("conv_fwd_kernel<3, 1, 1, 8, 1, 1, 4, 1, false>", K3, [32], 32, 4, 64, 512, {"stats": True}),
    ("conv_fwd_kernel<3, 1, 1, 8, 1, 1, 4, 1, false>", K3, [21], 20, 3, 61, 1000, {"resid": False, "stats": True}),
    ("conv_fwd_kernel<3, 1, 1, 8, 1, 1, 4, 1, false>", K3, [64], 64, 4, 16, 256, {"stats": True}),
    ("conv_fwd_kernel<3, 2, 2, 8, 1, 1, 4, 1, false>", K3D2, [32], 32, 4, 64, 512, {"stats": True}),
    ("conv_fwd_kernel<2, 2, 1, 8, 1, 1, 4, 1, false>", K2D2, [32], 32, 4, 64, 512, {}),
    ("conv_fwd_kernel<3, 1, 1, 8, 1, 1, 4, 1, true>", K3, [16, 16], 32, 4, 64, 512, {"scales": True}),
]

F16X3_CASES = [
    ("conv1x1_f16x3_kernel<1, 1>", K1, [32], 32, 4, 64, 512, {}),
    ("conv1x1_f16x3_kernel<2, 1>", K1, [32], 64, 4, 64, 512, {}),
    ("conv1x1_f16x3_kernel<4, 1>", K1, [64], 128, 4, 32, 512, {}),
    ("conv1x1_f16x3_kernel<8, 1>", K1, [64], 256, 4, 16, 256, {}),
    # 32 outputs: the 8-row tile is mapped to 4 rows
    ("conv_f16x3_kernel<3, 1, 1, 1, 1, 4, 1, false>", K3, [32], 32, 12, 64, 2048, {}),
    ("conv_f16x3_kernel<3, 2, 2, 1, 1, 4, 1, false>", K3D2, [8], 32, 12, 64, 2048, {}),
    ("conv_f16x3_kernel<2, 2, 1, 1, 1, 4, 1, false>", K2D2, [8], 32, 12, 64, 2048, {}),
    ("conv_f16x3_kernel<3, 1, 1, 1, 1, 4, 1, true>", K3, [16, 16], 32, 12, 64, 2048, {"scales": True}),
    # 64 outputs: M64_TH8 -> M64_TH4
    ("conv_f16x3_kernel<3, 1, 1, 2, 1, 4, 1, false>", K3, [32], 64, 4, 64, 1024, {}),
    ("conv_f16x3_kernel<3, 2, 2, 2, 1, 4, 1, false>", K3D2, [64], 64, 4, 64, 1024, {}),
    ("conv_f16x3_kernel<3, 2, 2, 2, 1, 4, 1, false>", K3D2, [21], 40, 5, 61, 1000, {"big": True}),
    ("conv_f16x3_kernel<2, 2, 1, 2, 1, 4, 1, false>", K2D2, [64], 64, 4, 64, 1024, {}),
    ("conv_f16x3_kernel<3, 1, 1, 2, 1, 4, 1, true>", K3, [32, 32], 64, 4, 64, 1024, {"scales": True}),
    # M128_TH4
    ("conv_f16x3_kernel<3, 1, 1, 2, 2, 2, 2, false>", K3, [64], 128, 4, 32, 1024, {}),
    ("conv_f16x3_kernel<3, 1, 1, 2, 2, 2, 2, false>", K3, [37], 160, 5, 29, 500, {"resid": False, "big": True}),
    ("conv_f16x3_kernel<3, 2, 2, 2, 2, 2, 2, false>", K3D2, [64], 128, 4, 32, 1024, {}),
    ("conv_f16x3_kernel<2, 2, 1, 2, 2, 2, 2, false>", K2D2, [128], 128, 4, 32, 1024, {}),
    ("conv_f16x3_kernel<3, 1, 1, 2, 2, 2, 2, true>", K3, [32, 32], 128, 4, 32, 1024, {"scales": True}),
]

# fused / special-purpose kernels whose oracle comparison (and name assertion) lives in another test
ELSEWHERE = {
    "ctx_h8_kernel<": "test_gpu_ctx_block.py",
    "tail2_h8_kernel<": "test_gpu_h8_tail.py",
    "ring3_h8_kernel<": "test_gpu_h8.py::test_deep_ring_3x3_full_resolution_layers / test_deep_ring_3x3_two_plain_sources",
    "gemm1x1_h8_kernel<": "test_gpu_h8.py::test_wide_1x1_gemm_kernel / test_wide_1x1_gemm_kernel_is_the_one_that_runs",
    "head_mc_h8_kernel<": "test_gpu_head_mc.py",
}


def _id(case):
    name, fam, parts, cout, n, h, w, opts = case
    return f"{name}|k{fam[0]}d{fam[1]}|{'+'.join(map(str, parts))}->{cout}|N{n}|{h}x{w}" + "".join(f"|{k}" for k in sorted(opts))


@pytest.mark.parametrize("case", H8_CASES, ids=_id)
def test_h8_instantiation(cuda, case):
    from test_gpu_h8 import _conv_case
    name, fam, parts, cout, n, h, w, opts = case
    _conv_case(cuda, n, parts, cout, h, w, fam, seed=cout + n + h + sum(parts), expect_kernel=name, **opts)


@pytest.mark.parametrize("case", FP32_CASES, ids=_id)
def test_fp32_instantiation(cuda, case):
    from test_gpu_conv import _run
    name, fam, parts, cout, n, h, w, opts = case
    _run(cuda, n, parts, cout, h, w, fam, seed=cout + n + h + sum(parts), expect_kernel=name, **opts)


@pytest.mark.parametrize("case", F16X3_CASES, ids=_id)
def test_f16x3_instantiation(cuda, case):
    from test_gpu_f16x3 import _run
    name, fam, parts, cout, n, h, w, opts = case
    _run(cuda, n, parts, cout, h, w, fam, seed=cout + n + h + sum(parts), expect_kernel=name, **opts)


def _recorded(fn):
    """Kernel instantiation names the conv launches inside fn() record (measurement mode), in launch order."""
    ops.TIMING, ops.TIMING_TAGS = [], []
    try:
        fn()
        torch.cuda.synchronize()
        return [(r[0], t) for r, t in zip(ops.TIMING, ops.TIMING_TAGS)]
    finally:
        ops.TIMING, ops.TIMING_TAGS = None, []


def _workloads(dev):
    """The runs whose conv launches must all be covered: name -> callable."""
    from semanticlidarunc_amd.loss import salsanext_loss
    from semanticlidarunc_amd.utils.mc_dropout import mc_predict

    def infer(precision, scans, h, w, passes, share_prefix=False):
        def run():
            sn.set_conv_precision(precision)
            try:
                model = seeded_model(sn.SalsaNext).to(dev)
                x, _ = synthetic_scan(scans, h, w, seed=1234)
                torch.manual_seed(100)
                with torch.no_grad():
                    out = mc_predict(model, [x.to(dev)], T=passes, share_prefix=share_prefix)
                assert all(bool(torch.isfinite(o.float()).all()) for o in out)
            finally:
                sn.set_conv_precision("fp32")
        return run

    def train(precision):
        def run():
            prev = sn._TRAIN_CONV_PRECISION
            sn.set_train_conv_precision(precision)
            try:
                model = seeded_model(sn.SalsaNext).to(dev).train()
                x, y = synthetic_scan(4, 64, 2048, seed=1234)
                scales = {k: v.to(dev) for k, v in osalsa.draw_dropout_scales(4, 0.2, torch.Generator().manual_seed(7)).items()}
                loss = salsanext_loss(model.forward_with_dropout_scales(x.to(dev), scales), y.to(dev), 1.0, 1.0, 0)[0]
                loss.backward()
                assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
            finally:
                sn.set_train_conv_precision(prev)
        return run

    return {
        "f16 headline 8x64x2048 T=8": infer("f16", 8, 64, 2048, 8),
        "f16 headline shared prefix": infer("f16", 8, 64, 2048, 8, share_prefix=True),
        "f16 B=1 stream T=8": infer("f16", 1, 64, 2048, 8),
        "f16 configs[4] 128x4096 T=16": infer("f16", 1, 128, 4096, 16),
        "fp32 headline": infer("fp32", 8, 64, 2048, 8),
        "f16x3 headline": infer("f16x3", 8, 64, 2048, 8),
        "fp32 training step B=4": train("fp32"),
    }


def test_every_launched_conv_instantiation_has_a_case(cuda):
    """The bench headline (both schedules), the B = 1 stream, configs[4], the fp32 / f16x3 headline and one fp32 training step
    (forward, dgrad): every conv instantiation they record has an oracle case above that asserts its name, or a pointer to the test
    that checks it.  Outputs are only checked to be finite here."""
    covered = {c[0] for c in H8_CASES + FP32_CASES + F16X3_CASES}
    missing = {}
    for run, fn in _workloads(cuda).items():
        for name, tag in _recorded(fn):
            if name not in covered and not any(name.startswith(p) for p in ELSEWHERE):
                missing.setdefault(name, f"{run}: {tag}")
    assert not missing, "conv instantiations without a case:\n" + "\n".join(f"  {k}   (e.g. {v})" for k, v in sorted(missing.items()))
