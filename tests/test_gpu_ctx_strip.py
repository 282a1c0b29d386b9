"""GPU: the column-strip schedule of the fused ResContextBlock kernel (csrc/ctx_block_h8.hip).  Each workgroup walks down a strip of 64
columns in bands of 8 rows and keeps the s / a1 rows it already computed in LDS row rings; a strip is split into row segments only when
there are fewer strips than CUs.  Covered here: strips of several bands, split segments, ragged H and W, and that the output does not
depend on how the launch is segmented.  Bars as in test_gpu_ctx_block.py: the three unfused launches and the fp32 oracle."""
import pytest
import torch

from oracle import salsanext as osalsa
from semanticlidarunc_amd import h8
from semanticlidarunc_amd import salsanext as sn
from semanticlidarunc_amd.testing import randomize_bn_

pytestmark = pytest.mark.gpu

_NCU = 256          # workgroups of one launch (one per CU)


def _segments(n, h, w):
    """(bands per strip, segments per strip) that the launch picks: a mirror of launch_ctx, used to state what each case covers."""
    strips, bands = n * ((w + 63) // 64), (h + 7) // 8
    per = bands
    if strips < _NCU:
        per = -(-bands // min(bands, -(-_NCU // strips)))
    return bands, -(-bands // per)


def _block(cin, seed, cuda):
    torch.manual_seed(seed)
    return randomize_bn_(sn.ResContextBlock(cin, 32), seed + 1).eval().to(cuda)


def _run(blk, xh, fuse):
    prev = sn._FUSE_CTX
    sn._FUSE_CTX = fuse
    try:
        with torch.no_grad():
            return blk(xh)
    finally:
        sn._FUSE_CTX = prev


def _input(cin, n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g) * torch.linspace(0.5, 20.0, cin).view(1, cin, 1, 1)
    x[:, :, h // 3, : w // 2] = 0.0                                    # a run of empty returns
    return x


def _check_three_launches(blk, xh, n, h, w):
    got = _run(blk, xh, True)
    ref3 = _run(blk, xh, False)
    assert got.shape == ref3.shape == (n, 4, h, w, 8) and got.dtype == torch.float16
    a, b = h8.from_h8(got).cpu(), h8.from_h8(ref3).cpu()
    diff = (a - b).abs()
    assert float(diff.max()) <= 4e-3 * float(b.abs().max()) + 1e-3 and float((diff > 0).float().mean()) <= 0.02, \
        (float(diff.max()), float((diff > 0).float().mean()))
    return a


def _check_oracle(blk, xh, cin, a):
    sd = {("blk." + k): v.detach().cpu() for k, v in blk.state_dict().items()}
    for k in list(sd):
        if k.endswith("conv1.weight") or k.endswith("conv2.weight") or k.endswith("conv3.weight"):
            sd[k] = sd[k].half().float()
    net = osalsa._Net(sd, False, None)
    with torch.no_grad():
        want = net.context(h8.from_h8(xh, cin).cpu(), "blk")
    err = (a - want).abs()
    assert float(err.max()) <= 6e-3 * float(want.abs().max()) + 2e-3, float(err.max())


# (cin, n, h, w): whole strips of 8 and 16 bands; split segments of 1 and 2 bands; ragged H and W, Cin 5 and 32
CASES = [
    (32, 16, 64, 1024),      # 256 strips of 8 bands, not split
    (5, 8, 128, 2048),       # 256 strips of 16 bands, not split
    (32, 1, 64, 512),        # 8 strips, split into 8 segments of 1 band
    (5, 2, 128, 1000),       # 32 strips (ragged W), 8 segments of 2 bands
    (32, 1, 13, 75),         # ragged H and W: 2 bands, one segment each
    (5, 3, 61, 1000),        # ragged H (last band of 5 rows) and W, 48 strips, segments of 2 bands
    (32, 5, 61, 75),         # ragged, 10 strips, 8 segments of 1 band
    (5, 1, 13, 1000),
]


@pytest.mark.parametrize("cin,n,h,w", CASES)
def test_strip_bands_and_segments_match_the_three_launches(cuda, cin, n, h, w):
    blk = _block(cin, 7 + cin, cuda)
    xh = h8.to_h8(_input(cin, n, h, w, cin * 1000 + h + w).to(cuda))
    a = _check_three_launches(blk, xh, n, h, w)
    if n * h * w <= 2 * 64 * 1024:                                    # the CPU oracle on the smaller cases
        _check_oracle(blk, xh, cin, a)


def test_case_table_covers_both_schedules():
    segs = [_segments(n, h, w) for _, n, h, w in CASES]
    assert any(s == 1 and b >= 8 for b, s in segs) and any(s > 1 and b // s >= 2 for b, s in segs) and any(b == s > 1 for b, s in segs)


@pytest.mark.parametrize("cin", [5, 32])
def test_output_does_not_depend_on_the_segmentation(cuda, cin):
    """The same image alone (8 strips: every strip split into 8 segments of one band) and inside a batch of 64 (512 strips: whole
    strips of 8 bands) gives bit-identical output."""
    n, h, w = 64, 64, 512
    assert _segments(1, h, w) == (8, 8) and _segments(n, h, w) == (8, 1)
    blk = _block(cin, 21 + cin, cuda)
    xh = h8.to_h8(_input(cin, n, h, w, 5 + cin).to(cuda))
    batch = _run(blk, xh, True)
    for i in (0, 37, 63):
        alone = _run(blk, xh[i:i + 1].contiguous(), True)
        assert torch.equal(alone[0], batch[i]), i
