"""GPU: the strict MC schedule reads its B distinct input images in place.  `ctx_h8_kernel` with a broadcast input (output image n is the
block of x[n % B], csrc/ctx_block_h8.hip) against the same kernel on the materialised x.repeat(T): the same instructions on the same
values, so every output bit is equal; and `mc_predict` with the broadcast on against off, same generator state."""
import pytest
import torch

from semanticlidarunc_amd import h8
from semanticlidarunc_amd import salsanext as sn
from semanticlidarunc_amd.testing import randomize_bn_, seeded_model, synthetic_scan
from semanticlidarunc_amd.utils.mc_dropout import mc_predict

pytestmark = pytest.mark.gpu


def _ctx_operands(blk):
    packs = [h8.pack_conv_weight_h8(c.weight.detach().contiguous()) for c in (blk.conv1, blk.conv2, blk.conv3)]
    folded = [blk._folded_bn(blk._prepared(c), bn) for c, bn in ((blk.conv2, blk.bn1), (blk.conv3, blk.bn2))]
    return packs, [c.bias.detach() for c in (blk.conv1, blk.conv2, blk.conv3)], folded


@pytest.mark.parametrize("cin,b,t,h,w", [(5, 8, 2, 64, 512), (5, 3, 3, 16, 80), (32, 2, 5, 13, 75), (5, 1, 4, 8, 64), (16, 5, 2, 24, 200)])
def test_broadcast_input_equals_the_repeated_one(cuda, cin, b, t, h, w):
    torch.manual_seed(cin + b)
    blk = randomize_bn_(sn.ResContextBlock(cin, 32), cin + 7).eval().to(cuda)
    g = torch.Generator().manual_seed(100 * cin + w)
    x = torch.randn(b, cin, h, w, generator=g) * torch.linspace(0.5, 20.0, cin).view(1, cin, 1, 1)
    xh = h8.to_h8(x.to(cuda))
    packs, bias, folded = _ctx_operands(blk)
    args = (cin, packs[0], packs[1], packs[2], bias[0], bias[1], folded[0], bias[2], folded[1], 0.01)
    with torch.no_grad():
        want = h8.ctx_block_h8(xh.repeat(t, 1, 1, 1, 1).contiguous(), *args)
        got = h8.ctx_block_h8(xh, *args, n_out=t * b)
        one = h8.ctx_block_h8(xh, *args)
    assert got.shape == want.shape == (t * b, 4, h, w, 8)
    assert torch.equal(got, want)
    assert torch.equal(got[(t - 1) * b:], one)                # pass t - 1 of image i is the block of image i
    for bad in (0, t * b + 1) if b > 1 else (0,):             # not a positive multiple of the input batch
        with pytest.raises(RuntimeError):
            h8.ctx_block_h8(xh, *args, n_out=bad)


@pytest.mark.parametrize("b,t,h,w", [(1, 2, 64, 2048), (3, 3, 48, 176)])
def test_mc_predict_with_and_without_the_input_broadcast(cuda, b, t, h, w):
    model = seeded_model(sn.SalsaNext).to(cuda)
    x, _ = synthetic_scan(b, h, w, seed=17)
    x = x.to(cuda)
    sn.set_conv_precision("f16")
    prev = sn._MC_BCAST_INPUT
    try:
        outs = []
        for on in (True, False):
            sn._MC_BCAST_INPUT = on
            torch.manual_seed(23)
            outs.append([v.clone() for v in mc_predict(model, [x], T=t)])
    finally:
        sn._MC_BCAST_INPUT = prev
        sn.set_conv_precision("fp32")
    for got, want in zip(*outs):
        assert got.shape == want.shape and torch.equal(got, want)
    assert float(outs[0][2].max()) > 0.0                      # the passes really differ: the mutual information is not identically zero
