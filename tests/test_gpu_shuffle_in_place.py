"""GPU: UpBlock.conv1 reading its PixelShuffle'd input in place (slu_h8_src.shuffle) against pixel_shuffle_h8 followed by the plain-source
conv: ring3_h8_kernel<1, 1, 5, 1, 4> (the 80 -> 32 layer at full resolution) and every SCALED 3x3 conv_h8_kernel instantiation of the
coverage tables (shuffled source plus a scaled skip).  The multipliers are 0 or powers of 1.25, exact in fp16, and both forms round the
product to fp16 once before the same MFMA sequence: EQUAL outputs are expected, bit for bit."""
import pytest
import torch

from semanticlidarunc_amd import h8, ops
from semanticlidarunc_amd import salsanext as sn
from semanticlidarunc_amd.h8 import H8Source
from semanticlidarunc_amd.testing import seeded_model, synthetic_scan
from semanticlidarunc_amd.utils.mc_dropout import mc_predict

pytestmark = pytest.mark.gpu
RING3 = "ring3_h8_kernel<1, 1, 5, 1, 4>"


@pytest.mark.parametrize("n,h,w,mult,tight", [(1, 64, 2048, "composed", False), (3, 48, 1000, "composed", False), (3, 64, 2048, "zeros", True),
                                              (9, 24, 720, None, False), (2, 64, 2048, "ones", False)])
def test_in_place_source_equals_the_materialised_shuffle(cuda, n, h, w, mult, tight):
    g = torch.Generator(device=cuda).manual_seed(n * 1000 + w)
    stored_buf = None
    if tight:                                   # the stored tensor is allocated FIRST, from an empty cache: a segment of its own that it fills
        torch.cuda.empty_cache()
        stored_buf = torch.empty(n, 8, h // 2, w // 2, 8, dtype=torch.float16, device=cuda)
        p, nbytes = stored_buf.data_ptr(), stored_buf.numel() * 2
        seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= p < s["address"] + s["total_size"]]
        assert len(seg) == 1 and seg[0]["address"] + seg[0]["total_size"] == p + nbytes, "the tensor does not end its allocation"
    x = torch.randn(n, 64, h // 2, w // 2, device=cuda, generator=g)                  # the tensor PixelShuffle is applied to
    skip = h8.to_h8(torch.randn(n, 64, h, w, device=cuda, generator=g))
    perm = h8.shuffle_store_perm(64, cuda)
    stored = h8.to_h8(x.index_select(1, perm).contiguous())                          # what a permuting producer writes
    if stored_buf is not None:
        stored = stored_buf.copy_(stored)
    plain = h8.to_h8(x)
    sx = None
    if mult == "composed":                      # products of up to three Dropout2d sites: 0, 1.25, 1.25^2, 1.25^3
        k = torch.randint(0, 4, (n, 64), device=cuda, generator=g).float()
        sx = torch.where(torch.rand(n, 64, device=cuda, generator=g) < 0.25, torch.zeros_like(k), 1.25 ** k)
    elif mult == "zeros":
        sx = torch.zeros(n, 64, device=cuda)
        sx[:, ::5] = 1.25
    elif mult == "ones":
        sx = torch.ones(n, 64, device=cuda)
    wgt = torch.randn(32, 80, 3, 3, device=cuda, generator=g) / 27.0
    bias, bn_a, bn_b = (torch.randn(32, device=cuda, generator=g) * 0.1, torch.rand(32, device=cuda, generator=g) + 0.5,
                        torch.randn(32, device=cuda, generator=g) * 0.1)
    wpack = h8.pack_conv_weight_h8(wgt)
    kw = dict(bias=bias, slope=0.01, bn_a=bn_a, bn_b=bn_b)
    want = h8.conv2d_h8([H8Source(h8.pixel_shuffle_h8(plain, sx)), H8Source(skip)], wpack, 80, 32, 3, 1, 1, **kw)
    ops.TIMING, ops.TIMING_TAGS = [], []
    try:
        got = h8.conv2d_h8([H8Source(stored, None if sx is None else sx.index_select(1, perm).contiguous(), 0, True), H8Source(skip)],
                           wpack, 80, 32, 3, 1, 1, **kw)
        launched = [t[0] for t in ops.TIMING]
        nbytes = ops.TIMING[0][2]
    finally:
        ops.TIMING, ops.TIMING_TAGS = None, []
    assert launched == [RING3]
    # byte accounting: the stored source tensor ONCE (n x 64 ch x h/2 x w/2 fp16), the skip, the output, the weights
    assert nbytes == 2.0 * n * 64 * (h // 2) * (w // 2) + 2.0 * n * 64 * h * w + 2.0 * n * 32 * h * w + 2.0 * 32 * 80 * 9
    assert got.shape == want.shape == (n, 4, h, w, 8)
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())
    if mult == "zeros":                         # the dropped channels really matter: without multipliers the result differs
        other = h8.conv2d_h8([H8Source(stored, None, 0, True), H8Source(skip)], wpack, 80, 32, 3, 1, 1, **kw)
        assert not torch.equal(other, want)


SCALED_CASES = [      # (instantiation, shuffled channels | skip channels, Cout, N, H, W): rows of test_gpu_dispatch_coverage.H8_CASES
    ("conv_h8_kernel<3, 1, 1, 2, 2, 4, 2, true, false, false, 1, 0, false>", (64, 64), 128, 2, 64, 1024),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 4, 2, true, false, false, 1, 0, false>", (64, 72), 160, 3, 24, 1000),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 2, 2, true, false, false, 1, 0, false>", (64, 64), 128, 64, 4, 256),
    ("conv_h8_kernel<3, 1, 1, 2, 2, 2, 2, true, false, false, 1, 0, false>", (32, 256), 128, 8, 16, 512),
    ("conv_h8_kernel<3, 1, 1, 2, 1, 8, 2, true, false, false, 1, 0, false>", (32, 32), 64, 4, 64, 1024),
    ("conv_h8_kernel<3, 1, 1, 2, 1, 8, 2, true, false, false, 1, 0, false>", (32, 40), 40, 3, 96, 1000),
    ("conv_h8_kernel<3, 1, 1, 1, 1, 4, 1, true, false, false, 1, 0, false>", (64, 256), 128, 8, 8, 256),
]


@pytest.mark.parametrize("name,parts,cout,n,h,w", SCALED_CASES)
@pytest.mark.parametrize("mult", ["composed", "skip_only"])
def test_scaled_kernels_read_the_shuffled_source_in_place(cuda, name, parts, cout, n, h, w, mult):
    """A shuffled source plus a scaled skip (UpBlock.conv1 of upBlock1-3) on every SCALED 3x3 instantiation; odd N, W not a multiple of
    64, a skip that is not whole K-steps, zero and composed multipliers on both sources, and no multiplier on the shuffled one."""
    cu, cs = parts
    g = torch.Generator(device=cuda).manual_seed(cout * 100 + w + n)
    x = torch.randn(n, 4 * cu, h // 2, w // 2, device=cuda, generator=g)
    skip = h8.to_h8(torch.randn(n, cs, h, w, device=cuda, generator=g))
    perm = h8.shuffle_store_perm(4 * cu, cuda)
    stored, plain = h8.to_h8(x.index_select(1, perm).contiguous()), h8.to_h8(x)

    def table(c):
        k = torch.randint(0, 4, (n, c), device=cuda, generator=g).float()
        return torch.where(torch.rand(n, c, device=cuda, generator=g) < 0.25, torch.zeros_like(k), 1.25 ** k)
    sx = table(4 * cu) if mult == "composed" else None
    ss = table(8 * ((cs + 7) // 8))
    wgt = torch.randn(cout, cu + cs, 3, 3, device=cuda, generator=g) / (3.0 * (cu + cs) ** 0.5)
    bias, bn_a, bn_b = (torch.randn(cout, device=cuda, generator=g) * 0.1, torch.rand(cout, device=cuda, generator=g) + 0.5,
                        torch.randn(cout, device=cuda, generator=g) * 0.1)
    wpack = h8.pack_conv_weight_h8(wgt)
    kw = dict(bias=bias, slope=0.01, bn_a=bn_a, bn_b=bn_b)
    launched = []
    for srcs in ([H8Source(h8.pixel_shuffle_h8(plain, sx)), H8Source(skip, ss)],
                 [H8Source(stored, None if sx is None else sx.index_select(1, perm).contiguous(), 0, True), H8Source(skip, ss)]):
        ops.TIMING, ops.TIMING_TAGS = [], []
        try:
            launched.append((h8.conv2d_h8(srcs, wpack, cu + cs, cout, 3, 1, 1, **kw), ops.TIMING[0][0]))
        finally:
            ops.TIMING, ops.TIMING_TAGS = None, []
    (want, kw_name), (got, kg_name) = launched
    assert kw_name == kg_name == name
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())
    assert float(want.float().abs().max()) > 0.1


def test_shapes_outside_the_in_place_form_raise(cuda):
    stored = torch.zeros(1, 8, 8, 32, 8, dtype=torch.float16, device=cuda)
    skip = torch.zeros(1, 8, 16, 64, 8, dtype=torch.float16, device=cuda)
    wpack = h8.pack_conv_weight_h8(torch.zeros(32, 80, 3, 3, device=cuda))
    with pytest.raises(RuntimeError):           # 4 tiles and no multiplier anywhere: neither form covers it, nothing falls back silently
        h8.conv2d_h8([H8Source(stored, None, 0, True), H8Source(skip)], wpack, 80, 32, 3, 1, 1)


def test_draw_kernel_stored_order_is_an_index_select_of_the_channel_order(cuda):
    n, sites = 6, [(64, 0.2, True), (16, 0.2, True), (80, 0.3, True), (128, 0.2, True)]
    outs = lambda sh: [("a", 64, [(0, 0), (1, 0), (2, 0)], sh), ("b", 64, [(-1, 0), (1, 0)], sh), ("c", 128, [(3, 0)], sh), ("d", 64, [(0, 0)], 0)]
    res = []
    for sh in (1, 2):
        torch.manual_seed(77)
        res.append({k: v.clone() for k, v in ops.DropoutPlan(n, sites, outs(sh), cuda).run().items()})
    for key, c in (("a", 64), ("b", 64), ("c", 128)):
        assert torch.equal(res[1][key], res[0][key].index_select(1, h8.shuffle_store_perm(c, cuda)))
        assert not torch.equal(res[1][key], res[0][key])
    assert torch.equal(res[1]["d"], res[0]["d"])
    assert set(res[0]["a"].unique().tolist()) > {0.0}


def _with_switch(on, fn):
    prev = sn._SHUFFLE_IN_PLACE
    sn._SHUFFLE_IN_PLACE = on
    try:
        return fn()
    finally:
        sn._SHUFFLE_IN_PLACE = prev


@pytest.mark.parametrize("b,h,w", [(1, 64, 2048), (3, 48, 1008)])
def test_model_outputs_do_not_depend_on_the_fold(cuda, b, h, w):
    model = seeded_model(sn.SalsaNext).to(cuda).eval()
    x, _ = synthetic_scan(b, h, w, seed=31)
    x = x.to(cuda)
    g = torch.Generator().manual_seed(9)
    scales = {f"{blk}.{name}": ((torch.rand(b, c, generator=g) > 0.2).float() * 1.25).to(cuda) for blk, name, c in sn.SalsaNext._DROPOUT_SITES}
    sn.set_conv_precision("f16")
    try:
        with torch.no_grad():
            assert model._in_place_blocks(b, h, w, scaled=True) == ("upBlock1", "upBlock2", "upBlock3", "upBlock4")
            assert model._in_place_blocks(b, h, w, scaled=False) == ("upBlock4",)
            outs = [_with_switch(on, lambda: model.forward_with_dropout_scales(x, scales)) for on in (True, False)]
            assert torch.equal(outs[0], outs[1])
            det = [_with_switch(on, lambda: model(x)) for on in (True, False)]
            assert torch.equal(det[0], det[1])
        mc = []
        for on in (True, False):                # live Dropout2d: the multipliers come from the draw kernel, in stored order when folded
            torch.manual_seed(41)
            mc.append(_with_switch(on, lambda: [v.clone() for v in mc_predict(model, [x], T=2)]))
        for u, v in zip(*mc):
            assert torch.equal(u, v)
        assert float(mc[0][2].max()) > 0.0
    finally:
        sn.set_conv_precision("fp32")
