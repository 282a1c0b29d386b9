"""GPU: the ResNet-FPN model (models.semanticFCN, resnet18 / resnet34) on the half-precision storage path -- conv precision "f16", h8 tensors
[N, G, H, W, 8] fp16 from the stem's input to the last conv's output -- and the kernels it adds (csrc/fpn_h8.hip, the (2,1,1) conv family,
conv_h8_late_kernel).

Bars.  Data movement: bit-exact on fp16-representable inputs.  Convs: the project's h8 bar 2^-10 |y| + 1e-4 max(1, max|y| / 30) against F.conv2d
on the same fp16-rounded operands.  Attention: 2^-10 |y| + 1e-6.  Model: against the fp32 oracle with a bar from a CPU EMULATION of fp16 storage
(`emulated_fp16_storage`: the oracle with BN-folded fp16 weights, fp16 inputs and every stored tensor rounded to fp16), never from the code under
test: with E the emulation's error and Fl its argmax-flip share, max|y - want| <= max(1e-3 max(1, max|want|), 3 E) and flips <= 3 Fl + 1e-3
(the factor 3: accumulation order and the one-ulp differences it propagates)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import fpn as ofpn
from semanticlidarunc_amd import _lib, h8, ops, salsanext as sn
from semanticlidarunc_amd.fpn import SemanticNetworkWithFPN
from semanticlidarunc_amd.testing import randomize_bn_

pytestmark = pytest.mark.gpu


def r16(t):
    return t.half().float()


def _rand16(g, *shape, scale=1.0):
    return r16(torch.randn(*shape, generator=g) * scale)


def _h8_bar(err, want):
    return bool((err <= 2.0 ** -10 * want.abs() + 1e-4 * max(1.0, float(want.abs().max()) / 30)).all())


def _check_conv(got_h8, want, tag):
    """got_h8 [N, G, H, W, 8] against fp32 NCHW `want` at the h8 conv bar; pad channels exactly 0"""
    c = want.shape[1]
    full = h8.from_h8(got_h8).cpu()
    assert bool((full[:, c:] == 0).all()), tag
    err = (full[:, :c] - want).abs()
    print(f"{tag}: max err {float(err.max()):.3e}, max |want| {float(want.abs().max()):.3f}")
    assert _h8_bar(err, want), (tag, float(err.max()))


@pytest.fixture
def f16_precision():
    sn.set_conv_precision("f16")
    yield
    sn.set_conv_precision("fp32")


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. data movement, bit-exact
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 20, 12, 40), (1, 5, 7, 37)])
def test_maxpool_bit_exact_and_padding_is_minus_inf(cuda, shape):
    g = torch.Generator().manual_seed(11)
    x = r16(-(torch.randn(*shape, generator=g).abs() + 0.5))    # all negative: a zero pad tap would win every border maximum
    got = h8.maxpool3s2_h8(h8.to_h8(x.to(cuda)))
    want = F.max_pool2d(x, 3, 2, 1)
    assert tuple(got.shape) == (shape[0], (shape[1] + 7) // 8, (shape[2] + 1) // 2, (shape[3] + 1) // 2, 8)
    full = h8.from_h8(got).cpu()
    assert torch.equal(full[:, :shape[1]], want) and float(want.max()) < 0
    assert bool((full[:, shape[1]:] == 0).all())                # pad channels stay 0


@pytest.mark.parametrize("m,f", [(0, 1)] + [(m, f) for m in (3, 6, 8) for f in (2, 4, 8)])
def test_space_to_depth_with_meta_injection_bit_exact(cuda, m, f):
    g = torch.Generator().manual_seed(12)
    x = _rand16(g, 2, 64, 12, 40)
    xin, meta = x, None
    if m:
        meta = _rand16(g, 2, m, 12 * f, 40 * f, scale=30.0)
        xin = torch.cat([x[:, :-m], F.interpolate(meta, scale_factor=1 / f, mode="nearest")], 1)      # ops.space_to_depth2_cat's input
    y, y00 = h8.space_to_depth2_h8(h8.to_h8(x.to(cuda)), None if meta is None else meta.to(cuda), 64, f)
    assert tuple(y.shape) == (2, 32, 6, 20, 8) and tuple(y00.shape) == (2, 8, 6, 20, 8)
    y, y00 = h8.from_h8(y).cpu(), h8.from_h8(y00).cpu()
    for p in (0, 1):
        for q in (0, 1):
            assert torch.equal(y[:, (2 * p + q) * 64:(2 * p + q + 1) * 64], xin[:, :, p::2, q::2]), (p, q)
    assert torch.equal(y00, xin[:, :, ::2, ::2])
    if m:                                                        # the same thing the fp32 path's kernel computes
        ref = ops.space_to_depth2_cat(x.to(cuda), 64 - m, ops.nearest_down(meta.to(cuda), f)).cpu()
        assert torch.equal(y, ref)


def test_depth_to_space_into_slices_of_one_buffer(cuda, f16_precision):
    g = torch.Generator().manual_seed(13)
    torch.manual_seed(0)
    m = SemanticNetworkWithFPN("resnet18", 2, 3, num_classes=5).to(cuda).eval()
    n, hh, ww = 2, 16, 48
    pattern = (torch.arange(n * 12 * hh * ww * 8, dtype=torch.float32) % 1021 - 510).reshape(n, 12, hh, ww, 8).half().to(cuda)
    for name, ct, g_off in (("up2", m.upsample_layer_x2, 0), ("up3", m.upsample_layer_x3, 4), ("up4", m.upsample_layer_x4, 8)):
        s = ct.stride[0]
        fin = _rand16(g, n, ct.in_channels, hh // s, ww // s)
        ups = pattern.clone()
        m._up_h8("t." + name, ct, h8.to_h8(fin.to(cuda)), ups, g_off)
        others = [b for b in range(12) if not g_off <= b < g_off + 4]
        assert torch.equal(ups[:, others], pattern[:, others]), name          # the other slices: bit-identical
        want = F.conv_transpose2d(fin, r16(ct.weight.detach().cpu()), ct.bias.detach().cpu(), stride=s)
        _check_conv(ups[:, g_off:g_off + 4].contiguous(), want, name)


@pytest.mark.parametrize("classes", [3, 20])
def test_last_depth_to_space_with_elu_plus_one(cuda, classes):
    g = torch.Generator().manual_seed(14)
    y = _rand16(g, 2, 4 * classes, 5, 37, scale=2.0)
    got = h8.depth_to_space_h8(h8.to_h8(y.to(cuda)), 2, elu_plus_one=True, classes=classes).cpu()
    want = F.elu(F.pixel_shuffle(y, 2)) + 1
    assert got.shape == want.shape and got.dtype == torch.float32
    assert float((got - want).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. convs
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage,shape,m,f", [("layer2", (2, 64, 16, 80), 0, 2), ("layer2", (2, 64, 16, 80), 6, 2),
                                             ("layer4", (1, 256, 8, 32), 0, 8), ("layer4", (1, 256, 8, 32), 3, 8)])
def test_stride2_conv_as_2x2_conv_of_space_to_depth(cuda, f16_precision, stage, shape, m, f):
    """3x3 / s2 (64 -> 128: output W = 40, a ragged 64-column tile; 256 -> 512) and the 1x1 / s2 downsample on phase (0,0)"""
    g = torch.Generator().manual_seed(21)
    torch.manual_seed(0)
    model = randomize_bn_(SemanticNetworkWithFPN("resnet18", 2, max(m, 1), num_classes=5), 3).to(cuda).eval()
    blk = getattr(model, stage)[0]
    x = _rand16(g, *shape)
    xin, meta = x, None
    if m:
        meta = _rand16(g, shape[0], m, shape[2] * f, shape[3] * f, scale=10.0)
        xin = torch.cat([x[:, :-m], F.interpolate(meta, scale_factor=1 / f, mode="nearest")], 1)
    s2d, x00 = h8.space_to_depth2_h8(h8.to_h8(x.to(cuda)), None if meta is None else meta.to(cuda), shape[1], f)
    got = model._run_h8(model._p_conv_s2("t.conv1", blk.conv1, blk.bn1, shape[1]), [s2d])
    w, b = model._fold(blk.conv1.weight, blk.conv1.bias, blk.bn1)
    _check_conv(got, F.relu(F.conv2d(xin, r16(w.cpu()), b.cpu(), stride=2, padding=1)), f"{stage} 3x3/s2 m={m}")
    got = model._run_h8(model._p_conv("t.down", blk.downsample[0], blk.downsample[1]), [x00], relu=False)
    w, b = model._fold(blk.downsample[0].weight, None, blk.downsample[1])
    _check_conv(got, F.conv2d(xin, r16(w.cpu()), b.cpu(), stride=2), f"{stage} 1x1/s2 m={m}")


@pytest.mark.parametrize("c,shape", [(64, (2, 16, 80)), (512, (1, 2, 5)), (128, (3, 9, 70))])
def test_late_activation(cuda, c, shape):
    """out = relu(conv + bias + resid); 64 -> 64 is the shape the ring kernel would take if the flag were ignored"""
    g = torch.Generator().manual_seed(22)
    n, hh, ww = shape
    x, w = _rand16(g, n, c, hh, ww), _rand16(g, c, c, 3, 3, scale=(9 * c) ** -0.5)
    bias, r = torch.randn(c, generator=g) * 0.1, _rand16(g, n, c, hh, ww)
    pre = F.conv2d(x, w, bias, padding=1) + r
    assert 0.3 < float((pre < 0).float().mean()) < 0.7          # about half the sums are negative
    got = h8.conv2d_h8([h8.H8Source(h8.to_h8(x.to(cuda)))], h8.pack_conv_weight_h8(w.to(cuda)), c, c, 3, 1, 1, bias=bias.to(cuda), slope=0.0,
                       resid=h8.to_h8(r.to(cuda)), act_after_resid=True)
    _check_conv(got, F.relu(pre), f"late {c}")


def _kernel_name(srcs, cout, k, dil, pad, n, h, w, resid, late):
    d = _lib.ConvH8Desc()
    for i, c in enumerate(srcs):
        d.src[i].ptr, d.src[i].G = 1 << 20, c // 8
    d.nsrc, d.N, d.H, d.W, d.Cout, d.ksize, d.dil, d.pad = len(srcs), n, h, w, cout, k, dil, pad
    d.wpack = d.bias = d.out = 1 << 20
    d.resid, d.has_act, d.act_after_resid = (1 << 20) if resid else None, 1, 1 if late else 0
    buf = C.create_string_buffer(96)
    assert _lib.load().slu_conv2d_h8_kernel_name(C.byref(d), buf, 96) == 0
    return buf.value.decode()


# one shape per tile configuration the dispatch can pick beyond the small ones above (>= 256 workgroups of that tile), named so that a dispatch
# change that stops covering an instantiation shows: <MB, WM, WN, RPW, ..., OPT, ONE>
@pytest.mark.parametrize("srcs,shape,args", [
    ((128,), (4, 64, 512), "2, 2, 4, 2, false, false, false, 1, 15, true"),      # 128-channel configuration, whole records on the way out
    ((64, 64), (4, 64, 512), "2, 2, 4, 2, false, false, false, 1, 0, false"),    # ... its two-source form
    ((128,), (1, 32, 2048), "2, 2, 2, 2, false, false, false, 1, 0, false"),
    ((64,), (1, 64, 4096), "2, 1, 8, 2, false, false, false, 1, 0, false"),
    ((64,), (1, 32, 4096), "2, 1, 4, 2, false, false, false, 1, 0, false"),
    ((32,), (1, 64, 4096), "1, 1, 8, 2, false, false, false, 1, 0, false"),
    ((32,), (1, 32, 4096), "1, 1, 4, 2, false, false, false, 1, 0, false")])
def test_late_activation_in_every_tile_configuration(cuda, srcs, shape, args):
    g = torch.Generator().manual_seed(24)
    n, hh, ww = shape
    c = sum(srcs)
    assert _kernel_name(srcs, c, 3, 1, 1, n, hh, ww, True, True) == f"conv_h8_late_kernel<3, 1, 1, {args}>"
    x, w = _rand16(g, n, c, hh, ww), _rand16(g, c, c, 3, 3, scale=(9 * c) ** -0.5)
    bias, r = torch.randn(c, generator=g) * 0.1, _rand16(g, n, c, hh, ww)
    xs, c0 = [], 0
    for cs in srcs:
        xs.append(h8.H8Source(h8.to_h8(x[:, c0:c0 + cs].contiguous().to(cuda))))
        c0 += cs
    got = h8.conv2d_h8(xs, h8.pack_conv_weight_h8(w.to(cuda)), c, c, 3, 1, 1, bias=bias.to(cuda), slope=0.0, resid=h8.to_h8(r.to(cuda)),
                       act_after_resid=True)
    _check_conv(got, F.relu(F.conv2d(x, w, bias, padding=1) + r), f"late {srcs} {shape}")


@pytest.mark.parametrize("cin,cout,shape,args", [
    (64, 128, (4, 64, 512), "2, 2, 4, 2, false, false, false, 1, 15, true"),
    (64, 128, (1, 32, 2048), "2, 2, 2, 2, false, false, false, 1, 0, false"),
    (64, 64, (1, 64, 4096), "2, 1, 8, 2, false, false, false, 1, 0, false"),
    (16, 32, (1, 64, 4096), "1, 1, 8, 2, false, true, false, 1, 0, false"),      # weights resident in LDS
    (12, 20, (2, 9, 70), "1, 1, 4, 1, false, true, false, 1, 0, false")])        # pad channels on both sides
def test_2x2_conv_with_taps_at_minus_one_and_zero(cuda, cin, cout, shape, args):
    """the (2,1,1) family on its own: out[y, x] = sum_ab w[a, b] x[y - 1 + a, x - 1 + b]"""
    g = torch.Generator().manual_seed(25)
    n, hh, ww = shape
    assert _kernel_name((8 * ((cin + 7) // 8),), cout, 2, 1, 1, n, hh, ww, False, False) == f"conv_h8_kernel<2, 1, 1, {args}>"
    x, w, bias = _rand16(g, n, cin, hh, ww), _rand16(g, cout, cin, 2, 2, scale=(4 * cin) ** -0.5), torch.randn(cout, generator=g) * 0.1
    got = h8.conv2d_h8([h8.H8Source(h8.to_h8(x.to(cuda)))], h8.pack_conv_weight_h8(w.to(cuda)), cin, cout, 2, 1, 1, bias=bias.to(cuda), slope=0.0)
    _check_conv(got, F.relu(F.conv2d(F.pad(x, (1, 0, 1, 0)), w, bias)), f"(2,1,1) {cin}->{cout} {shape}")


def test_late_activation_is_refused_where_it_is_not_built(cuda):
    g = torch.Generator().manual_seed(23)
    x, r = h8.to_h8(_rand16(g, 1, 64, 8, 64).to(cuda)), h8.to_h8(_rand16(g, 1, 64, 8, 64).to(cuda))
    for k, dil, pad in ((1, 1, 0), (3, 2, 2)):
        w = h8.pack_conv_weight_h8(_rand16(g, 64, 64, k, k).to(cuda))
        h8.conv2d_h8([h8.H8Source(x)], w, 64, 64, k, dil, pad, slope=0.0, resid=r)              # fine without the flag
        with pytest.raises(RuntimeError):
            h8.conv2d_h8([h8.H8Source(x)], w, 64, 64, k, dil, pad, slope=0.0, resid=r, act_after_resid=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. attention
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,c,hh,ww", [(2, 32, 3, 300), (1, 256, 2, 8), (1, 64, 2, 2048)])
def test_attention_row(cuda, n, c, hh, ww):
    g = torch.Generator().manual_seed(31)
    tv = _rand16(g, n, 2 * c, hh, ww)
    w_a, b_a = torch.randn(c, generator=g) * 3 / c ** 0.5, torch.randn(1, generator=g)      # scores of spread 3: a peaked softmax
    got = h8.from_h8(h8.attention_row_h8(h8.to_h8(tv.to(cuda)), w_a.to(cuda), b_a.to(cuda))).cpu()
    s = (torch.tanh(tv[:, :c]) * w_a.view(1, c, 1, 1)).sum(1, keepdim=True) + b_a
    want = tv[:, c:] * torch.softmax(s, -1)
    err = (got - want).abs()
    print(f"attention C={c} W={ww}: max err {float(err.max()):.3e}, score spread {float(s.std()):.2f}, max p {float(torch.softmax(s, -1).max()):.3f}")
    assert bool((err <= 2.0 ** -10 * want.abs() + 1e-6).all()), float(err.max())


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the model against the fp32 oracle, bar from a CPU emulation of fp16 storage
# ------------------------------------------------------------------------------------------------------------------------------------
def emulated_fp16_storage(sd, x, meta, backbone, attention=True, multi_scale_meta=True, emulate=True):
    """(output, largest |value| of a stored tensor) of oracle.fpn.fpn_forward.  emulate: with what the h8 path rounds to fp16 rounded -- conv
    weights after BatchNorm folding (the attention's W_q + W_k as one matrix), the inputs, and every tensor it stores: ReLU outputs (stem, blocks,
    FPN, decoder), the down-sample branch, an attention's conv outputs (q + k, v) and its result, ConvTranspose outputs (the last conv's
    included).  emulate=False: the plain fp32 oracle, which only records the peak."""
    peak = [0.0]

    def store(t):
        peak[0] = max(peak[0], float(t.abs().max()))
        return r16(t) if emulate else t

    sd = {k: v.clone().float() if v.is_floating_point() else v.clone() for k, v in sd.items()}
    if emulate:
        for k in [k for k in sd if k.endswith(".running_var")]:          # fold every BatchNorm that follows a conv into it
            bn = k[:-len(".running_var")]
            if bn == "backbone.bn1" or not bn.startswith(("backbone.layer", "fpn_block", "decoder_semantic")):
                continue                                                 # (backbone.bn1 is unused; layerN.* / stem.* alias backbone.*)
            head, idx = bn.rsplit(".", 1)
            conv = {"bn1": head + ".conv1", "bn2": head + ".conv2"}.get(idx, f"{head}.{int(idx) - 1}" if idx.isdigit() else None)
            a = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + 1e-5)
            b = sd[bn + ".bias"] - sd[bn + ".running_mean"] * a
            if conv + ".bias" in sd:
                b = b + sd[conv + ".bias"] * a
                sd[conv + ".bias"] = torch.zeros_like(sd[conv + ".bias"])
            sd[conv + ".weight"] = sd[conv + ".weight"] * a.view(-1, 1, 1, 1)
            sd[bn + ".weight"], sd[bn + ".bias"] = torch.ones_like(a), b
            sd[bn + ".running_mean"], sd[bn + ".running_var"] = torch.zeros_like(a), torch.full_like(a, 1.0 - 1e-5)
        for k in sd:
            # (the score weights stay fp32; W_q + W_k is rounded as one matrix below)
            if k.endswith(".weight") and sd[k].dim() == 4 and not k.endswith(("attention_conv.weight", "query_conv.weight", "key_conv.weight")):
                sd[k] = r16(sd[k])
        x, meta = r16(x), r16(meta)

    real = (ofpn.F.relu, ofpn.F.conv_transpose2d, ofpn._bn, ofpn._attention)

    def bn(t, sd_, p):
        y = real[2](t, sd_, p)
        return store(y) if p.endswith("downsample.1") else y

    def att(t, sd_, p):
        if not emulate:
            return store(real[3](t, sd_, p))
        qk = store(F.conv2d(t, r16(sd_[p + ".query_conv.weight"] + sd_[p + ".key_conv.weight"]), sd_[p + ".query_conv.bias"] + sd_[p + ".key_conv.bias"]))
        v = store(F.conv2d(t, sd_[p + ".value_conv.weight"], sd_[p + ".value_conv.bias"]))
        s = F.conv2d(torch.tanh(qk), sd_[p + ".attention_conv.weight"], sd_[p + ".attention_conv.bias"])
        return store(v * torch.softmax(s, dim=-1))

    ofpn.F.relu = lambda t, *a, **k: store(real[0](t, *a, **k))
    ofpn.F.conv_transpose2d = lambda *a, **k: store(real[1](*a, **k))
    ofpn._bn, ofpn._attention = bn, att
    try:
        with torch.no_grad():
            y = ofpn.fpn_forward(sd, x, meta, backbone=backbone, attention=attention, multi_scale_meta=multi_scale_meta)
    finally:
        ofpn.F.relu, ofpn.F.conv_transpose2d, ofpn._bn, ofpn._attention = real
    return y, peak[0]


def ouster_like_scan(batch, h, w, seed, max_range=120.0):
    """x = (range, reflectivity), meta = (xyz, unit normals) at Ouster magnitudes: range up to 120 m with a heavy tail, 10 % empty returns"""
    g = torch.Generator().manual_seed(seed)
    rng = torch.exp(torch.randn(batch, 1, h, w, generator=g) * 0.9 + 2.3).clamp(0.5, max_range)
    az = torch.linspace(-3.1416, 3.1416, w).view(1, 1, 1, w).expand(batch, 1, h, w)
    el = torch.linspace(0.39, -0.39, h).view(1, 1, h, 1).expand(batch, 1, h, w)
    xyz = torch.cat([rng * torch.cos(el) * torch.cos(az), rng * torch.cos(el) * torch.sin(az), rng * torch.sin(el)], 1)
    nrm = F.normalize(torch.randn(batch, 3, h, w, generator=g), dim=1)
    empty = torch.rand(batch, 1, h, w, generator=g) < 0.10
    x = torch.cat([rng, torch.rand(batch, 1, h, w, generator=g)], 1).masked_fill(empty, 0.0)
    return x.contiguous(), torch.cat([xyz, nrm], 1).masked_fill(empty, 0.0).contiguous()


_CASES = {
    "golden_resnet18_m6_c20": dict(kw=dict(backbone="resnet18", input_channels=2, meta_channel_dim=6, num_classes=20), golden="fpn_resnet18_m6_c20"),
    "golden_resnet34_m3_c3_noatt": dict(kw=dict(backbone="resnet34", input_channels=2, meta_channel_dim=3, num_classes=3, attention=False,
                                                multi_scale_meta=False), golden="fpn_resnet34_m3_c3_noatt"),
    "resnet18_randn_2x48x80": dict(kw=dict(backbone="resnet18", input_channels=2, meta_channel_dim=6, num_classes=20), shape=(2, 48, 80)),
    "resnet18_ouster_1x128x512": dict(kw=dict(resnet_type="resnet18", meta_channel_dim=6, num_classes=20), ouster=(1, 128, 512)),
}


@pytest.mark.parametrize("case", list(_CASES))
def test_model_against_fp32_oracle_with_emulated_bar(cuda, case):
    c = _CASES[case]
    kw = c["kw"]
    torch.manual_seed(0)
    model = randomize_bn_(SemanticNetworkWithFPN(**kw), 3).eval()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if "golden" in c:
        gd = golden(c["golden"])
        s = sum(float(v.double().sum()) for v in sd.values() if v.is_floating_point())
        a = sum(float(v.double().abs().sum()) for v in sd.values() if v.is_floating_point())
        assert np.allclose([s, a], gd["sd_digest"], rtol=1e-10)
        x, meta = torch.from_numpy(np.asarray(gd["x"])), torch.from_numpy(np.asarray(gd["meta"]))
    elif "ouster" in c:
        x, meta = ouster_like_scan(*c["ouster"], seed=5)
    else:
        g = torch.Generator().manual_seed(3)
        n, hh, ww = c["shape"]
        x, meta = torch.randn(n, 2, hh, ww, generator=g), torch.randn(n, 6, hh, ww, generator=g)
    okw = dict(backbone=kw.get("backbone", kw.get("resnet_type")), attention=kw.get("attention", True), multi_scale_meta=kw.get("multi_scale_meta", True))
    want, peak = emulated_fp16_storage(sd, x, meta, emulate=False, **okw)
    if "golden" in c:
        assert float((want - torch.from_numpy(np.asarray(gd["out"]))).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))      # the oracle is the reference
    emu, _ = emulated_fp16_storage(sd, x, meta, emulate=True, **okw)
    scale = max(1.0, float(want.abs().max()))
    E = float((emu - want).abs().max())
    Fl = float((emu.argmax(1) != want.argmax(1)).float().mean())
    assert E <= 2e-3 * scale, f"unsuitable fixture: the emulation itself is {E:.2e} from the oracle"
    model.to(cuda)
    sn.set_conv_precision("f16")
    try:
        with torch.no_grad():
            y = model(x.to(cuda), meta.to(cuda)).cpu()
    finally:
        sn.set_conv_precision("fp32")
    err = float((y - want).abs().max())
    flips = float((y.argmax(1) != want.argmax(1)).float().mean())
    print(f"{case}: output scale {scale:.3f}, HIP f16 err {err:.3e} (emulation E {E:.3e}), flips {flips:.2e} (emulation {Fl:.2e}), stored peak {peak:.1f}")
    assert y.shape == want.shape and y.dtype == torch.float32 and bool(torch.isfinite(y).all()) and float(y.min()) >= 0
    if "ouster" in c:
        assert peak < 65504.0 / 16.0, f"largest stored activation {peak:.0f}"
    assert err <= max(1e-3 * scale, 3 * E), (err, E)
    assert flips <= 3 * Fl + 1e-3, (flips, Fl)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. it really is the h8 path; 6. refusals and unchanged paths
# ------------------------------------------------------------------------------------------------------------------------------------
def _small_model(cuda, backbone="resnet18"):
    torch.manual_seed(0)
    model = randomize_bn_(SemanticNetworkWithFPN(backbone, 2, 3, num_classes=5), 3).to(cuda).eval()
    g = torch.Generator().manual_seed(4)
    return model, torch.randn(1, 2, 32, 64, generator=g).to(cuda), torch.randn(1, 3, 32, 64, generator=g).to(cuda)


def test_f16_forward_runs_on_h8_kernels_only_and_the_cache_follows_precision_and_weights(cuda, monkeypatch):
    model, x, meta = _small_model(cuda)
    with torch.no_grad():
        y32 = model(x, meta)
        sn.set_conv_precision("f16")
        try:
            with monkeypatch.context() as mp:
                mp.setattr(ops, "conv2d_fused", lambda *a, **k: (_ for _ in ()).throw(AssertionError("fp32-storage conv on the f16 path")))
                y16 = model(x, meta)
                packed = {k: v.wpack.data_ptr() for k, v in model._packed.items()}
                assert torch.equal(model(x, meta), y16)
                assert packed == {k: v.wpack.data_ptr() for k, v in model._packed.items()}      # nothing re-packed per call
            assert not torch.equal(y16, y32)
            sn.set_conv_precision("fp32")
            assert torch.equal(model(x, meta), y32)              # the cache is keyed by precision
            sn.set_conv_precision("f16")
            model.fpn_block1[0].weight.mul_(1.5)                 # in place: the parameter's version moves
            model.layer3[0].bn1.running_var.mul_(0.5)
            y_new = model(x, meta)
            fresh = copy.deepcopy(model)
            fresh.__dict__.pop("_packed", None)
            assert not torch.equal(y_new, y16) and torch.equal(y_new, fresh(x, meta))
        finally:
            sn.set_conv_precision("fp32")


def test_resnet50_refuses_f16_and_training_is_untouched(cuda, f16_precision):
    model, x, meta = _small_model(cuda, "resnet50")
    with torch.no_grad(), pytest.raises(RuntimeError, match="'f16'"):
        model(x, meta)
    model, x, meta = _small_model(cuda)
    model.train()
    with torch.no_grad():
        y16 = model(x, meta)
        sn.set_conv_precision("fp32")
        y32 = model(x, meta)
    assert torch.equal(y16, y32)                                 # _wants_autograd routes to the training path whatever the precision
