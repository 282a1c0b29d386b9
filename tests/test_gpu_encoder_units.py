"""GPU: what the encoder unit kernels share (csrc/encoder_unit.h) -- the packed weight images bit for bit against the numpy restatement of the
layout include/slu.h documents (tests/afrag_restatement.py), the two-source input with a channel offset in the pool and the sampling (Fire and
the tail have it in their own files), and the overlap rule of every entry point that takes a slu_cat2.

Bars: exact equality everywhere -- the images and the two data-movement kernels copy fp32 values."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import afrag_restatement as A
from semanticlidarunc_amd import _lib, ops

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------- 1. the packed weight images ----------------
@pytest.mark.parametrize("co,c", A.SHUFFLE_SHAPES, ids=[f"{co}x{c}" for co, c in A.SHUFFLE_SHAPES])
def test_shuffle_tail_image_is_the_documented_layout(cuda, co, c):
    w = A.shuffle_weight(co, c)
    got = ops.pack_shuffle_tail_weight(torch.from_numpy(w).to(cuda)).cpu().numpy()
    assert _same_bits(got, A.shuffle_tail_image(w))


@pytest.mark.parametrize("cin,s,e1,e3", A.FIRE_SHAPES, ids=[f"{c[0]}_s{c[1]}_e{c[2]}+{c[3]}" for c in A.FIRE_SHAPES])
def test_fire_image_is_the_documented_layout(cuda, cin, s, e1, e3):
    wsq, w1, w3 = A.fire_weights(cin, s, e1, e3)
    got = ops.pack_fire_weight(*(torch.from_numpy(t).to(cuda) for t in (wsq, w1, w3))).cpu().numpy()
    assert _same_bits(got, A.fire_image(wsq, w1, w3))


# ---------------- 2. two sources, the first one read from a channel offset ----------------
def _wide(h, w):
    """x [2, 5, h, w] = the concatenation; (a 5 + 3 + 2-channel first tensor whose unread channels are NaN, the 2-channel second source)"""
    x = torch.randn(2, 5, h, w, generator=torch.Generator().manual_seed(10 * h + w))
    first = torch.cat([torch.full((2, 5, h, w), NAN), x[:, :3], torch.full((2, 2, h, w), NAN)], 1)
    return x, first, x[:, 3:].contiguous()


@pytest.mark.parametrize("h,w", [(5, 7), (3, 3)])
def test_ceil_pool_reads_a_channel_range_and_a_second_source(cuda, h, w):
    x, first, second = _wide(h, w)
    got = ops.maxpool3s2_ceil(first.to(cuda), coff=5, cuse=3, src2=second.to(cuda)).cpu()
    assert torch.equal(got, F.max_pool2d(x, 3, 2, 0, ceil_mode=True))


def test_sample2_reads_a_channel_range_and_a_second_source(cuda):
    x, first, second = _wide(5, 7)
    got = ops.regnet_sample2(first.to(cuda), 5, 3, second.to(cuda)).cpu()
    assert torch.equal(got, x[:, :, ::2, ::2])


# ---------------- 3. out must not overlap an input ----------------
# Every buffer that a refused call names holds a random pattern and is compared with its copy after a synchronize: a launch on aliased buffers
# would have rewritten it.  Each buffer is as large as both of its roles, so even a launch would stay inside it.
def _pattern(cuda, *shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(cuda)


def _unchanged(pairs):
    torch.cuda.synchronize()
    return all(torch.equal(t, before) for t, before in pairs)


def test_tail_refuses_an_aliased_out(cuda):
    n, h, w, co = 1, 4, 8, 12
    a, b, o = (_pattern(cuda, n, 2 * co, h, w, seed=s) for s in (1, 2, 3))      # src (8 of its channels read), src2, out / pass-through: one shape
    c = 8 + 2 * co
    wdw, bdw, wpw, bpw = _pattern(cuda, c, 9, seed=4), _pattern(cuda, c, seed=5), _pattern(cuda, co, c, seed=6), _pattern(cuda, co, seed=7)
    wpack = ops.pack_shuffle_tail_weight(wpw)
    lib = _lib.load()
    d = _lib.ShuffleTailDesc()
    d.src0, d.ct0, d.c0, d.src1, d.ct1, d.c1 = a.data_ptr(), 2 * co, 8, b.data_ptr(), 2 * co, 2 * co
    d.N, d.H, d.W, d.stride, d.Co, d.parity = n, h, w, 1, co, 1
    d.wdw, d.bdw, d.wpack, d.bpw = wdw.data_ptr(), bdw.data_ptr(), wpack.data_ptr(), bpw.data_ptr()
    d.out = o.data_ptr()
    assert lib.slu_shuffle_tail_fwd(ctypes.byref(d), None) == 0                  # the descriptor itself is fine
    kept = [(t, t.clone()) for t in (a, b, o)]
    for out in (a, b):                                                           # out == src0, out == src1
        d.out = out.data_ptr()
        assert lib.slu_shuffle_tail_fwd(ctypes.byref(d), None) == -1
        with pytest.raises(RuntimeError, match="overlap"):
            ops.shuffle_tail(a, wdw, bdw, wpack, bpw, co, 1, out=out, cuse=8, src2=b)
    d.out, d.pass_, d.pass_ct = o.data_ptr(), o.data_ptr(), 2 * co               # pass == out
    assert lib.slu_shuffle_tail_fwd(ctypes.byref(d), None) == -1
    with pytest.raises(RuntimeError, match="overlap"):
        ops.shuffle_tail(a, wdw, bdw, wpack, bpw, co, 1, out=o, cuse=8, src2=b, passthrough=o)
    assert _unchanged(kept)
    with pytest.raises(RuntimeError):
        ops.shuffle_tail(a, wdw[:8].contiguous(), bdw[:8].contiguous(), ops.pack_shuffle_tail_weight(wpw[:, :8].contiguous()), bpw, co, 1, cuse=8,
                         src2=torch.empty(n, 0, h, w, device=cuda))              # an empty second source


def test_fire_refuses_an_aliased_out(cuda):
    n, h, w, s, e = 1, 4, 8, 16, 32
    a, b, o = (_pattern(cuda, n, 2 * e, h, w, seed=s_) for s_ in (1, 2, 3))      # src (16 of its channels read), src2, out: one shape
    cin = 16 + 2 * e
    wpack = ops.pack_fire_weight(_pattern(cuda, s, cin, seed=4), _pattern(cuda, e, s, seed=5), _pattern(cuda, e, s, 3, 3, seed=6))
    bsq, b1, b3 = _pattern(cuda, s, seed=7), _pattern(cuda, e, seed=8), _pattern(cuda, e, seed=9)
    lib = _lib.load()
    d = _lib.FireDesc()
    d.src0, d.ct0, d.c0, d.src1, d.ct1, d.c1 = a.data_ptr(), 2 * e, 16, b.data_ptr(), 2 * e, 2 * e
    d.N, d.H, d.W, d.S, d.E1, d.E3 = n, h, w, s, e, e
    d.wpack, d.bsq, d.b1, d.b3, d.out = wpack.data_ptr(), bsq.data_ptr(), b1.data_ptr(), b3.data_ptr(), o.data_ptr()
    assert lib.slu_fire_fwd(ctypes.byref(d), None) == 0
    kept = [(t, t.clone()) for t in (a, b, o)]
    for out in (a, b):
        d.out = out.data_ptr()
        assert lib.slu_fire_fwd(ctypes.byref(d), None) == -1
        with pytest.raises(RuntimeError, match="overlap"):
            ops.fire(a, wpack, bsq, b1, b3, out=out, cuse=16, src2=b)
    assert _unchanged(kept)


@pytest.mark.parametrize("entry", ["slu_maxpool3s2_ceil_fwd", "slu_regnet_sample2"])
def test_pool_and_sampling_refuse_an_aliased_out(cuda, entry):
    """ops.maxpool3s2_ceil and ops.regnet_sample2 allocate their output themselves, so only the library can be handed an aliased one."""
    n, h, w = 2, 5, 7
    a, b = _pattern(cuda, n, 6, h, w, seed=1), _pattern(cuda, n, 4, h, w, seed=2)
    cat = _lib.Cat2(a.data_ptr(), b.data_ptr(), 6, 1, 3, 4, 4)
    fn = getattr(_lib.load(), entry)
    x = torch.cat([a[:, 1:4], b], 1)
    want = x[:, :, ::2, ::2] if entry == "slu_regnet_sample2" else F.max_pool2d(x, 3, 2, 0, ceil_mode=True)
    y = torch.empty(want.shape, device=cuda)
    assert fn(ctypes.byref(cat), y.data_ptr(), n, h, w, None) == 0
    assert torch.equal(y, want)
    kept = [(t, t.clone()) for t in (a, b)]
    for out in (a, b):                                                           # both hold more floats than the output
        assert out.numel() >= y.numel()
        assert fn(ctypes.byref(cat), out.data_ptr(), n, h, w, None) == -1
    assert _unchanged(kept)
