"""CPU: the conv dispatch, asked for names.  slu_conv2d_h8_kernel_name / slu_conv2d_kernel_name / slu_conv_tail_h8_kernel_name walk the
dispatch of their launch with a leaf that prints its template arguments instead of launching, so they need no GPU: every row of the
case tables of test_gpu_dispatch_coverage.py must select the instantiation it names from a descriptor with placeholder addresses, and
a descriptor the launch refuses must get the launch's status.  A dispatch edit that loses an instantiation fails here, before a GPU run."""
import ctypes as C
import os

import pytest

from semanticlidarunc_amd import _lib
from test_gpu_dispatch_coverage import F16X3_CASES, FP32_CASES, H8_CASES, _id

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libslu_hip.so not built")
PTR = 0x10000          # non-null, 16-byte aligned; name mode never dereferences it
SLU_EUNSUPPORTED = -2


def _name(fn, desc, n=96):
    buf = C.create_string_buffer(n)
    rc = getattr(_lib.load(), fn)(C.byref(desc), buf, n)
    return rc, buf.value.decode()


def _h8_desc(fam, parts, cout, n, h, w, scales=False, resid=True, out_f32=False, nbatch_last=0, bias=True, bn=True, act=True, big=False,
             late=False, shuffle=False):
    """The descriptor test_gpu_h8._conv_case hands to h8.conv2d_h8 for these options.  late: the activation after the residual add
    (act_after_resid); shuffle: source 0 is read through PixelShuffle in place (4x the stored blocks, at half the size)."""
    d = _lib.ConvH8Desc()
    for i, c in enumerate(parts):
        g = (c + 7) // 8
        nb = nbatch_last if (nbatch_last and i == len(parts) - 1 and i > 0 and nbatch_last != n) else 0
        d.src[i].ptr, d.src[i].scale, d.src[i].G, d.src[i].nbatch = PTR, PTR if scales else None, g, nb
    d.nsrc = len(parts)
    d.N, d.H, d.W, d.Cout = n, h, w, cout
    d.ksize, d.dil, d.pad = fam
    d.wpack, d.bias = PTR, PTR if bias else None
    d.has_act, d.slope = (1, 0.01) if act else (0, 0.0)
    d.bn_a = d.bn_b = PTR if bn else None
    d.resid, d.out = PTR if (resid and not out_f32) else None, PTR
    d.out_f32_nchw = 1 if out_f32 else 0
    d.act_after_resid = 1 if late else 0
    if shuffle:
        d.src[0].G, d.src[0].shuffle = 4 * d.src[0].G, 1
    return d


def _conv_desc(precision, fam, parts, cout, n, h, w, scales=False, resid=True, bias=True, bn=True, act=True, stats=False, big=False):
    """The descriptor test_gpu_conv._run / test_gpu_f16x3._run hand to ops.conv2d_fused for these options."""
    d = _lib.ConvDesc()
    for i, c in enumerate(parts):
        d.src[i].ptr, d.src[i].scale, d.src[i].C = PTR, PTR if scales else None, c
    d.nsrc = len(parts)
    d.N, d.H, d.W, d.Cin, d.Cout = n, h, w, sum(parts), cout
    d.ksize, d.dil, d.pad = fam
    d.ck = 16 if precision == "f16x3" or fam[0] == 1 else 8
    d.wpack, d.bias = PTR, PTR if bias else None
    d.has_act, d.slope = (1, 0.01) if act else (0, 0.0)
    d.bn_a = d.bn_b = PTR if bn else None
    d.resid, d.out = PTR if resid else None, PTR
    d.precision = {"fp32": 0, "f16x3": 1}[precision]
    d.stats = PTR if stats else None
    return d


@pytest.mark.parametrize("case", H8_CASES, ids=_id)
def test_h8_case_selects_its_instantiation(case):
    name, fam, parts, cout, n, h, w, opts = case
    assert _name("slu_conv2d_h8_kernel_name", _h8_desc(fam, parts, cout, n, h, w, **opts)) == (0, name)


@pytest.mark.parametrize("case", FP32_CASES, ids=_id)
def test_fp32_case_selects_its_instantiation(case):
    name, fam, parts, cout, n, h, w, opts = case
    assert _name("slu_conv2d_kernel_name", _conv_desc("fp32", fam, parts, cout, n, h, w, **opts), 64) == (0, name)


@pytest.mark.parametrize("case", F16X3_CASES, ids=_id)
def test_f16x3_case_selects_its_instantiation(case):
    name, fam, parts, cout, n, h, w, opts = case
    assert _name("slu_conv2d_kernel_name", _conv_desc("f16x3", fam, parts, cout, n, h, w, **opts), 64) == (0, name)


@pytest.mark.parametrize("c,resid,shortcut,name", [
    (32, False, False, "tail2_h8_kernel<1, 2, 3, 0>"),
    (32, True, False, "tail2_h8_kernel<1, 2, 3, 1>"),
    (64, False, False, "tail2_h8_kernel<2, 1, 4, 0>"),
    (64, True, False, "tail2_h8_kernel<2, 1, 4, 1>"),
    (64, False, True, "tail2_h8_kernel<2, 1, 4, 2>"),
    (128, True, False, "tail_h8_kernel<2, 2, 4, 1, false>"),
])
def test_tail_shape_selects_its_instantiation(c, resid, shortcut, name):
    d = _lib.ConvTailH8Desc()
    d.a1 = d.a2 = d.w2x2 = d.w1x1 = d.out = PTR
    d.N, d.H, d.W, d.C = 2, 64, 512, c
    d.biasA = d.bnA_a = d.bnA_b = d.biasB = d.bnB_a = d.bnB_b = PTR
    d.hasactA, d.slopeA, d.hasactB, d.slopeB = 1, 0.01, 1, 0.01
    d.resid = PTR if resid else None
    if shortcut:
        d.sc_x = d.sc_w = d.sc_bias = PTR
        d.sc_cin, d.sc_hasact, d.sc_slope = 32, 1, 0.01
    assert _name("slu_conv_tail_h8_kernel_name", d) == (0, name)


@pytest.mark.parametrize("what,fam,parts,cout,opts", [
    ("2x2 / dil 1 with multipliers", (2, 1, 1), [64], 64, dict(scales=True, resid=False)),
    ("a geometry no family has", (3, 3, 3), [64], 64, dict()),
    ("late activation without a residual", (3, 1, 1), [64], 64, dict(late=True, resid=False, bn=False)),
    ("late activation on a 1x1", (1, 1, 0), [64], 64, dict(late=True, bn=False)),
    ("late activation with a folded BatchNorm", (3, 1, 1), [64], 64, dict(late=True)),
    ("shuffled source 0 on a 1x1", (1, 1, 0), [16, 64], 32, dict(shuffle=True, scales=True, resid=False)),
    ("shuffled source, no multipliers, not a ring3 shape", (3, 1, 1), [16, 64], 128, dict(shuffle=True, resid=False)),
    ("fp32 output of a 3x3", (3, 1, 1), [64], 20, dict(out_f32=True)),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else "")
def test_h8_dispatch_refuses(what, fam, parts, cout, opts):
    """The refusals that sit between the families' gates: each must come back as SLU_EUNSUPPORTED, not as some kernel's name."""
    assert _name("slu_conv2d_h8_kernel_name", _h8_desc(fam, parts, cout, 2, 64, 1024, **opts)) == (SLU_EUNSUPPORTED, "")


def test_name_call_returns_the_status_of_the_launch():
    # dropout multipliers with more than 64 input blocks on the tiled path: launch_h8_k refuses (its LDS table of multipliers holds 64 blocks)
    rc, _ = _name("slu_conv2d_h8_kernel_name", _h8_desc((3, 1, 1), [256, 264], 128, 2, 64, 1024, scales=True))
    assert rc == SLU_EUNSUPPORTED
    # (ksize, dil, pad) combinations no family instantiates
    rc, _ = _name("slu_conv2d_kernel_name", _conv_desc("fp32", (3, 3, 3), [32], 32, 2, 64, 512), 64)
    assert rc == SLU_EUNSUPPORTED
    rc, _ = _name("slu_conv2d_kernel_name", _conv_desc("f16x3", (3, 1, 0), [32], 32, 2, 64, 512), 64)
    assert rc == SLU_EUNSUPPORTED
    # and the buffer rules: null, too short
    lib = _lib.load()
    d = _h8_desc((3, 1, 1), [64], 128, 2, 64, 1024)
    assert lib.slu_conv2d_h8_kernel_name(C.byref(d), None, 96) == -1
    assert _name("slu_conv2d_h8_kernel_name", d, 16)[0] == -1
