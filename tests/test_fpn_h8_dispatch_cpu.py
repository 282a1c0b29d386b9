"""CPU: what the h8 conv dispatch selects for the layers the ResNet-FPN model adds (names only: slu_conv2d_h8_kernel_name makes no HIP call).
The late activation has ONE implementation, conv_h8_late_kernel; every other path must refuse the flag, never ignore it."""
import ctypes as C
import os

import pytest

from semanticlidarunc_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libslu_hip.so not built")
PTR = 0x10000          # non-null, 16-byte aligned; name mode never dereferences it
SLU_EUNSUPPORTED = -2


def _name(fam, cin, cout, n, h, w, late=False, resid=True, act=True, bn=False, scale=False):
    d = _lib.ConvH8Desc()
    d.src[0].ptr, d.src[0].scale, d.src[0].G = PTR, PTR if scale else None, (cin + 7) // 8
    d.nsrc, d.N, d.H, d.W, d.Cout = 1, n, h, w, cout
    d.ksize, d.dil, d.pad = fam
    d.wpack, d.bias, d.out, d.resid = PTR, PTR, PTR, PTR if resid else None
    d.has_act, d.slope = (1, 0.0) if act else (0, 0.0)
    d.bn_a = d.bn_b = PTR if bn else None
    d.act_after_resid = 1 if late else 0
    buf = C.create_string_buffer(96)
    return _lib.load().slu_conv2d_h8_kernel_name(C.byref(d), buf, 96), buf.value.decode()


# the second conv of every BasicBlock of resnet18 / 34 at 1 x 128 x 2048 (64 x 1024 after the stem) and the shapes of tests/test_gpu_fpn_h8.py
@pytest.mark.parametrize("c,n,h,w", [(64, 1, 64, 1024), (128, 1, 32, 512), (256, 1, 16, 256), (512, 1, 8, 128), (64, 2, 16, 80), (512, 1, 2, 5),
                                     (128, 3, 9, 70)])
def test_late_activation_selects_its_own_kernel(c, n, h, w):
    rc, name = _name((3, 1, 1), c, c, n, h, w, late=True)
    assert rc == 0 and name.startswith("conv_h8_late_kernel<3, 1, 1, "), (rc, name)
    rc, plain = _name((3, 1, 1), c, c, n, h, w, late=False, resid=False)
    assert rc == 0 and "late" not in plain                      # (64 -> 64 without a residual is ring3_h8_kernel's layer)


def test_late_activation_is_refused_everywhere_else():
    assert _name((3, 1, 1), 64, 64, 8, 64, 2048, resid=False)[1].startswith("ring3_h8_kernel")      # the ring kernel's layer (no epilogue for it) ...
    assert _name((3, 1, 1), 64, 64, 8, 64, 2048, late=True)[1].startswith("conv_h8_late_kernel")      # ... goes to the late kernel with the flag
    for kw in (dict(fam=(1, 1, 0)), dict(fam=(1, 1, 0), cin=768, cout=256, h=16, w=512),      # streaming 1x1, the 1x1 GEMM
               dict(fam=(3, 2, 2)), dict(fam=(2, 2, 1)), dict(fam=(2, 1, 1)),
               dict(resid=False), dict(act=False), dict(bn=True), dict(scale=True)):
        a = dict(fam=(3, 1, 1), cin=64, cout=64, n=1, h=64, w=1024)
        a.update(kw)
        fam = a.pop("fam")
        assert _name(fam, **a)[0] == 0, kw                      # fine without the flag ...
        assert _name(fam, late=True, **a)[0] == SLU_EUNSUPPORTED, kw      # ... refused with it


@pytest.mark.parametrize("cin,cout,h,w", [(256, 128, 32, 512), (512, 256, 16, 256), (1024, 512, 8, 128), (256, 128, 8, 40)])
def test_stride2_convs_run_on_the_2_1_1_family(cin, cout, h, w):
    rc, name = _name((2, 1, 1), cin, cout, 1, h, w, resid=False)
    assert rc == 0 and name.startswith("conv_h8_kernel<2, 1, 1, "), (rc, name)
    assert _name((2, 1, 1), cin, cout, 1, h, w, resid=False, scale=True)[0] == SLU_EUNSUPPORTED      # no multipliers on this family
