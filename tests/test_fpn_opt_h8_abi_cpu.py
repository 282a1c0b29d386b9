"""CPU: the C ABI of the `semanticFCN_opt` h8 path (csrc/fpn_opt_h8.hip) and the conv dispatch of every conv layer of that model (names only:
slu_conv2d_h8_kernel_name makes no HIP call, and nothing here launches a kernel)."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT
from semanticlidarunc_amd import _lib, h8

NEW = ("slu_bilinear_upsample_h8", "slu_groupnorm_stats_h8", "slu_groupnorm_apply_h8", "slu_spatial_softmax_gate_h8")
PTR = 0x10000          # non-null, 16-byte aligned; name mode never dereferences it


def test_the_new_symbols_are_declared_typed_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slu.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW + ("slu_groupnorm_stats_h8_workspace_bytes",):
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/slu.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert _lib.ABI_VERSION >= 36 and _lib.load().slu_abi_version() == _lib.ABI_VERSION


def test_conv2d_h8_takes_n_out():
    assert "n_out" in inspect.signature(h8.conv2d_h8).parameters


def test_null_arguments_and_unsupported_shapes_are_refused_before_any_launch():
    lib = _lib.load()
    assert lib.slu_bilinear_upsample_h8(None, None, 1, 1, 4, 4, 2, None) == -1
    assert lib.slu_bilinear_upsample_h8(PTR, PTR, 1, 1, 4, 4, 3, None) == -1            # s = 3
    assert lib.slu_groupnorm_stats_h8(None, 1, 8, 16, 8, 1e-5, None, None, None, None) == -1
    assert lib.slu_groupnorm_stats_h8(PTR, 1, 32, 16, 2, 1e-5, PTR, PTR, PTR, None) == -2     # 16 channels per group
    assert lib.slu_groupnorm_stats_h8(PTR, 1, 24, 16, 8, 1e-5, PTR, PTR, PTR, None) == -2     # 3 channels per group
    assert lib.slu_groupnorm_apply_h8(None, None, None, None, None, 1, None, 1, 8, 16, 8, 1, 0, None) == -1
    assert lib.slu_groupnorm_apply_h8(PTR, PTR, PTR, None, None, 1, PTR, 1, 8, 16, 8, 3, 1, None) == -1      # in place into a slice
    assert lib.slu_groupnorm_apply_h8(PTR, PTR, PTR, None, None, 1, 2 * PTR, 1, 8, 16, 8, 3, 3, None) == -1  # slice past the buffer
    assert lib.slu_spatial_softmax_gate_h8(None, None, None, None, 1, 8, 16, None) == -1
    # one partial of 16 doubles per (plane, part); 2 planes of 128 x 2048 records are cut into 256 parts each
    assert lib.slu_groupnorm_stats_h8_workspace_bytes(1, 16, 128 * 2048) == 2 * 256 * 16 * 8
    assert lib.slu_groupnorm_stats_h8_workspace_bytes(2, 16, 4) == 4 * 1 * 16 * 8
    assert lib.slu_groupnorm_stats_h8_workspace_bytes(0, 16, 4) == 0


def _rc(n, h, w, srcs, cout, k, relu=False, f32=False):
    """srcs: (channels, scaled, nbatch) per source"""
    d = _lib.ConvH8Desc()
    for i, (c, scaled, nb) in enumerate(srcs):
        d.src[i].ptr, d.src[i].scale, d.src[i].G, d.src[i].nbatch = PTR, PTR if scaled else None, (c + 7) // 8, nb
    d.nsrc, d.N, d.H, d.W, d.Cout = len(srcs), n, h, w, cout
    d.ksize, d.dil, d.pad = (3, 1, 1) if k == 3 else (1, 1, 0)
    d.wpack, d.out = PTR, PTR
    d.has_act, d.slope = (1, 0.0) if relu else (0, 0.0)
    d.out_f32_nchw = 1 if f32 else 0
    buf = C.create_string_buffer(96)
    return _lib.load().slu_conv2d_h8_kernel_name(C.byref(d), buf, 96), buf.value.decode()


def _layers(n, hh, ww):
    """(tag, N, H, W, sources, Cout, k, relu, fp32 NCHW output) of the head of resnet18 / resnet34 `semanticFCN_opt` for an hh x ww input: level l
    (1 .. 4) has 32 * 2^(l - 1) channels at (hh, ww) / 2^l; the decoder runs at level 1 and its UpsampleBlock and head at the input size."""
    out = []
    for lvl, c in ((1, 32), (2, 64), (3, 128), (4, 256)):
        h, w = hh >> lvl, ww >> lvl
        out.append((f"att{lvl}.proj", n, h, w, [(c, False, 0)], c // 8, 1, True, False))
        out.append((f"att{lvl}.score h8", n, h, w, [(c // 8, False, 0)], 1, 1, False, False))
        out.append((f"att{lvl}.score f32", n, h, w, [(c // 8, False, 0)], 1, 1, False, True))
    h, w = hh >> 1, ww >> 1
    for c in (64, 128, 256):
        out.append((f"up {c}->32", n, h, w, [(c, False, 0)], 32, 3, False, False))
    out.append(("dec0 2 src", n, h, w, [(32, False, 0), (96, False, 0)], 32, 3, False, False))
    out.append(("dec0 2 src scaled", n, h, w, [(32, True, 0), (96, True, 0)], 32, 3, False, False))
    out.append(("dec0 3 src scaled", n, h, w, [(32, True, 0), (32, True, 0), (64, True, 0)], 32, 3, False, False))
    if n > 1:
        out.append(("dec0 2 src broadcast", n, h, w, [(32, True, 1), (96, True, 1)], 32, 3, False, False))
        out.append(("dec0 3 src broadcast", n, h, w, [(32, True, 1), (32, True, 1), (64, True, 1)], 32, 3, False, False))
    out.append(("dec1", n, h, w, [(32, False, 0)], 32, 3, False, False))
    out.append(("dec_up", n, hh, ww, [(32, False, 0)], 16, 3, False, False))
    out.append(("head 20", n, hh, ww, [(16, False, 0)], 20, 1, False, True))
    out.append(("head 21", n, hh, ww, [(16, False, 0)], 21, 1, False, True))
    return out


@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("hh,ww", [(16, 64), (128, 2048)])
def test_every_conv_of_the_model_is_dispatched(n, hh, ww):
    for tag, nn_, h, w, srcs, cout, k, relu, f32 in _layers(n, hh, ww):
        rc, name = _rc(nn_, h, w, srcs, cout, k, relu, f32)
        assert rc == 0 and name, (tag, n, hh, ww, rc)
