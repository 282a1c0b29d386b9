"""Checked wrappers of the fp16 channel-blocked ("h8") inference kernels (include/slu.h, section "h8").

An h8 activation is a contiguous ``torch.float16`` tensor of shape ``[N, G, H, W, 8]`` holding channels
``8g .. 8g+7`` of pixel (h, w) in its last axis (pad channels are zero).  All arithmetic happens in the HIP
kernels (fp16 operands, fp32 accumulate / epilogue); torch only owns the memory.
"""
from __future__ import annotations


import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib, ops
from ._lib import ConvH8Desc, check
from .ops import _ptr, _req, _stream


class H8Source(NamedTuple):
    tensor: torch.Tensor                    # [nimg, G, H, W, 8] fp16
    scale: Optional[torch.Tensor] = None    # [N, 8 G] fp32 multiplier (folded Dropout2d) or None
    nbatch: int = 0                         # > 0: tensor holds nbatch images, output image n reads image n % nbatch
    shuffle: bool = False                   # first source only: nn.PixelShuffle(2) of `tensor` ([N, G, H/2, W/2, 8], channels stored in
                                            # shuffle order: shuffle_store_perm), read in place; scale [N, 8 G] in stored order.
                                            # Covered: the 80 -> 32 3x3 layer (ring3) and 3x3 layers with multipliers (slu.h)


def shuffle_store_perm(channels: int, device=None) -> torch.Tensor:
    """perm[p] = the channel that position p of a tensor STORED IN SHUFFLE ORDER holds: stored block 4 go + sub, slot k <- channel
    32 go + 4 k + sub (sub = 2 i + j), so that block go of nn.PixelShuffle(2)(t) at pixel (2 h + i, 2 w + j) is the stored record of block
    4 go + sub at (h, w).  A producer stores t[:, perm] by permuting the rows of its weight, bias and folded BatchNorm with perm."""
    if channels % 32:
        raise RuntimeError(f"shuffle_store_perm: {channels} channels are not whole groups of 32")
    key = (int(channels), None if device is None else str(device))
    perm = _STORE_PERM.get(key)
    if perm is None:
        p = torch.arange(channels, device=device)
        perm = _STORE_PERM[key] = 32 * (p // 32) + 4 * (p % 8) + (p // 8) % 4
    return perm


_STORE_PERM = {}


_SHUFFLE_OK = {}


def conv_shuffle_in_place_supported(*args, **kw) -> bool:
    """conv_shuffle_in_place_kernel(...) is not None."""
    return conv_shuffle_in_place_kernel(*args, **kw) is not None


def conv_shuffle_in_place_kernel(n: int, h: int, w: int, c_stored: int, c_skip: int, cout: int, ksize: int, dil: int, pad: int,
                                 scaled: bool, skip_scaled: bool = False, skip_nbatch: int = 0) -> Optional[str]:
    """Does slu_conv2d_h8_fwd read a first source of `c_stored` stored channels through PixelShuffle in place for this layer (output n x h x w,
    a second source of c_skip channels)?  Asked of the launch's own dispatch (slu_conv2d_h8_kernel_name on a descriptor of that shape: no
    memory is touched), cached per shape: the name of the kernel that would, or None.  Today: ring3_h8_kernel<1, 1, 5, 1, 4> (64 stored
    channels, plain 64-channel skip, 32 outputs, >= 256 tiles) and the SCALED 3x3 conv_h8_kernel instantiations (some source carries
    multipliers, 3 * c_stored / 32 + input blocks <= 64)."""
    key = (n, h, w, c_stored, c_skip, cout, ksize, dil, pad, bool(scaled), bool(skip_scaled), int(skip_nbatch))
    ok = _SHUFFLE_OK.get(key, 0)
    if ok == 0:
        ok = None
        if c_stored % 64 == 0 and c_skip % 8 == 0 and h % 2 == 0 and w % 2 == 0:
            d = ConvH8Desc()
            fake = 1 << 20                                   # an aligned non-null address: the dispatch only tests and formats
            d.src[0].ptr, d.src[0].scale, d.src[0].G, d.src[0].shuffle = fake, (fake if scaled else None), c_stored // 8, 1
            d.nsrc = 1
            if c_skip:
                d.src[1].ptr, d.src[1].scale, d.src[1].G, d.src[1].nbatch = fake, (fake if skip_scaled else None), c_skip // 8, int(skip_nbatch)
                d.nsrc = 2
            d.N, d.H, d.W, d.Cout, d.ksize, d.dil, d.pad = n, h, w, cout, ksize, dil, pad
            d.wpack, d.out, d.has_act, d.slope = fake, fake, 1, 0.01
            buf = C.create_string_buffer(96)
            if _lib.load().slu_conv2d_h8_kernel_name(C.byref(d), buf, 96) == 0:
                ok = buf.value.decode()
        _SHUFFLE_OK[key] = ok
    return ok


def _req_h8(t: torch.Tensor, name: str) -> torch.Tensor:
    _req(t, name, torch.float16)
    if t.dim() != 5 or t.shape[4] != 8:
        raise RuntimeError(f"{name}: expected an h8 tensor [N, G, H, W, 8], got {tuple(t.shape)}")
    return t


def to_h8(x: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 NCHW -> h8 (channels padded to a multiple of 8 with zeros), optionally times scale[n, c]."""
    _req(x, "x")
    if x.dim() != 4:
        raise RuntimeError(f"x: expected NCHW, got {tuple(x.shape)}")
    n, c, h, w = x.shape
    if scale is not None:
        _req(scale, "scale")
        if tuple(scale.shape) != (n, c):
            raise RuntimeError(f"scale: expected {(n, c)}, got {tuple(scale.shape)}")
    y = torch.empty((n, (c + 7) // 8, h, w, 8), dtype=torch.float16, device=x.device)
    check(_lib.load().slu_nchw_to_h8(x.data_ptr(), _ptr(scale), y.data_ptr(), n, c, h, w, _stream()), "slu_nchw_to_h8")
    return y


def from_h8(x: torch.Tensor, channels: Optional[int] = None) -> torch.Tensor:
    """h8 -> fp32 NCHW with `channels` channels (default 8 G)."""
    _req_h8(x, "x")
    n, g, h, w, _ = x.shape
    c = 8 * g if channels is None else int(channels)
    if not 8 * (g - 1) < c <= 8 * g:
        raise RuntimeError(f"from_h8: {c} channels do not fit {g} blocks")
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_h8_to_nchw(x.data_ptr(), y.data_ptr(), n, c, h, w, _stream()), "slu_h8_to_nchw")
    return y


def pack_conv_weight_h8(weight: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 weight -> fp16 MFMA A-fragment image (re-run after every weight update)."""
    _req(weight, "weight")
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise RuntimeError(f"weight: expected [Cout,Cin,k,k], got {tuple(weight.shape)}")
    lib = _lib.load()
    cout, cin, ks, _ = weight.shape
    nbytes = lib.slu_packed_weight_bytes_h8(cout, cin, ks)
    if nbytes == 0:
        raise RuntimeError("pack_conv_weight_h8: unsupported weight shape")
    out = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    check(lib.slu_pack_conv_weight_h8(weight.data_ptr(), cout, cin, ks, out.data_ptr(), _stream()), "slu_pack_conv_weight_h8")
    return out


def conv2d_h8(srcs: Sequence[H8Source], wpack: torch.Tensor, cin: int, cout: int, ksize: int, dil: int, pad: int,
              bias: Optional[torch.Tensor] = None, slope: Optional[float] = None,
              bn_a: Optional[torch.Tensor] = None, bn_b: Optional[torch.Tensor] = None,
              resid: Optional[torch.Tensor] = None, out_f32_nchw: bool = False, act_after_resid: bool = False,
              n_out: Optional[int] = None) -> torch.Tensor:
    """out = [resid +] bn_a * leaky(conv(cat(srcs * scale)) + bias) + bn_b  (slu_conv2d_h8_fwd).
    `cin` = real input channels the weight was packed with (only the last source may carry pad channels).
    act_after_resid: out = leaky(conv + bias + resid) instead (a BasicBlock's second conv): 3x3 / dil 1 / pad 1 with a residual and a slope
    only; any other layer raises (SLU_EUNSUPPORTED).
    n_out: the number of output images, so that EVERY source may be batch-broadcast (nbatch): the stacked passes of an MC-dropout
    evaluation read one shared set of images.  Default: the batch of the first source, which then must hold it in full."""
    lib = _lib.load()
    if not 1 <= len(srcs) <= _lib.MAX_SRC:
        raise RuntimeError(f"conv2d_h8: 1..{_lib.MAX_SRC} sources supported, got {len(srcs)}")
    d = ConvH8Desc()
    n = None if n_out is None else int(n_out)
    if n is not None and n <= 0:
        raise RuntimeError(f"conv2d_h8: n_out={n_out} is not a positive number of images")
    h = w = None
    gin = 0
    keep = []
    for i, s in enumerate(srcs):
        t = _req_h8(s.tensor, f"src[{i}]")
        sn, sg, sh, sw, _ = t.shape
        gstored = sg
        if s.shuffle:
            if i != 0 or sg % 8 or s.nbatch:
                raise RuntimeError("src[0] only may be read through PixelShuffle in place, with whole groups of 64 stored channels")
            sg, sh, sw = sg // 4, 2 * sh, 2 * sw
        if s.nbatch:
            if n is None or sn != s.nbatch or n % sn:
                raise RuntimeError(f"src[{i}]: a batch-broadcast source must follow a full-batch source (or n_out be given) and divide N")
            sn = n
        if n is None:
            n = sn
        if h is None:
            h, w = sh, sw
        if (sn, sh, sw) != (n, h, w):
            raise RuntimeError(f"src[{i}]: spatial/batch size {(sn, sh, sw)} != {(n, h, w)}")
        if s.scale is not None:
            _req(s.scale, f"src[{i}].scale")
            if tuple(s.scale.shape) != (n, 8 * gstored):
                raise RuntimeError(f"src[{i}].scale: expected {(n, 8 * gstored)}, got {tuple(s.scale.shape)}")
        d.src[i].ptr, d.src[i].scale, d.src[i].G, d.src[i].nbatch = t.data_ptr(), _ptr(s.scale), gstored, int(s.nbatch)
        d.src[i].shuffle = 1 if s.shuffle else 0
        gin += sg
        keep.append(t)
    if not 8 * (gin - 1) < cin <= 8 * gin:
        raise RuntimeError(f"conv2d_h8: cin={cin} does not match {gin} input blocks")
    _req(wpack, "wpack", torch.uint8)
    if wpack.numel() != lib.slu_packed_weight_bytes_h8(cout, cin, ksize):
        raise RuntimeError(f"wpack: {wpack.numel()} bytes does not match Cout={cout} Cin={cin} k={ksize} (h8)")
    for t, nme in ((bias, "bias"), (bn_a, "bn_a"), (bn_b, "bn_b")):
        if t is not None:
            _req(t, nme)
            if t.numel() != cout:
                raise RuntimeError(f"{nme}: expected {cout} elements, got {t.numel()}")
    if (bn_a is None) != (bn_b is None):
        raise RuntimeError("bn_a and bn_b must be given together")
    gout = (cout + 7) // 8
    if out_f32_nchw:
        if resid is not None:
            raise RuntimeError("conv2d_h8: no residual on the fp32 NCHW output form")
        out = torch.empty((n, cout, h, w), dtype=torch.float32, device=keep[0].device)
    else:
        out = torch.empty((n, gout, h, w, 8), dtype=torch.float16, device=keep[0].device)
    if resid is not None:
        _req_h8(resid, "resid")
        if tuple(resid.shape) != (n, gout, h, w, 8):
            raise RuntimeError(f"resid: expected {(n, gout, h, w, 8)}, got {tuple(resid.shape)}")
    d.nsrc = len(srcs)
    d.N, d.H, d.W, d.Cout = n, h, w, cout
    d.ksize, d.dil, d.pad = ksize, dil, pad
    d.wpack, d.bias = wpack.data_ptr(), _ptr(bias)
    d.has_act, d.slope = (0, 0.0) if slope is None else (1, float(slope))
    d.bn_a, d.bn_b, d.resid, d.out = _ptr(bn_a), _ptr(bn_b), _ptr(resid), out.data_ptr()
    d.out_f32_nchw = 1 if out_f32_nchw else 0
    d.act_after_resid = 1 if act_after_resid else 0
    if ops.TIMING is None:
        check(lib.slu_conv2d_h8_fwd(C.byref(d), _stream()), "slu_conv2d_h8_fwd")
        return out
    # measurement mode (bench.py): HIP events on the launch stream around this one kernel
    buf = C.create_string_buffer(96)
    check(lib.slu_conv2d_h8_kernel_name(C.byref(d), buf, 96), "slu_conv2d_h8_kernel_name")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.slu_conv2d_h8_fwd(C.byref(d), _stream()), "slu_conv2d_h8_fwd")
    e1.record()
    flops = 2.0 * cin * cout * ksize * ksize * n * h * w
    # (a source read through PixelShuffle in place contributes cin / 4 of its stored channels at 4x the pixels: its tensor, once)
    nbytes = n * h * w * (2.0 * cin + (4.0 if out_f32_nchw else 2.0) * cout) + 2.0 * cout * cin * ksize * ksize
    ops.TIMING.append((buf.value.decode(), flops, nbytes, e0, e1, nbytes + (n * h * w * 2.0 * cout if resid is not None else 0.0)))
    ops.TIMING_TAGS.append(f"N{n} {cin}->{cout} k{ksize}d{dil} {h}x{w}")
    return out


def conv_tail_supported(channels: int, h: int, w: int) -> bool:
    return bool(_lib.load().slu_conv_tail_h8_supported(int(channels), int(h), int(w)))


_TAIL_NAMES: dict = {}


def conv_tail_kernel_name(channels: int, n: int, h: int, w: int, resid: bool) -> str:
    """The kernel instantiation conv_tail_h8 launches for this shape, by the library's own dispatch (slu_conv_tail_h8_kernel_name walked
    with placeholder addresses; no launch)."""
    key = (int(channels), int(n), int(h), int(w), bool(resid))
    name = _TAIL_NAMES.get(key)
    if name is None:
        d = _lib.ConvTailH8Desc()
        d.a1 = d.a2 = d.w2x2 = d.w1x1 = d.out = 0x1000
        d.resid = 0x1000 if resid else None
        d.C, d.N, d.H, d.W = key[:4]
        buf = C.create_string_buffer(96)
        check(_lib.load().slu_conv_tail_h8_kernel_name(C.byref(d), buf, 96), "slu_conv_tail_h8_kernel_name")
        name = _TAIL_NAMES[key] = buf.value.decode()
    return name


def conv_tail_shortcut_supported(channels: int, cin: int) -> bool:
    return bool(_lib.load().slu_conv_tail_h8_shortcut_supported(int(channels), int(cin)))


def conv_tail_h8(a1: torch.Tensor, a2: torch.Tensor, w2x2: torch.Tensor, w1x1: torch.Tensor,
                 bias_a: Optional[torch.Tensor], slope_a: Optional[float], bn_a: Optional[tuple],
                 bias_b: Optional[torch.Tensor], slope_b: Optional[float], bn_b: Optional[tuple],
                 resid: Optional[torch.Tensor] = None, shortcut: Optional[tuple] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The fused tail of a SalsaNext block (slu_conv_tail_h8_fwd):
        a3  = bn_a(leaky(conv2x2_dil2(a2) + bias_a));   out = [resid +] bn_b(leaky(conv1x1(cat(a1, a2, a3)) + bias_b))
    a1 / a2 / resid: h8 [N, C/8, H, W, 8]; w2x2 / w1x1: pack_conv_weight_h8 of [C, C, 2, 2] / [C, 3C, 1, 1]; bn_*: (scale, shift) or None.
    shortcut = (x, wpack, bias, slope, cin) instead of resid: resid = leaky(conv1x1(x) + bias) computed inside the kernel from the block's input
    x (h8 [N, cin/8, H, W, 8], wpack = pack_conv_weight_h8 of [C, cin, 1, 1]); conv_tail_shortcut_supported(C, cin).
    out: an h8 tensor of a1's shape to write into (default: a new one)."""
    lib = _lib.load()
    _req_h8(a1, "a1")
    _req_h8(a2, "a2")
    if a1.shape != a2.shape:
        raise RuntimeError(f"conv_tail_h8: a1 {tuple(a1.shape)} != a2 {tuple(a2.shape)}")
    n, g, h, w, _ = a1.shape
    c = 8 * g
    if not conv_tail_supported(c, h, w):
        raise RuntimeError(f"conv_tail_h8: C={c} is not covered by the fused kernel (use two conv2d_h8 calls)")
    _req(w2x2, "w2x2", torch.uint8)
    _req(w1x1, "w1x1", torch.uint8)
    if w2x2.numel() != lib.slu_packed_weight_bytes_h8(c, c, 2) or w1x1.numel() != lib.slu_packed_weight_bytes_h8(c, 3 * c, 1):
        raise RuntimeError("conv_tail_h8: packed weight sizes do not match C")
    d = _lib.ConvTailH8Desc()
    for name, t in (("bias_a", bias_a), ("bias_b", bias_b)) + tuple((f"bn_{k}[{i}]", v) for k, pair in (("a", bn_a), ("b", bn_b)) if pair is not None
                                                                       for i, v in enumerate(pair)):
        if t is not None:
            _req(t, name)
            if t.numel() != c:
                raise RuntimeError(f"{name}: expected {c} elements, got {t.numel()}")
    if resid is not None:
        _req_h8(resid, "resid")
        if resid.shape != a1.shape:
            raise RuntimeError(f"resid: expected {tuple(a1.shape)}, got {tuple(resid.shape)}")
    if shortcut is not None:
        sx, sw, sb, sslope, scin = shortcut
        if resid is not None:
            raise RuntimeError("conv_tail_h8: resid and shortcut are exclusive")
        if not conv_tail_shortcut_supported(c, scin):
            raise RuntimeError(f"conv_tail_h8: shortcut {scin} -> {c} is not covered (run the 1x1 conv and pass resid)")
        _req_h8(sx, "shortcut.x")
        _req(sw, "shortcut.w", torch.uint8)
        if tuple(sx.shape) != (n, scin // 8, h, w, 8) or sw.numel() != lib.slu_packed_weight_bytes_h8(c, scin, 1):
            raise RuntimeError("conv_tail_h8: shortcut operand sizes do not match")
        if sb is not None:
            _req(sb, "shortcut.bias")
            if sb.numel() != c:
                raise RuntimeError(f"shortcut.bias: expected {c} elements, got {sb.numel()}")
    if out is None:
        out = torch.empty_like(a1)
    else:
        _req_h8(out, "out")
        if out.shape != a1.shape:
            raise RuntimeError(f"out: expected {tuple(a1.shape)}, got {tuple(out.shape)}")
    d.a1, d.a2, d.N, d.H, d.W, d.C = a1.data_ptr(), a2.data_ptr(), n, h, w, c
    if shortcut is not None:
        d.sc_x, d.sc_w, d.sc_bias, d.sc_cin = sx.data_ptr(), sw.data_ptr(), _ptr(sb), int(scin)
        d.sc_hasact, d.sc_slope = (0, 0.0) if sslope is None else (1, float(sslope))
    d.w2x2, d.w1x1 = w2x2.data_ptr(), w1x1.data_ptr()
    d.biasA, d.bnA_a, d.bnA_b = _ptr(bias_a), _ptr(None if bn_a is None else bn_a[0]), _ptr(None if bn_a is None else bn_a[1])
    d.biasB, d.bnB_a, d.bnB_b = _ptr(bias_b), _ptr(None if bn_b is None else bn_b[0]), _ptr(None if bn_b is None else bn_b[1])
    d.hasactA, d.slopeA = (0, 0.0) if slope_a is None else (1, float(slope_a))
    d.hasactB, d.slopeB = (0, 0.0) if slope_b is None else (1, float(slope_b))
    d.resid, d.out = _ptr(resid), out.data_ptr()
    if ops.TIMING is None:
        check(lib.slu_conv_tail_h8_fwd(C.byref(d), _stream()), "slu_conv_tail_h8_fwd")
        return out
    buf = C.create_string_buffer(96)
    check(lib.slu_conv_tail_h8_kernel_name(C.byref(d), buf, 96), "slu_conv_tail_h8_kernel_name")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.slu_conv_tail_h8_fwd(C.byref(d), _stream()), "slu_conv_tail_h8_fwd")
    e1.record()
    # the layer-granular convention of SURVEY 8(d): both convs read their inputs and write their outputs once
    scin = shortcut[4] if shortcut is not None else 0
    flops = 2.0 * c * (c * (4 + 3) + scin) * n * h * w
    # layer-granular convention: every conv reads its inputs and writes its output once (the shortcut conv: x in, shortcut out)
    nbytes = n * h * w * 2.0 * (c + c + 3 * c + c + (scin + c if shortcut is not None else 0)) + 2.0 * c * (c * (4 + 3) + scin)
    # what the fused kernel must move: a1, a2 (+ the residual, or the shortcut's input) in, out once, weights
    min_bytes = n * h * w * 2.0 * (c * 3 + (c if resid is not None else 0) + scin) + 2.0 * c * (c * (4 + 3) + scin)
    ops.TIMING.append((buf.value.decode(), flops, nbytes, e0, e1, min_bytes))
    ops.TIMING_TAGS.append(f"N{n} {c}->{c} k2d2 + {3 * c}->{c} k1" + (f" + {scin}->{c} k1 shortcut" if shortcut is not None else "") + f" fused {h}x{w}")
    return out


def ctx_block_supported(cin: int, c: int, h: int, w: int) -> bool:
    return bool(_lib.load().slu_ctx_block_h8_supported(int(cin), int(c), int(h), int(w)))


def ctx_block_h8(x: torch.Tensor, cin: int, w1: torch.Tensor, w2: torch.Tensor, w3: torch.Tensor, bias1: Optional[torch.Tensor],
                 bias2: Optional[torch.Tensor], bn1: Optional[tuple], bias3: Optional[torch.Tensor], bn2: Optional[tuple],
                 slope: float, n_out: Optional[int] = None) -> torch.Tensor:
    """One fused ResContextBlock (slu_ctx_block_h8_fwd, SalsaNext.py:25-39):
        s = leaky(conv1x1(x) + bias1);  a1 = bn1(leaky(conv3x3(s) + bias2));  out = s + bn2(leaky(conv3x3_dil2(a1) + bias3))
    x: h8 [N, ceil(cin/8), H, W, 8]; w1 / w2 / w3: pack_conv_weight_h8 of [32, cin, 1, 1] / [32, 32, 3, 3] / [32, 32, 3, 3]; bn*: (scale, shift).
    n_out: a multiple of N: output image n is the block of x[n % N] (the stacked passes of an MC-dropout evaluation share their input)."""
    lib = _lib.load()
    _req_h8(x, "x")
    nimg, g, h, w, _ = x.shape
    n = nimg if n_out is None else int(n_out)
    if n <= 0 or n % nimg:
        raise RuntimeError(f"ctx_block_h8: n_out={n} is not a multiple of the {nimg} input images")
    if not 8 * (g - 1) < cin <= 8 * g or not ctx_block_supported(cin, 32, h, w):
        raise RuntimeError(f"ctx_block_h8: cin={cin} with {g} input blocks is not covered by the fused kernel")
    for t, nme, shape in ((w1, "w1", (32, cin, 1)), (w2, "w2", (32, 32, 3)), (w3, "w3", (32, 32, 3))):
        _req(t, nme, torch.uint8)
        if t.numel() != lib.slu_packed_weight_bytes_h8(*shape):
            raise RuntimeError(f"{nme}: packed weight size does not match {shape}")
    vecs = (("bias1", bias1), ("bias2", bias2), ("bias3", bias3)) + tuple((f"bn{k}[{i}]", v) for k, pair in ((1, bn1), (2, bn2)) if pair is not None
                                                                           for i, v in enumerate(pair))
    for name, t in vecs:
        if t is not None:
            _req(t, name)
            if t.numel() != 32:
                raise RuntimeError(f"{name}: expected 32 elements, got {t.numel()}")
    out = torch.empty((n, 4, h, w, 8), dtype=torch.float16, device=x.device)
    d = _lib.CtxBlockH8Desc()
    d.x, d.N, d.H, d.W, d.Cin, d.C = x.data_ptr(), n, h, w, int(cin), 32
    d.w1, d.w2, d.w3 = w1.data_ptr(), w2.data_ptr(), w3.data_ptr()
    d.bias1, d.bias2, d.bias3 = _ptr(bias1), _ptr(bias2), _ptr(bias3)
    d.bn1_a, d.bn1_b = _ptr(None if bn1 is None else bn1[0]), _ptr(None if bn1 is None else bn1[1])
    d.bn2_a, d.bn2_b = _ptr(None if bn2 is None else bn2[0]), _ptr(None if bn2 is None else bn2[1])
    d.slope, d.out = float(slope), out.data_ptr()
    d.nbatch = 0 if n == nimg else nimg
    if ops.TIMING is None:
        check(lib.slu_ctx_block_h8_fwd(C.byref(d), _stream()), "slu_ctx_block_h8_fwd")
        return out
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.slu_ctx_block_h8_fwd(C.byref(d), _stream()), "slu_ctx_block_h8_fwd")
    e1.record()
    px = float(n * h * w)
    flops = 2.0 * (cin * 32 + 2 * 9 * 32 * 32) * px
    # SURVEY 8(d) layer-granular bytes of the three convs (each reads its input and writes its output once) vs what the fused kernel moves
    nbytes = px * 2.0 * ((8 * g + 32) + (32 + 32) + (32 + 32)) + 2.0 * (32 * cin + 2 * 9 * 32 * 32)
    # (a broadcast input is counted once: its nimg images, not the n reads of them)
    min_bytes = float(h * w) * 2.0 * (nimg * 8 * g + n * 32) + 2.0 * (32 * cin + 2 * 9 * 32 * 32)
    ops.TIMING.append((f"ctx_h8_kernel<{1 if cin <= 16 else 2}>", flops, nbytes, e0, e1, min_bytes))
    ops.TIMING_TAGS.append(f"N{n} {cin}->32 k1 + 32->32 k3d1 + 32->32 k3d2 fused {h}x{w}")
    return out


def head_mc_h8(x: torch.Tensor, wpack: torch.Tensor, bias: Optional[torch.Tensor], classes: int, passes: int, batch: int, eps: float = 1e-12):
    """x: h8 [T*B, G, H, W, 8] (pass-major) -> (p_bar [B,C,H,W], H_norm [B,H,W], MI_norm [B,H,W], preds int64 [B,H,W]): the 1x1 head
    conv and the MC-dropout reduction of trainer.py:1143-1154 in one launch (slu_head_mc_h8)."""
    _req_h8(x, "x")
    n, g, h, w, _ = x.shape
    if n != passes * batch:
        raise RuntimeError(f"head_mc_h8: {n} images != T * B = {passes} * {batch}")
    lib = _lib.load()
    _req(wpack, "wpack", torch.uint8)
    if wpack.numel() != lib.slu_packed_weight_bytes_h8(classes, 8 * g, 1):
        raise RuntimeError("head_mc_h8: packed weight size does not match the head")
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != classes:
            raise RuntimeError(f"bias: expected {classes} elements, got {bias.numel()}")
    dev = x.device
    p_bar = torch.empty((batch, classes, h, w), dtype=torch.float32, device=dev)
    hn = torch.empty((batch, h, w), dtype=torch.float32, device=dev)
    mi = torch.empty((batch, h, w), dtype=torch.float32, device=dev)
    preds = torch.empty((batch, h, w), dtype=torch.int64, device=dev)
    args = (x.data_ptr(), passes, batch, g, h * w, wpack.data_ptr(), _ptr(bias), classes, float(eps), p_bar.data_ptr(), hn.data_ptr(),
            mi.data_ptr(), preds.data_ptr(), _stream())
    if ops.TIMING is None:
        check(lib.slu_head_mc_h8(*args), "slu_head_mc_h8")
        return p_bar, hn, mi, preds
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.slu_head_mc_h8(*args), "slu_head_mc_h8")
    e1.record()
    # layer-granular accounting: the head conv reads its fp16 input and "writes" fp32 logits; the epilogue of SURVEY 8(d) reads them back
    flops = 2.0 * 8 * g * classes * n * h * w
    nbytes = n * h * w * (2.0 * 8 * g + 4.0 * classes) + 2.0 * classes * 8 * g
    # what the fused kernel must move: the decoder output of every pass in, p_bar / H / MI / argmax of every scan out
    min_bytes = n * h * w * 2.0 * 8 * g + batch * h * w * (4.0 * classes + 16.0) + 2.0 * classes * 8 * g
    ops.TIMING.append((f"head_mc_h8_kernel<{g // 2}, {(classes + 7) // 8}>", flops, nbytes, e0, e1, min_bytes))
    ops.TIMING_TAGS.append(f"N{n} {8 * g}->{classes} k1 head + MC reduce T={passes} {h}x{w}")
    return p_bar, hn, mi, preds


def avgpool3s2_h8(x: torch.Tensor, scale: Optional[torch.Tensor] = None, n_out: Optional[int] = None) -> torch.Tensor:
    """AvgPool2d(3, 2, 1) of x[n % B] * scale[n] for n < n_out (n_out = B unless x is shared by stacked MC passes)."""
    _req_h8(x, "x")
    b, g, h, w, _ = x.shape
    n = b if n_out is None else int(n_out)
    if n % b:
        raise RuntimeError("avgpool3s2_h8: n_out must be a multiple of the input batch")
    if scale is not None:
        _req(scale, "scale")
        if tuple(scale.shape) != (n, 8 * g):
            raise RuntimeError(f"scale: expected {(n, 8 * g)}, got {tuple(scale.shape)}")
    y = torch.empty((n, g, (h + 1) // 2, (w + 1) // 2, 8), dtype=torch.float16, device=x.device)
    check(_lib.load().slu_avgpool3s2_h8(x.data_ptr(), _ptr(scale), y.data_ptr(), n, 0 if n == b else b, g, h, w, _stream()),
          "slu_avgpool3s2_h8")
    return y


def pixel_shuffle_h8(x: torch.Tensor, scale_in: Optional[torch.Tensor] = None, scale_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.PixelShuffle(2) of x * scale_in[n, c_in], times scale_out[n, c_out] (both Dropout2d multipliers around it)."""
    _req_h8(x, "x")
    n, g, h, w, _ = x.shape
    for t, nme, c in ((scale_in, "scale_in", 8 * g), (scale_out, "scale_out", 2 * g)):
        if t is not None:
            _req(t, nme)
            if tuple(t.shape) != (n, c):
                raise RuntimeError(f"{nme}: expected {(n, c)}, got {tuple(t.shape)}")
    y = torch.empty((n, (2 * g + 7) // 8, 2 * h, 2 * w, 8), dtype=torch.float16, device=x.device)
    check(_lib.load().slu_pixel_shuffle_h8(x.data_ptr(), _ptr(scale_in), _ptr(scale_out), y.data_ptr(), n, g, h, w, _stream()),
          "slu_pixel_shuffle_h8")
    return y


def maxpool3s2_h8(x: torch.Tensor) -> torch.Tensor:
    """nn.MaxPool2d(3, 2, 1) (slu_maxpool3s2_h8): padding is -inf, pad channels stay 0."""
    _req_h8(x, "x")
    n, g, h, w, _ = x.shape
    y = torch.empty((n, g, (h + 1) // 2, (w + 1) // 2, 8), dtype=torch.float16, device=x.device)
    check(_lib.load().slu_maxpool3s2_h8(x.data_ptr(), y.data_ptr(), n, g, h, w, _stream()), "slu_maxpool3s2_h8")
    return y


def space_to_depth2_h8(x: torch.Tensor, meta: Optional[torch.Tensor] = None, channels: Optional[int] = None, factor: int = 1,
                       phase00: bool = True):
    """(y, y00) = slu_space_to_depth2_h8: y [N, 4 G, H/2, W/2, 8] phase-major (channel (2 p + q) 8 G + c = x[c, 2 y + p, 2 x + q]) and, with
    phase00, y00 [N, G, H/2, W/2, 8] = phase (0, 0) alone (else None).  meta: fp32 [N, m, factor H, factor W] whose nearest 1 / factor
    down-sampling replaces the last m of x's `channels` (default 8 G) real channels on the way."""
    _req_h8(x, "x")
    n, g, h, w, _ = x.shape
    if h % 2 or w % 2:
        raise RuntimeError(f"space_to_depth2_h8: H and W must be even, got {(h, w)}")
    c = 8 * g if channels is None else int(channels)
    m = 0
    if meta is not None:
        _req(meta, "meta")
        if factor not in (1, 2, 4, 8):
            raise RuntimeError(f"space_to_depth2_h8: factor {factor} is not one of 1, 2, 4, 8")
        if meta.dim() != 4 or (meta.shape[0], meta.shape[2], meta.shape[3]) != (n, factor * h, factor * w):
            raise RuntimeError(f"meta: expected [{n}, m, {factor * h}, {factor * w}], got {tuple(meta.shape)}")
        m = meta.shape[1]
        if not (8 * (g - 1) < c <= 8 * g and 0 < m <= c):
            raise RuntimeError(f"space_to_depth2_h8: {m} meta channels / {c} channels do not fit {g} blocks")
    y = torch.empty((n, 4 * g, h // 2, w // 2, 8), dtype=torch.float16, device=x.device)
    y00 = torch.empty((n, g, h // 2, w // 2, 8), dtype=torch.float16, device=x.device) if phase00 else None
    check(_lib.load().slu_space_to_depth2_h8(x.data_ptr(), _ptr(meta), m, c, int(factor), y.data_ptr(), _ptr(y00), n, g, h, w, _stream()),
          "slu_space_to_depth2_h8")
    return y, y00


def attention_row_h8(tv: torch.Tensor, w_a: torch.Tensor, b_a: torch.Tensor) -> torch.Tensor:
    """out = v * softmax_W(b_a + sum_c w_a[c] tanh(t[c])) with (t, v) = the two channel halves of tv [N, 2 C / 8, H, W, 8]
    (slu_attention_row_h8); w_a fp32 [C], b_a fp32 [1]."""
    _req_h8(tv, "tv")
    n, g2, h, w, _ = tv.shape
    if g2 % 2:
        raise RuntimeError(f"attention_row_h8: {g2} blocks are not two equal halves")
    c = 4 * g2
    _req(w_a, "w_a")
    _req(b_a, "b_a")
    if w_a.numel() != c or b_a.numel() != 1:
        raise RuntimeError(f"attention_row_h8: expected w_a of {c} and b_a of 1 element, got {w_a.numel()} and {b_a.numel()}")
    out = torch.empty((n, g2 // 2, h, w, 8), dtype=torch.float16, device=tv.device)
    check(_lib.load().slu_attention_row_h8(tv.data_ptr(), w_a.data_ptr(), b_a.data_ptr(), out.data_ptr(), n, c, h, w, _stream()),
          "slu_attention_row_h8")
    return out


def depth_to_space_h8(y: torch.Tensor, s: int, out: Optional[torch.Tensor] = None, g_off: int = 0, elu_plus_one: bool = False,
                      classes: Optional[int] = None) -> torch.Tensor:
    """Two forms.  Plain (slu_depth_to_space_h8): y [N, s s Cout / 8, H, W, 8] with channels ordered (i, j, cout), Cout % 8 == 0, s in 2 / 4 / 8
    -> blocks [g_off, g_off + Cout / 8) of `out` [N, Gtot, s H, s W, 8] (allocated with exactly Cout / 8 blocks when None).
    elu_plus_one (slu_depth_to_space2_elu_h8, s = 2): y [N, ceil(4 classes / 8), H, W, 8] with channels ordered (class, i, j) -> fp32 NCHW
    [N, classes, 2 H, 2 W] = elu(pixel_shuffle(y)) + 1."""
    _req_h8(y, "y")
    n, g, h, w, _ = y.shape
    lib = _lib.load()
    if elu_plus_one:
        if s != 2 or classes is None or (4 * classes + 7) // 8 != g or out is not None:
            raise RuntimeError(f"depth_to_space_h8: the ELU + 1 form takes s = 2 and `classes` matching the {g} blocks of y")
        res = torch.empty((n, classes, 2 * h, 2 * w), dtype=torch.float32, device=y.device)
        check(lib.slu_depth_to_space2_elu_h8(y.data_ptr(), res.data_ptr(), n, int(classes), h, w, _stream()), "slu_depth_to_space2_elu_h8")
        return res
    if s not in (2, 4, 8) or g % (s * s):
        raise RuntimeError(f"depth_to_space_h8: {g} blocks are not s * s = {s * s} whole groups (s in 2, 4, 8)")
    go = g // (s * s)
    if out is None:
        out = torch.empty((n, go, s * h, s * w, 8), dtype=torch.float16, device=y.device)
    _req_h8(out, "out")
    if (out.shape[0], out.shape[2], out.shape[3]) != (n, s * h, s * w) or g_off < 0 or g_off + go > out.shape[1]:
        raise RuntimeError(f"out: blocks [{g_off}, {g_off + go}) of {tuple(out.shape)} do not take {(n, go, s * h, s * w, 8)}")
    check(lib.slu_depth_to_space_h8(y.data_ptr(), out.data_ptr(), n, 8 * go, int(s), h, w, out.shape[1], int(g_off), _stream()),
          "slu_depth_to_space_h8")
    return out


# ---- what `semanticFCN_opt` puts between its convs (csrc/fpn_opt_h8.hip) ----
def _timed(name: str, tag: str, flops: float, nbytes: float, launch) -> None:
    """Run one launch; in measurement mode (ops.TIMING) between HIP events, recorded like the convs."""
    if ops.TIMING is None:
        launch()
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    ops.TIMING.append((name, flops, nbytes, e0, e1, nbytes))
    ops.TIMING_TAGS.append(tag)


def bilinear_upsample_h8(x: torch.Tensor, s: int) -> torch.Tensor:
    """F.interpolate(scale_factor=s, mode='bilinear', align_corners=False) of an h8 tensor, s in 2 / 4 / 8 (slu_bilinear_upsample_h8)."""
    _req_h8(x, "x")
    n, g, h, w, _ = x.shape
    s = int(s)
    y = torch.empty((n, g, s * h, s * w, 8), dtype=torch.float16, device=x.device)
    _timed("bilinear_up_h8_kernel", f"N{n} bilinear x{s} {8 * g}ch {h}x{w}", 7.0 * y.numel(), 2.0 * (x.numel() + y.numel()),
           lambda: check(_lib.load().slu_bilinear_upsample_h8(x.data_ptr(), y.data_ptr(), n, g, h, w, s, _stream()), "slu_bilinear_upsample_h8"))
    return y


def _req_gn(x: torch.Tensor, channels: int, groups: int, what: str):
    _req_h8(x, "x")
    n, g, h, w, _ = x.shape
    c, groups = int(channels), int(groups)
    if not 8 * (g - 1) < c <= 8 * g or groups < 1 or c % groups:
        raise RuntimeError(f"{what}: {c} channels in {groups} groups do not fit the {g} blocks of x")
    return n, g, h, w, c, groups


def groupnorm_stats_h8(x: torch.Tensor, channels: int, groups: int, eps: float = 1e-5) -> torch.Tensor:
    """[2, N * groups] fp32 (mean, rstd) of nn.GroupNorm(groups, channels, eps) over the stored values of an h8 tensor
    (slu_groupnorm_stats_h8; groups 1, 2, 4 or 8 channels wide, anything else raises)."""
    n, g, h, w, c, groups = _req_gn(x, channels, groups, "groupnorm_stats_h8")
    lib = _lib.load()
    stats = torch.empty((2, n * groups), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(1, lib.slu_groupnorm_stats_h8_workspace_bytes(n, c, h * w) // 8), dtype=torch.float64, device=x.device)
    _timed("groupnorm_partial_h8_kernel", f"N{n} GroupNorm({groups}, {c}) statistics {h}x{w}", 3.0 * x.numel(), 2.0 * x.numel(),
           lambda: check(lib.slu_groupnorm_stats_h8(x.data_ptr(), n, c, h * w, groups, float(eps), stats[0].data_ptr(), stats[1].data_ptr(),
                                                    ws.data_ptr(), _stream()), "slu_groupnorm_stats_h8"))
    return stats


def groupnorm_apply_h8(x: torch.Tensor, channels: int, groups: int, stats: torch.Tensor, gamma: Optional[torch.Tensor],
                       beta: Optional[torch.Tensor], relu: bool = False, out: Optional[torch.Tensor] = None, g_off: int = 0) -> torch.Tensor:
    """(x - mean) * rstd * gamma + beta [-> ReLU] with stats = groupnorm_stats_h8(x, channels, groups), into blocks [g_off, g_off + G) of `out`
    ([N, Gtot, H, W, 8]; a new tensor of G blocks when None; `out is x`: in place).  slu_groupnorm_apply_h8."""
    n, g, h, w, c, groups = _req_gn(x, channels, groups, "groupnorm_apply_h8")
    _req(stats, "stats")
    if tuple(stats.shape) != (2, n * groups):
        raise RuntimeError(f"stats: expected {(2, n * groups)}, got {tuple(stats.shape)}")
    for t, nme in ((gamma, "gamma"), (beta, "beta")):
        if t is not None:
            _req(t, nme)
            if t.numel() != c:
                raise RuntimeError(f"{nme}: expected {c} elements, got {t.numel()}")
    if out is None:
        out = torch.empty_like(x)
    _req_h8(out, "out")
    g_off = int(g_off)
    if (out.shape[0], out.shape[2], out.shape[3]) != (n, h, w) or g_off < 0 or g_off + g > out.shape[1]:
        raise RuntimeError(f"out: blocks [{g_off}, {g_off + g}) of {tuple(out.shape)} do not take {(n, g, h, w, 8)}")
    if out.data_ptr() == x.data_ptr() and (out.shape[1] != g or g_off):
        raise RuntimeError("groupnorm_apply_h8: in place only as the whole tensor")
    _timed("groupnorm_apply_h8_kernel", f"N{n} GroupNorm({groups}, {c}) apply{' + ReLU' if relu else ''} {h}x{w}", 3.0 * x.numel(), 4.0 * x.numel(),
           lambda: check(_lib.load().slu_groupnorm_apply_h8(x.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), _ptr(gamma), _ptr(beta),
                                                            1 if relu else 0, out.data_ptr(), n, c, h * w, groups, out.shape[1], g_off, _stream()),
                         "slu_groupnorm_apply_h8"))
    return out


def spatial_softmax_gate_h8(x: torch.Tensor, score: torch.Tensor) -> torch.Tensor:
    """x * softmax(score over H * W) + x (SpatialAttention of semanticFCN_opt): x h8 [N, G, H, W, 8], score fp32 [N, 1, H, W]
    (slu_spatial_softmax_gate_h8)."""
    _req_h8(x, "x")
    _req(score, "score")
    n, g, h, w, _ = x.shape
    if tuple(score.shape) != (n, 1, h, w):
        raise RuntimeError(f"spatial_softmax_gate_h8: score [N, 1, H, W] = {(n, 1, h, w)} expected, got {tuple(score.shape)}")
    stats = torch.empty(2 * n, dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    _timed("spatial_gate_h8_kernel", f"N{n} softmax(H W) gate {8 * g}ch {h}x{w}", 2.0 * x.numel(), 4.0 * x.numel() + 8.0 * score.numel(),
           lambda: check(_lib.load().slu_spatial_softmax_gate_h8(x.data_ptr(), score.data_ptr(), stats.data_ptr(), out.data_ptr(), n, 8 * g, h * w,
                                                                 _stream()), "slu_spatial_softmax_gate_h8"))
    return out
