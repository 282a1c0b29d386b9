"""Thin, checked Python wrappers over the C ABI (include/slu.h).

torch tensors own the memory; every function validates device / dtype / contiguity / shape on the
host before the launch (a wrong shape must never reach a hand-written kernel) and launches on
torch's current HIP stream.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from ._lib import ConvDesc, check

INT64_MIN = -(2 ** 63)

# bench.py sets this to a list to collect (kernel name, algorithmic flops, algorithmic bytes, ev0, ev1)
# per conv launch; None (the default) adds nothing to the launch path.
TIMING = None
TIMING_TAGS = []


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on '{t.device}'; the HIP path only runs on a GPU (no CPU fallback)")
    if t.device.index != torch.cuda.current_device():
        # launches go to the CURRENT device's stream; a tensor living on another GPU would be dereferenced there
        raise RuntimeError(f"{name}: tensor is on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                           "call torch.cuda.set_device(local_rank) (distributed.init_from_env does) or use `with torch.cuda.device(t.device)`")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: tensor must be contiguous")
    return t


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req_shapes(*items) -> None:
    """(tensor, name, shape) ...: _req, and the shape."""
    for t, nme, shp in items:
        _req(t, nme)
        if tuple(t.shape) != shp:
            raise RuntimeError(f"{nme}: expected {shp}, got {tuple(t.shape)}")


def _overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.data_ptr() < b.data_ptr() + b.numel() * b.element_size() and b.data_ptr() < a.data_ptr() + a.numel() * a.element_size()


def _out_or_new(fn: str, out: Optional[torch.Tensor], shape, inputs) -> torch.Tensor:
    """A new float32 tensor next to inputs[0], or the caller's `out`: checked, of this shape, overlapping none of `inputs` (None entries skipped)."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=inputs[0].device)
    _req(out, "out")
    if tuple(out.shape) != tuple(shape):
        raise RuntimeError(f"out: expected {tuple(shape)}, got {tuple(out.shape)}")
    if any(t is not None and _overlaps(out, t) for t in inputs):
        raise RuntimeError(f"{fn}: out must not overlap an input")
    return out


# ------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------
class ConvSource(NamedTuple):
    """One channel-concatenated input of a fused conv."""
    tensor: torch.Tensor                    # [N,C,H,W], or [N,C,H/2,W/2] when pixel_shuffle
    scale: Optional[torch.Tensor] = None    # [N,C] multiplier (folded Dropout2d) or None
    pixel_shuffle: bool = False
    nbatch: int = 0                         # > 0: tensor holds nbatch images, output image n reads image n % nbatch
    cuse: int = 0                           # > 0: only the first cuse channels of the tensor contribute
    coff: int = 0                           # > 0: the channels read start at coff (x[:, coff:coff + cuse]); needs cuse, no scale / pixel_shuffle


def conv_ck(ksize: int) -> int:
    return _lib.load().slu_conv_ck(ksize)


def pack_conv_weight(weight: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 weight -> MFMA A-fragment image (re-run after every weight update)."""
    _req(weight, "weight")
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise RuntimeError(f"weight: expected [Cout,Cin,k,k], got {tuple(weight.shape)}")
    lib = _lib.load()
    cout, cin, ks, _ = weight.shape
    ck = lib.slu_conv_ck(ks)
    n = lib.slu_packed_weight_floats(cout, cin, ks, ck)
    if n == 0:
        raise RuntimeError("pack_conv_weight: unsupported weight shape")
    out = torch.empty(n, dtype=torch.float32, device=weight.device)
    check(lib.slu_pack_conv_weight(weight.data_ptr(), cout, cin, ks, ck, out.data_ptr(), _stream()), "slu_pack_conv_weight")
    return out


class WeightPackPlan:
    """The forward AND data-gradient MFMA images of a list of conv weights, rebuilt by ONE launch (slu_pack_conv_weights_multi) into buffers
    that keep their addresses: `fwd[i]` == pack_conv_weight(w_i), `dgrad[i]` == pack_conv_weight(dgrad_weight(w_i)).  The plan records the
    weights' addresses; `matches(weights)` tells whether it still describes them (a parameter that was re-allocated needs a new plan)."""

    def __init__(self, weights: Sequence[torch.Tensor]):
        lib = _lib.load()
        self.ptrs = [w.data_ptr() for w in weights]
        self.fwd, self.dgrad = [], []
        jobs = (_lib.PackJob * (2 * len(weights)))()
        begin = 0
        for i, w in enumerate(weights):
            _req(w, f"weights[{i}]")
            if w.dim() != 4 or w.shape[2] != w.shape[3]:
                raise RuntimeError(f"weights[{i}]: expected [Cout,Cin,k,k], got {tuple(w.shape)}")
            cout, cin, ks, _ = w.shape
            ck = lib.slu_conv_ck(ks)
            for d, (co, ci), store in ((0, (cout, cin), self.fwd), (1, (cin, cout), self.dgrad)):
                n = lib.slu_packed_weight_floats(co, ci, ks, ck)
                if n == 0:
                    raise RuntimeError(f"weights[{i}]: unsupported shape {tuple(w.shape)}")
                out = torch.empty(n, dtype=torch.float32, device=w.device)
                store.append(out)
                j = jobs[2 * i + d]
                j.w, j.out, j.cout, j.cin, j.ksize, j.ck, j.dgrad, j.begin = w.data_ptr(), out.data_ptr(), cout, cin, ks, ck, d, begin
                begin += n
        self.total, self.njobs = begin, 2 * len(weights)
        import ctypes
        raw = bytes(ctypes.string_at(ctypes.addressof(jobs), ctypes.sizeof(jobs)))
        self.jobs = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(weights[0].device)

    def matches(self, weights: Sequence[torch.Tensor]) -> bool:
        return len(weights) == len(self.ptrs) and all(w.data_ptr() == p for w, p in zip(weights, self.ptrs))

    def run(self) -> None:
        check(_lib.load().slu_pack_conv_weights_multi(self.jobs.data_ptr(), self.njobs, self.total, _stream()), "slu_pack_conv_weights_multi")


def pack_conv_weight_f16x3(weight: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 weight -> split-fp16 (hi, lo) MFMA A-fragment image for precision='f16x3'.
    Each weight is stored as hi = fp16(w) toward zero and lo = fp16(w - hi): 22 bits while lo is a normal fp16 (|w| >= 2^-3), an absolute
    error of 2^-24 below that.  The conv stays within 2e-5 of its output scale while the weights (and the inputs) have rms >= 2^-8 (4e-3);
    smaller weights -- BatchNorm-folded ones can be -- lose accuracy as 2^-24 / rms|w|."""
    _req(weight, "weight")
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise RuntimeError(f"weight: expected [Cout,Cin,k,k], got {tuple(weight.shape)}")
    lib = _lib.load()
    cout, cin, ks, _ = weight.shape
    n = lib.slu_packed_weight_bytes_f16x3(cout, cin, ks)
    if n == 0:
        raise RuntimeError("pack_conv_weight_f16x3: unsupported weight shape")
    out = torch.empty(n, dtype=torch.uint8, device=weight.device)
    check(lib.slu_pack_conv_weight_f16x3(weight.data_ptr(), cout, cin, ks, out.data_ptr(), _stream()), "slu_pack_conv_weight_f16x3")
    return out


PRECISIONS = {"fp32": 0, "f16x3": 1}


def bn_fold(gamma, beta, mean, var, eps: float):
    """(a, b) with  a*x + b == eval BatchNorm(x)."""
    c = gamma.numel()
    for t, nme in ((gamma, "gamma"), (beta, "beta"), (mean, "running_mean"), (var, "running_var")):
        _req(t, nme)
        if t.numel() != c:
            raise RuntimeError("bn_fold: size mismatch")
    a = torch.empty(c, dtype=torch.float32, device=gamma.device)
    b = torch.empty_like(a)
    check(_lib.load().slu_bn_fold(gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), float(eps), c,
                                  a.data_ptr(), b.data_ptr(), _stream()), "slu_bn_fold")
    return a, b


def conv2d_fused(srcs: Sequence[ConvSource], wpack: torch.Tensor, cout: int, ksize: int, dil: int, pad: int,
                 bias: Optional[torch.Tensor] = None, slope: Optional[float] = None,
                 bn_a: Optional[torch.Tensor] = None, bn_b: Optional[torch.Tensor] = None,
                 resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 precision: str = "fp32", act: Optional[str] = None, act_after_resid: bool = False,
                 stats: Optional[torch.Tensor] = None, n_out: Optional[int] = None) -> torch.Tensor:
    """out = resid + bn_a * leaky(conv(cat(srcs)) + bias) + bn_b   (see slu_conv2d_fwd).
    precision 'fp32' (exact, wpack from pack_conv_weight) or 'f16x3' (split-fp16, wpack from pack_conv_weight_f16x3).
    'f16x3' is within (2^-21 + 2^-24 / rms|x| + 2^-24 / rms|w|) of the output scale of the exact result: ~1e-6 for O(1) operands, 2e-5 while
    both operands have rms >= 2^-8, worse below; |x| above 65504 is carried by the lo part up to 131008.
    n_out: the output batch, for a conv whose sources are all batch-broadcast (`ConvSource.nbatch`); otherwise it is the first source's."""
    if precision not in PRECISIONS:
        raise ValueError(f"unknown conv precision {precision!r}")
    lib = _lib.load()
    if not 1 <= len(srcs) <= _lib.MAX_SRC:
        raise RuntimeError(f"conv2d_fused: 1..{_lib.MAX_SRC} sources supported, got {len(srcs)}")
    d = ConvDesc()
    n = h = w = None
    if n_out is not None:
        n = int(n_out)
        if n < 1:
            raise RuntimeError("conv2d_fused: n_out must be positive")
    cin = 0
    keep = []
    for i, s in enumerate(srcs):
        t = _req(s.tensor, f"src[{i}]")
        if t.dim() != 4:
            raise RuntimeError(f"src[{i}]: expected NCHW, got {tuple(t.shape)}")
        sn, sc, sh, sw = t.shape
        if s.pixel_shuffle:
            if sc % 4:
                raise RuntimeError(f"src[{i}]: PixelShuffle(2) needs C % 4 == 0")
            sh, sw, contributed = sh * 2, sw * 2, sc // 4
        elif s.cuse:
            if not 0 < s.cuse <= sc:
                raise RuntimeError(f"src[{i}]: cuse must be in 1..C")
            contributed = s.cuse
        else:
            contributed = sc
        if s.coff:
            # a channel range x[:, coff:coff + cuse] is the prefix of the tensor that starts coff planes later with the same batch stride: the
            # kernels bound every channel they read by `cuse` (a ragged last K-chunk reads element 0 of the source instead), so nothing past
            # plane coff + cuse - 1 of the last image is touched
            if s.pixel_shuffle or s.scale is not None or not s.cuse or s.coff < 0 or s.coff + s.cuse > sc:
                raise RuntimeError(f"src[{i}]: coff needs cuse with coff + cuse <= C and neither scale nor pixel_shuffle")
        if s.nbatch:
            if n is None or sn != s.nbatch or n % sn:
                raise RuntimeError(f"src[{i}]: a batch-broadcast source must follow a full-batch source (or n_out be given) and divide N")
            sn = n
        if h is None:
            n, h, w = sn if n is None else n, sh, sw
        if (sn, sh, sw) != (n, h, w):
            raise RuntimeError(f"src[{i}]: spatial/batch size {(sn, sh, sw)} != {(n, h, w)}")
        if s.scale is not None:
            _req(s.scale, f"src[{i}].scale")
            if tuple(s.scale.shape) != (sn, sc):
                raise RuntimeError(f"src[{i}].scale: expected {(sn, sc)}, got {tuple(s.scale.shape)}")
        d.src[i].nbatch = int(s.nbatch)
        d.src[i].cuse = int(s.cuse)
        d.src[i].ptr = t.data_ptr() + 4 * int(s.coff) * sh * sw
        d.src[i].scale = _ptr(s.scale)
        d.src[i].C = sc
        d.src[i].pixel_shuffle = 1 if s.pixel_shuffle else 0
        cin += contributed
        keep.append(t)
    if precision == "f16x3":
        ck = 16
        _req(wpack, "wpack", torch.uint8)
        if wpack.numel() != lib.slu_packed_weight_bytes_f16x3(cout, cin, ksize):
            raise RuntimeError(f"wpack: {wpack.numel()} bytes does not match Cout={cout} Cin={cin} k={ksize} (f16x3)")
    else:
        ck = lib.slu_conv_ck(ksize)
        _req(wpack, "wpack")
        if wpack.numel() != lib.slu_packed_weight_floats(cout, cin, ksize, ck):
            raise RuntimeError(f"wpack: {wpack.numel()} floats does not match Cout={cout} Cin={cin} k={ksize}")
    for t, nme in ((bias, "bias"), (bn_a, "bn_a"), (bn_b, "bn_b")):
        if t is not None:
            _req(t, nme)
            if t.numel() != cout:
                raise RuntimeError(f"{nme}: expected {cout} elements, got {t.numel()}")
    if (bn_a is None) != (bn_b is None):
        raise RuntimeError("bn_a and bn_b must be given together")
    if out is None:
        out = torch.empty((n, cout, h, w), dtype=torch.float32, device=keep[0].device)
    else:
        _req(out, "out")
        if tuple(out.shape) != (n, cout, h, w):
            raise RuntimeError(f"out: expected {(n, cout, h, w)}, got {tuple(out.shape)}")
    if resid is not None:
        _req(resid, "resid")
        if tuple(resid.shape) != (n, cout, h, w):
            raise RuntimeError(f"resid: expected {(n, cout, h, w)}, got {tuple(resid.shape)}")
    d.nsrc = len(srcs)
    d.N, d.H, d.W, d.Cin, d.Cout = n, h, w, cin, cout
    d.ksize, d.dil, d.pad, d.ck = ksize, dil, pad, ck
    d.wpack, d.bias = wpack.data_ptr(), _ptr(bias)
    d.has_act, d.slope = (0, 0.0) if slope is None else (1, float(slope))
    if act is not None:                     # explicit activation kind overrides `slope`
        if act not in ("relu", "tanh", "silu", "none"):
            raise ValueError(f"unknown activation {act!r}")
        d.has_act, d.slope = {"relu": (1, 0.0), "tanh": (2, 0.0), "silu": (3, 0.0), "none": (0, 0.0)}[act]
        if act_after_resid and act in ("tanh", "silu"):
            raise ValueError(f"activation {act!r} has no after-the-residual form")
    if act_after_resid and d.has_act:
        d.has_act |= 4
    d.bn_a, d.bn_b, d.resid, d.out = _ptr(bn_a), _ptr(bn_b), _ptr(resid), out.data_ptr()
    d.precision = PRECISIONS[precision]
    if stats is not None:
        # per-channel sum / sum of squares of the stored output, added into `stats` (f64 [2, Cout], zeroed by the caller)
        _req(stats, "stats", torch.float64)
        if tuple(stats.shape) != (2, cout) or precision != "fp32":
            raise RuntimeError("stats: expected a float64 [2, Cout] tensor with precision='fp32'")
        d.stats = stats.data_ptr()
    if TIMING is None:
        check(lib.slu_conv2d_fwd(C.byref(d), _stream()), "slu_conv2d_fwd")
        return out
    # measurement mode (bench.py): HIP events on the launch stream around this one kernel
    buf = C.create_string_buffer(64)
    check(lib.slu_conv2d_kernel_name(C.byref(d), buf, 64), "slu_conv2d_kernel_name")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.slu_conv2d_fwd(C.byref(d), _stream()), "slu_conv2d_fwd")
    e1.record()
    flops = 2.0 * cin * cout * ksize * ksize * n * h * w
    nbytes = 4.0 * (n * h * w * (cin + cout) + cout * cin * ksize * ksize)
    TIMING.append((buf.value.decode(), flops, nbytes, e0, e1))
    TIMING_TAGS.append(f"N{n} {cin}->{cout} k{ksize}d{dil} {h}x{w}")
    return out


def avgpool3s2_bcast(x: torch.Tensor, scale: Optional[torch.Tensor], n_out: int) -> torch.Tensor:
    """avgpool3s2 of x[n % B] * scale[n] for n < n_out: pools a B-image tensor into n_out = T*B stacked passes."""
    _req(x, "x")
    b, c, h, w = x.shape
    if n_out % b:
        raise RuntimeError("avgpool3s2_bcast: n_out must be a multiple of the input batch")
    if scale is not None:
        _req(scale, "scale")
        if tuple(scale.shape) != (n_out, c):
            raise RuntimeError(f"scale: expected {(n_out, c)}, got {tuple(scale.shape)}")
    y = torch.empty((n_out, c, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_avgpool3s2_bcast_fwd(x.data_ptr(), _ptr(scale), y.data_ptr(), n_out, b, c, h, w, _stream()),
          "slu_avgpool3s2_bcast_fwd")
    return y


def avgpool3s2(x: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req(x, "x")
    n, c, h, w = x.shape
    if scale is not None:
        _req(scale, "scale")
        if tuple(scale.shape) != (n, c):
            raise RuntimeError(f"scale: expected {(n, c)}, got {tuple(scale.shape)}")
    y = torch.empty((n, c, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_avgpool3s2_fwd(x.data_ptr(), _ptr(scale), y.data_ptr(), n, c, h, w, _stream()), "slu_avgpool3s2_fwd")
    return y


# ------------------------------------------------------------------------------------------------
# uncertainty / loss / metrics
# ------------------------------------------------------------------------------------------------
def mc_reduce(mc_logits: torch.Tensor, eps: float = 1e-12):
    """[T,B,C,H,W] logits -> (p_bar[B,C,H,W], H_norm[B,H,W], MI_norm[B,H,W], preds[B,H,W] int64)."""
    _req(mc_logits, "mc_logits")
    if mc_logits.dim() != 5:
        raise RuntimeError(f"mc_logits: expected [T,B,C,H,W], got {tuple(mc_logits.shape)}")
    t, b, c, h, w = mc_logits.shape
    dev = mc_logits.device
    p_bar = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
    hn = torch.empty((b, h, w), dtype=torch.float32, device=dev)
    mi = torch.empty((b, h, w), dtype=torch.float32, device=dev)
    preds = torch.empty((b, h, w), dtype=torch.int64, device=dev)
    check(_lib.load().slu_mc_reduce(mc_logits.data_ptr(), t, b, c, h * w, float(eps), p_bar.data_ptr(), hn.data_ptr(),
                                    mi.data_ptr(), preds.data_ptr(), _stream()), "slu_mc_reduce")
    return p_bar, hn, mi, preds


def softmax_entropy(logits: torch.Tensor, eps: float = 1e-8):
    """[B,C,H,W] logits -> (probs, H_norm[B,H,W], preds[B,H,W] int64)."""
    _req(logits, "logits")
    b, c, h, w = logits.shape
    dev = logits.device
    probs = torch.empty_like(logits)
    hn = torch.empty((b, h, w), dtype=torch.float32, device=dev)
    preds = torch.empty((b, h, w), dtype=torch.int64, device=dev)
    check(_lib.load().slu_softmax_entropy(logits.data_ptr(), b, c, h * w, float(eps), probs.data_ptr(), hn.data_ptr(),
                                          preds.data_ptr(), _stream()), "slu_softmax_entropy")
    return probs, hn, preds


def confusion_update(confmat: torch.Tensor, preds: torch.Tensor, targets: torch.Tensor) -> None:
    """confmat[C,C] int64 (rows = GT) += bincount(t*C+p) over in-range pairs, in place."""
    _req(confmat, "confmat", torch.int64)
    _req(preds, "preds", torch.int64)
    _req(targets, "targets", torch.int64)
    if preds.numel() != targets.numel():
        raise RuntimeError("preds/targets size mismatch")
    c = confmat.shape[0]
    if confmat.dim() != 2 or confmat.shape[1] != c:
        raise RuntimeError("confmat must be [C,C]")
    check(_lib.load().slu_confusion_update(preds.data_ptr(), targets.data_ptr(), preds.numel(), c, confmat.data_ptr(),
                                           _stream()), "slu_confusion_update")


def ece_update(probs, labels, count, sum_correct, sum_conf, ignore_index=None) -> None:
    """Accumulate top-label calibration bins in place (count int64[nb], sums float64[nb])."""
    _req(probs, "probs")
    _req(labels, "labels", torch.int64)
    _req(count, "count", torch.int64)
    _req(sum_correct, "sum_correct", torch.float64)
    _req(sum_conf, "sum_conf", torch.float64)
    b, c, h, w = probs.shape
    if labels.numel() != b * h * w:
        raise RuntimeError("labels size mismatch")
    nb = count.numel()
    if sum_correct.numel() != nb or sum_conf.numel() != nb:
        raise RuntimeError("bin accumulator size mismatch")
    ign = INT64_MIN if ignore_index is None else int(ignore_index)
    check(_lib.load().slu_ece_update(probs.data_ptr(), labels.data_ptr(), b, c, h * w, ign, nb, count.data_ptr(),
                                     sum_correct.data_ptr(), sum_conf.data_ptr(), _stream()), "slu_ece_update")


def softmax_nll(logits: torch.Tensor, labels: torch.Tensor, clamp: float = 1e-8, want_probs: bool = True):
    """(probs or None, nll_sum float64[1]) : sum over pixels of -ln max(softmax(logits)[label], clamp)."""
    _req(logits, "logits")
    _req(labels, "labels", torch.int64)
    b, c, h, w = logits.shape
    if labels.numel() != b * h * w:
        raise RuntimeError("labels size mismatch")
    probs = torch.empty_like(logits) if want_probs else None
    acc = torch.zeros(1, dtype=torch.float64, device=logits.device)
    check(_lib.load().slu_softmax_nll_fwd(logits.data_ptr(), labels.data_ptr(), b, c, h * w, float(clamp), _ptr(probs),
                                          acc.data_ptr(), _stream()), "slu_softmax_nll_fwd")
    return probs, acc


# ------------------------------------------------------------------------------------------------
# loss kernels
# ------------------------------------------------------------------------------------------------
NLL_LOGITS, NLL_PROBS_CLAMP, NLL_PROBS_EPS, NLL_LOG_PROBS = 0, 1, 2, 3


def lovasz_class_mask(classes, c: int) -> int:
    """The kernel's class set for the reference's `classes` argument (lovasz.py:66): 0 = 'present'."""
    if classes == "present":
        return 0
    ids = range(c) if classes == "all" else [int(k) for k in classes]
    mask = 0
    for k in ids:
        if not 0 <= k < c:
            raise IndexError(f"Lovasz: class {k} out of range for {c} classes")      # the reference indexes probas[:, k]
        mask |= 1 << k
    if mask == 0:
        raise ValueError("Lovasz: empty class list")
    return mask


def lovasz_fwd(probs: torch.Tensor, labels: torch.Tensor, ignore_index=None, want_grad: bool = True, classes="present"):
    """(loss f32[1], n_summed f32[1], grad_probs [B,C,H,W] or None) -- Lovasz-Softmax over the present classes, all classes or a list."""
    _req(probs, "probs")
    _req(labels, "labels", torch.int64)
    b, c, h, w = probs.shape
    if labels.numel() != b * h * w:
        raise RuntimeError("labels size mismatch")
    lib = _lib.load()
    nbytes = lib.slu_lovasz_workspace_bytes(b, c, h * w)
    if nbytes == 0:
        raise RuntimeError("lovasz: unsupported shape")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=probs.device)
    loss = torch.empty(1, dtype=torch.float32, device=probs.device)
    npres = torch.empty(1, dtype=torch.float32, device=probs.device)
    grad = torch.empty_like(probs) if want_grad else None
    ign = INT64_MIN if ignore_index is None else int(ignore_index)
    check(lib.slu_lovasz_fwd(probs.data_ptr(), labels.data_ptr(), b, c, h * w, ign, lovasz_class_mask(classes, c), ws.data_ptr(), nbytes, loss.data_ptr(),
                             npres.data_ptr(), _ptr(grad), _stream()), "slu_lovasz_fwd")
    return loss, npres, grad


def nll_fwd(x: torch.Tensor, labels: torch.Tensor, kind: int, param: float = 0.0, ignore_index=None):
    """(nll_sum f64[1], count i64[1]) over pixels whose label is in [0,C) and != ignore_index."""
    _req(x, "x")
    _req(labels, "labels", torch.int64)
    b, c, h, w = x.shape
    if labels.numel() != b * h * w:
        raise RuntimeError("labels size mismatch")
    acc = torch.zeros(1, dtype=torch.float64, device=x.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=x.device)
    ign = INT64_MIN if ignore_index is None else int(ignore_index)
    check(_lib.load().slu_nll_fwd(x.data_ptr(), labels.data_ptr(), b, c, h * w, int(kind), float(param), ign, acc.data_ptr(),
                                  cnt.data_ptr(), _stream()), "slu_nll_fwd")
    return acc, cnt


def nll_bwd(x, labels, kind: int, param: float, ignore_index, gscale: torch.Tensor):
    """grad_x = gscale[0] * d(sum nll)/dx ; gscale is a 1-element fp32 device tensor."""
    _req(x, "x")
    _req(labels, "labels", torch.int64)
    _req(gscale, "gscale")
    b, c, h, w = x.shape
    g = torch.empty_like(x)
    ign = INT64_MIN if ignore_index is None else int(ignore_index)
    check(_lib.load().slu_nll_bwd(x.data_ptr(), labels.data_ptr(), b, c, h * w, int(kind), float(param), ign, gscale.data_ptr(),
                                  g.data_ptr(), _stream()), "slu_nll_bwd")
    return g


def softmax_loss_bwd(probs, labels=None, dense=None, w_dense: float = 1.0, w_nll: float = 0.0, clamp: float = 0.0, gout=None):
    """grad_logits = softmax backward of gout * (w_dense * dense - [c==y, p_y>=clamp] * w_nll / p_y)."""
    _req(probs, "probs")
    b, c, h, w = probs.shape
    if labels is not None:
        _req(labels, "labels", torch.int64)
    if dense is not None:
        _req(dense, "dense")
        if dense.shape != probs.shape:
            raise RuntimeError("dense gradient shape mismatch")
    if gout is not None:
        _req(gout, "gout")
    g = torch.empty_like(probs)
    check(_lib.load().slu_softmax_loss_bwd(probs.data_ptr(), _ptr(labels), _ptr(dense), float(w_dense), float(w_nll), float(clamp),
                                           _ptr(gout), b, c, h * w, g.data_ptr(), _stream()), "slu_softmax_loss_bwd")
    return g


# ------------------------------------------------------------------------------------------------
# training-side kernels
# ------------------------------------------------------------------------------------------------
def _fill_srcs(arr, srcs):
    n = h = w = None
    for i, s in enumerate(srcs):
        t = _req(s.tensor, f"src[{i}]")
        sn, sc, sh, sw = t.shape
        if s.coff:
            raise RuntimeError(f"src[{i}]: a channel offset is only read by the forward conv")
        if s.pixel_shuffle:
            sh, sw = sh * 2, sw * 2
        if n is None:
            n, h, w = sn, sh, sw
        elif (sn, sh, sw) != (n, h, w):
            raise RuntimeError(f"src[{i}]: size mismatch")
        if s.scale is not None:
            _req(s.scale, f"src[{i}].scale")
            if tuple(s.scale.shape) != (sn, sc):
                raise RuntimeError(f"src[{i}].scale: expected {(sn, sc)}")
        arr[i].ptr, arr[i].scale, arr[i].C, arr[i].pixel_shuffle = t.data_ptr(), _ptr(s.scale), sc, 1 if s.pixel_shuffle else 0
    return n, h, w


class _ZeroArena:
    """fp64 zeros by the slice.  A training step needs ~140 tiny zero-initialised accumulators (BatchNorm sums, bias gradients): one fill
    launch each was 0.6 ms of a 34 ms step.  A chunk is zeroed ONCE and handed out slice by slice -- every slice is used exactly once, as
    the accumulator a kernel adds into; an exhausted chunk is dropped (the views handed out keep it alive) and a new one zeroed.  While a
    stream is being captured into a HIP graph the plain torch.zeros is used (its fill is part of the graph and re-runs on replay)."""
    CHUNK = 1 << 16

    def __init__(self):
        self._chunks = {}          # (device, stream) -> [tensor, next free element]

    def take(self, shape, device) -> torch.Tensor:
        n = 1
        for d in shape:
            n *= int(d)
        if n > self.CHUNK // 4 or torch.cuda.is_current_stream_capturing():
            return torch.zeros(shape, dtype=torch.float64, device=device)
        # one chunk per (device, stream): the fill is ordered before the consumers only on the stream it was issued on, and the caching
        # allocator may hand a dropped chunk's block out again on that stream while another stream's kernels still add into it (the dropout
        # side stream and the graph warm-up stream of this package are real second streams)
        dev = torch.device(device)
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        ent = self._chunks.get(key)
        if ent is None or ent[1] + n > self.CHUNK:
            ent = self._chunks[key] = [torch.zeros(self.CHUNK, dtype=torch.float64, device=device), 0]
        out = ent[0][ent[1]:ent[1] + n].view(shape)
        ent[1] += n
        return out


_ZEROS64 = _ZeroArena()


class _ZeroArenaF32(_ZeroArena):
    """The same for the fp32 accumulators of the weight-gradient kernels (split-K partial sums added with atomics: the packed scratch of the
    3x3 / 2x2 families, the gradient itself for the 1x1 family): SalsaNext's ~50 of them total 7 M floats per step, one fill instead of 50.
    Slices start on 256-byte boundaries."""
    CHUNK = 1 << 23

    def take(self, n: int, device) -> torch.Tensor:
        n = int(n)
        if n > self.CHUNK // 2 or torch.cuda.is_current_stream_capturing():
            return torch.zeros(n, dtype=torch.float32, device=device)
        dev = torch.device(device)
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        ent = self._chunks.get(key)
        if ent is None or ent[1] + n > self.CHUNK:
            ent = self._chunks[key] = [torch.zeros(self.CHUNK, dtype=torch.float32, device=device), 0]
        out = ent[0][ent[1]:ent[1] + n]
        ent[1] += (n + 63) // 64 * 64
        return out


_ZEROS32 = _ZeroArenaF32()


def zeros_f64(shape, device) -> torch.Tensor:
    """A zero-filled float64 accumulator that is written once (see _ZeroArena)."""
    return _ZEROS64.take(tuple(shape) if not isinstance(shape, int) else (shape,), device)


def bn_stats(y: torch.Tensor):
    """(sum f64[C], sumsq f64[C]) over (N,H,W)."""
    _req(y, "y")
    n, c, h, w = y.shape
    sq = zeros_f64((2, c), y.device)
    s, q = sq[0], sq[1]
    check(_lib.load().slu_bn_stats(y.data_ptr(), n, c, h * w, s.data_ptr(), q.data_ptr(), _stream()), "slu_bn_stats")
    return s, q


def bn_bwd_reduce(dz, y, mean, invstd):
    """(sum dz, sum dz*xhat) per channel, f64."""
    for t, nme in ((dz, "dz"), (y, "y"), (mean, "mean"), (invstd, "invstd")):
        _req(t, nme)
    if dz.shape != y.shape:
        raise RuntimeError("dz / y shape mismatch")
    n, c, h, w = y.shape
    s12 = zeros_f64((2, c), y.device)
    s1, s2 = s12[0], s12[1]
    check(_lib.load().slu_bn_bwd_reduce(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), n, c, h * w, s1.data_ptr(),
                                        s2.data_ptr(), _stream()), "slu_bn_bwd_reduce")
    return s1, s2


def bn_coeffs_fwd(sums, count: float, gamma, beta, eps: float, momentum: float, running_mean, running_var, train: bool):
    """(mean, invstd, a, b) [C] fp32 in one launch; in train mode the running statistics are updated in place."""
    c = gamma.numel()
    dev = gamma.device
    out = torch.empty((4, c), dtype=torch.float32, device=dev)
    s, q = (sums if sums is not None else (None, None))
    for t, nme in ((gamma, "gamma"), (beta, "beta")):
        _req(t, nme)
    if running_mean is not None:
        _req(running_mean, "running_mean")
        _req(running_var, "running_var")
    check(_lib.load().slu_bn_coeffs_fwd(_ptr(s), _ptr(q), float(count), gamma.data_ptr(), beta.data_ptr(), float(eps), float(momentum),
                                        1 if train else 0, _ptr(running_mean), _ptr(running_var), c, out[0].data_ptr(), out[1].data_ptr(),
                                        out[2].data_ptr(), out[3].data_ptr(), _stream()), "slu_bn_coeffs_fwd")
    if train and running_mean is not None:
        # the kernel wrote the running statistics through raw pointers: tell torch, so that caches keyed on tensor versions
        # (salsanext._tkey: folded eval-BatchNorm coefficients) see the change
        torch.autograd.graph.increment_version(running_mean)
        torch.autograd.graph.increment_version(running_var)
    return out[0], out[1], out[2], out[3]


def bn_coeffs_bwd(s1, s2, count: float, gamma, mean, invstd, train: bool):
    """(k1, k2, k3, dgamma, dbeta) [C] fp32 in one launch."""
    c = gamma.numel()
    out = torch.empty((5, c), dtype=torch.float32, device=gamma.device)
    check(_lib.load().slu_bn_coeffs_bwd(s1.data_ptr(), s2.data_ptr(), float(count), gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                        1 if train else 0, c, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                        out[4].data_ptr(), _stream()), "slu_bn_coeffs_bwd")
    return out[0], out[1], out[2], out[3], out[4]


def affine(y, a=None, b=None, resid=None):
    """z = a[c]*y + b[c] + resid."""
    _req(y, "y")
    n, c, h, w = y.shape
    for t, nme in ((a, "a"), (b, "b")):
        if t is not None:
            _req(t, nme)
            if t.numel() != c:
                raise RuntimeError(f"{nme}: expected {c} elements")
    if resid is not None:
        _req(resid, "resid")
        if resid.shape != y.shape:
            raise RuntimeError("resid shape mismatch")
    z = torch.empty_like(y)
    check(_lib.load().slu_affine_fwd(y.data_ptr(), _ptr(a), _ptr(b), _ptr(resid), z.data_ptr(), n, c, h * w, _stream()), "slu_affine_fwd")
    return z


def bn_apply_fwd(y, sums, count: float, gamma, beta, eps: float, momentum: float, running_mean, running_var, train: bool, resid=None):
    """(z, mean, invstd): BatchNorm2d on y [+ resid] in ONE launch (coefficients derived inside; running statistics updated in train mode)."""
    _req(y, "y")
    n, c, h, w = y.shape
    for t, nme in ((gamma, "gamma"), (beta, "beta")):
        _req(t, nme)
    if resid is not None:
        _req(resid, "resid")
        if resid.shape != y.shape:
            raise RuntimeError("resid shape mismatch")
    if running_mean is not None:
        _req(running_mean, "running_mean")
        _req(running_var, "running_var")
    s, q = (sums if sums is not None else (None, None))
    z = torch.empty_like(y)
    mi = torch.empty((2, c), dtype=torch.float32, device=y.device)
    check(_lib.load().slu_bn_apply_fwd(y.data_ptr(), _ptr(s), _ptr(q), float(count), gamma.data_ptr(), beta.data_ptr(), float(eps), float(momentum),
                                       1 if train else 0, _ptr(running_mean), _ptr(running_var), _ptr(resid), z.data_ptr(), n, c, h * w,
                                       mi[0].data_ptr(), mi[1].data_ptr(), _stream()), "slu_bn_apply_fwd")
    if train and running_mean is not None:
        torch.autograd.graph.increment_version(running_mean)      # written through raw pointers (see bn_coeffs_fwd)
        torch.autograd.graph.increment_version(running_var)
    return z, mi[0], mi[1]


def bn_act_bwd(dz, y, s1=None, s2=None, count: float = 1.0, gamma=None, mean=None, invstd=None, train: bool = False, slope=None,
               want_dbias: bool = True):
    """(da, dbias f32 or None, dgamma, dbeta): the BatchNorm + LeakyReLU backward of a conv layer in ONE launch from the reduction sums s1 / s2
    (None: no BatchNorm), the bias gradient rounded to fp32 inside."""
    _req(dz, "dz")
    n, c, h, w = dz.shape
    has_bn = s1 is not None
    if y is not None:
        _req(y, "y")
        if y.shape != dz.shape:
            raise RuntimeError("y shape mismatch")
    da = torch.empty_like(dz)
    out = torch.empty((3, c), dtype=torch.float32, device=dz.device)            # dbias | dgamma | dbeta
    scratch = zeros_f64((2, c), dz.device) if want_dbias else None          # row 0: fp64 sums, row 1: the channels' ticket counters (uint32)
    check(_lib.load().slu_bn_act_bwd(dz.data_ptr(), _ptr(y), _ptr(s1), _ptr(s2), float(count), _ptr(gamma), _ptr(mean), _ptr(invstd),
                                     1 if has_bn else 0, 1 if train else 0, 0.0 if slope is None else float(slope), 0 if slope is None else 1,
                                     n, c, h * w, da.data_ptr(), None if scratch is None else scratch[0].data_ptr(),
                                     None if scratch is None else scratch[1].data_ptr(), out[0].data_ptr() if want_dbias else None,
                                     out[1].data_ptr(), out[2].data_ptr(), _stream()), "slu_bn_act_bwd")
    return da, (out[0] if want_dbias else None), (out[1] if has_bn else None), (out[2] if has_bn else None)


def act_affine_bwd(dz, y=None, k1=None, k2=None, k3=None, slope=None, want_dbias=True):
    """da = (k1*dz + k2 + k3*y) * leaky'(y);  dbias f64[C] = sum da."""
    _req(dz, "dz")
    n, c, h, w = dz.shape
    if y is not None:
        _req(y, "y")
        if y.shape != dz.shape:
            raise RuntimeError("y shape mismatch")
    for t, nme in ((k1, "k1"), (k2, "k2"), (k3, "k3")):
        if t is not None:
            _req(t, nme)
            if t.numel() != c:
                raise RuntimeError(f"{nme}: expected {c} elements")
    da = torch.empty_like(dz)
    db = zeros_f64((c,), dz.device) if want_dbias else None
    check(_lib.load().slu_act_affine_bwd(dz.data_ptr(), _ptr(y), _ptr(k1), _ptr(k2), _ptr(k3), 0.0 if slope is None else float(slope),
                                         0 if slope is None else 1, n, c, h * w, da.data_ptr(), _ptr(db), _stream()), "slu_act_affine_bwd")
    return da, db


def nchw_to_nhwc(x):
    _req(x, "x")
    n, c, h, w = x.shape
    cp = (c + 31) // 32 * 32
    out = torch.empty((n, h * w, cp), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_nchw_to_nhwc(x.data_ptr(), n, c, h * w, out.data_ptr(), _stream()), "slu_nchw_to_nhwc")
    return out


def gather_nhwc(srcs: Sequence[ConvSource]):
    arr = (_lib.ConvSrc * _lib.MAX_SRC)()
    n, h, w = _fill_srcs(arr, srcs)
    cin = sum(s.tensor.shape[1] // 4 if s.pixel_shuffle else s.tensor.shape[1] for s in srcs)
    cp = (cin + 31) // 32 * 32
    out = torch.empty((n, h * w, cp), dtype=torch.float32, device=srcs[0].tensor.device)
    check(_lib.load().slu_gather_nhwc(arr, len(srcs), n, h, w, out.data_ptr(), _stream()), "slu_gather_nhwc")
    return out


def split_grad(dcat, cbeg: int, src_shape, pixel_shuffle: bool, scale=None):
    _req(dcat, "dcat")
    n, ccat, h, w = dcat.shape
    sn, sc, sh, sw = src_shape
    if sn != n or (sh, sw) != ((h // 2, w // 2) if pixel_shuffle else (h, w)):
        raise RuntimeError("split_grad: source shape does not match the concatenated gradient")
    if scale is not None:
        _req(scale, "scale")
    out = torch.empty(tuple(src_shape), dtype=torch.float32, device=dcat.device)
    check(_lib.load().slu_split_grad(dcat.data_ptr(), n, ccat, int(cbeg), h, w, sc, 1 if pixel_shuffle else 0, _ptr(scale), out.data_ptr(),
                                     _stream()), "slu_split_grad")
    return out


def avgpool3s2_bwd(dy, scale, x_shape):
    _req(dy, "dy")
    n, c, h, w = x_shape
    if tuple(dy.shape) != (n, c, (h + 1) // 2, (w + 1) // 2):
        raise RuntimeError("avgpool3s2_bwd: dy shape mismatch")
    dx = torch.empty(tuple(x_shape), dtype=torch.float32, device=dy.device)
    check(_lib.load().slu_avgpool3s2_bwd(dy.data_ptr(), _ptr(scale), dx.data_ptr(), n, c, h, w, _stream()), "slu_avgpool3s2_bwd")
    return dx


def dgrad_weight(weight):
    """[Cout,Cin,k,k] -> [Cin,Cout,k,k] with taps mirrored: the weights of the data-gradient conv."""
    _req(weight, "weight")
    cout, cin, k, _ = weight.shape
    wd = torch.empty((cin, cout, k, k), dtype=torch.float32, device=weight.device)
    check(_lib.load().slu_dgrad_weight(weight.data_ptr(), cout, cin, k, wd.data_ptr(), _stream()), "slu_dgrad_weight")
    return wd


def conv2d_wgrad(da_t, in_t, n, h, w, cout, cin, ksize, dil, pad):
    """dW [cout,cin,k,k] from channel-last da_t [N,HW,Cop] and in_t [N,HW,Cip]."""
    _req(da_t, "da_t")
    _req(in_t, "in_t")
    cop, cip = (cout + 31) // 32 * 32, (cin + 31) // 32 * 32
    if tuple(da_t.shape) != (n, h * w, cop) or tuple(in_t.shape) != (n, h * w, cip):
        raise RuntimeError("conv2d_wgrad: operand shapes do not match")
    lib = _lib.load()
    scratch = torch.empty(lib.slu_wgrad_packed_floats(cout, cin, ksize), dtype=torch.float32, device=da_t.device)
    dw = torch.empty((cout, cin, ksize, ksize), dtype=torch.float32, device=da_t.device)
    check(lib.slu_conv2d_wgrad(da_t.data_ptr(), in_t.data_ptr(), n, h, w, cout, cin, ksize, dil, pad, scratch.data_ptr(), dw.data_ptr(),
                               _stream()), "slu_conv2d_wgrad")
    return dw


def conv2d_wgrad_nchw(da: torch.Tensor, srcs: Sequence[ConvSource], ksize: int, dil: int, pad: int):
    """dW [Cout, Cin, k, k] of a 3x3 (dil 1 / 2) or 2x2-dilated conv straight from NCHW da and its sources (PixelShuffle and multipliers
    included), or None when the shape is not covered (then: conv2d_wgrad on channel-last copies)."""
    _req(da, "da")
    n, cout, h, w = da.shape
    if (ksize, dil, pad) not in ((3, 1, 1), (3, 2, 2), (2, 2, 1)) or w % 16:
        return None
    if any(s.nbatch or s.cuse for s in srcs) or (h % 2 and any(s.pixel_shuffle for s in srcs)):
        return None
    arr = (_lib.ConvSrc * _lib.MAX_SRC)()
    if _fill_srcs(arr, srcs) != (n, h, w):
        raise RuntimeError("conv2d_wgrad_nchw: da and the sources disagree on (N, H, W)")
    cin = sum(s.tensor.shape[1] // 4 if s.pixel_shuffle else s.tensor.shape[1] for s in srcs)
    lib = _lib.load()
    scratch = _ZEROS32.take(lib.slu_wgrad_packed_floats(cout, cin, ksize), da.device)      # zero already: the launcher skips its fill
    dw = torch.empty((cout, cin, ksize, ksize), dtype=torch.float32, device=da.device)
    check(lib.slu_conv2d_wgrad_nchw(da.data_ptr(), arr, len(srcs), n, h, w, cout, ksize, dil, pad, scratch.data_ptr(), dw.data_ptr(), 1, _stream()),
          "slu_conv2d_wgrad_nchw")
    return dw


def conv1x1_wgrad_nchw(da: torch.Tensor, srcs: Sequence[ConvSource]):
    """dW [Cout, Cin, 1, 1] of a 1x1 conv straight from NCHW da and its plain sources, or None when the shape is not covered
    (then: conv2d_wgrad on channel-last copies)."""
    _req(da, "da")
    n, cout, h, w = da.shape
    if (h * w) % 32 or any(s.pixel_shuffle or s.scale is not None or s.nbatch or s.cuse for s in srcs):
        return None
    if any(s.tensor.shape[1] % 32 for s in srcs[:-1]) or any(tuple(s.tensor.shape[2:]) != (h, w) or s.tensor.shape[0] != n for s in srcs):
        return None
    arr = (_lib.ConvSrc * _lib.MAX_SRC)()
    _fill_srcs(arr, srcs)
    cin = sum(s.tensor.shape[1] for s in srcs)
    dw = _ZEROS32.take(cout * cin, da.device).view(cout, cin, 1, 1)                         # the kernel adds its partial sums into it
    check(_lib.load().slu_conv1x1_wgrad_nchw(da.data_ptr(), arr, len(srcs), n, h * w, cout, dw.data_ptr(), 1, _stream()), "slu_conv1x1_wgrad_nchw")
    return dw


# ------------------------------------------------------------------------------------------------
# ResNet-FPN data movement
# ------------------------------------------------------------------------------------------------
def maxpool3s2(x):
    _req(x, "x")
    n, c, h, w = x.shape
    y = torch.empty((n, c, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_maxpool3s2_fwd(x.data_ptr(), y.data_ptr(), n, c, h, w, _stream()), "slu_maxpool3s2_fwd")
    return y


def nearest_down(x, factor: int):
    _req(x, "x")
    n, c, h, w = x.shape
    if h % factor or w % factor:
        raise RuntimeError("nearest_down: H and W must be multiples of the factor")
    y = torch.empty((n, c, h // factor, w // factor), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_nearest_down(x.data_ptr(), y.data_ptr(), n, c, h, w, int(factor), _stream()), "slu_nearest_down")
    return y


def space_to_depth2(x):
    """[N,C,H,W] -> [N,4C,H/2,W/2], channel (2p+q)*C + c = x[c, 2y+p, 2x+q]."""
    _req(x, "x")
    n, c, h, w = x.shape
    if h % 2 or w % 2:
        raise RuntimeError("space_to_depth2: H and W must be even")
    y = torch.empty((n, 4 * c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_space_to_depth2(x.data_ptr(), y.data_ptr(), n, c, h, w, _stream()), "slu_space_to_depth2")
    return y


def space_to_depth2_cat(a, ca: int, b):
    """space_to_depth2 of cat(a[:, :ca], b) without materialising the concatenation."""
    _req(a, "a")
    _req(b, "b")
    n, ca_full, h, w = a.shape
    if b.shape[0] != n or tuple(b.shape[2:]) != (h, w) or not 0 < ca <= ca_full or h % 2 or w % 2:
        raise RuntimeError("space_to_depth2_cat: shape mismatch")
    cb = b.shape[1]
    y = torch.empty((n, 4 * (ca + cb), h // 2, w // 2), dtype=torch.float32, device=a.device)
    check(_lib.load().slu_space_to_depth2_cat(a.data_ptr(), ca_full, int(ca), b.data_ptr(), cb, y.data_ptr(), n, h, w, _stream()),
          "slu_space_to_depth2_cat")
    return y


def depth_to_space(x, r: int, elu_plus_one: bool = False, out: Optional[torch.Tensor] = None, c_off: int = 0):
    """nn.PixelShuffle(r), optionally followed by ELU(v) + 1.  With `out` [N,Ctot,H*r,W*r] the result is written into its
    channels [c_off, c_off + C/r^2) (several up-sampled maps sharing one concatenated buffer)."""
    _req(x, "x")
    n, c, h, w = x.shape
    if c % (r * r):
        raise RuntimeError("depth_to_space: C must be a multiple of r*r")
    cout = c // (r * r)
    if out is None:
        out = torch.empty((n, cout, h * r, w * r), dtype=torch.float32, device=x.device)
    else:
        _req(out, "out")
        if out.shape[0] != n or tuple(out.shape[2:]) != (h * r, w * r) or c_off < 0 or c_off + cout > out.shape[1]:
            raise RuntimeError("depth_to_space: `out` does not fit")
    check(_lib.load().slu_depth_to_space(x.data_ptr(), out.data_ptr(), n, cout, h, w, int(r), 1 if elu_plus_one else 0, int(c_off),
                                         out.shape[1], _stream()), "slu_depth_to_space")
    return out


def row_softmax_mul(score, value):
    """value * softmax(score, dim=-1); score [N,1,H,W], value [N,C,H,W]."""
    _req(score, "score")
    _req(value, "value")
    n, c, h, w = value.shape
    if tuple(score.shape) != (n, 1, h, w):
        raise RuntimeError("row_softmax_mul: score must be [N,1,H,W]")
    out = torch.empty_like(value)
    check(_lib.load().slu_row_softmax_mul(score.data_ptr(), value.data_ptr(), out.data_ptr(), n, c, h, w, _stream()), "slu_row_softmax_mul")
    return out


# ------------------------------------------------------------------------------------------------
# AUROC of error detection (metrics/auroc.py of the reference)
def bilinear_upsample(x: torch.Tensor, scale: int) -> torch.Tensor:
    """F.interpolate(x, scale_factor=scale, mode='bilinear', align_corners=False) on the device."""
    _req(x, "x")
    if x.dim() != 4 or int(scale) < 1:
        raise RuntimeError("bilinear_upsample: NCHW tensor and an integer scale >= 1 expected")
    n, c, h, w = x.shape
    y = torch.empty((n, c, h * int(scale), w * int(scale)), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_bilinear_upsample(x.data_ptr(), y.data_ptr(), n, c, h, w, int(scale), _stream()), "slu_bilinear_upsample")
    return y


def groupnorm(x: torch.Tensor, groups: int, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float = 1e-5, relu: bool = False,
              inplace: bool = False, return_stats: bool = False):
    """nn.GroupNorm(groups, C, eps)(x) [+ ReLU] for NCHW x."""
    _req(x, "x")
    if x.dim() != 4 or x.shape[1] % int(groups):
        raise RuntimeError(f"groupnorm: NCHW input with C divisible by groups={groups} expected, got {tuple(x.shape)}")
    n, c, h, w = x.shape
    for t, nme in ((gamma, "gamma"), (beta, "beta")):
        if t is not None:
            _req(t, nme)
            if t.numel() != c:
                raise RuntimeError(f"{nme}: expected {c} elements")
    stats = torch.empty((2, n * int(groups)), dtype=torch.float32, device=x.device)
    y = x if inplace else torch.empty_like(x)
    check(_lib.load().slu_groupnorm_fwd(x.data_ptr(), _ptr(gamma), _ptr(beta), n, c, h * w, int(groups), float(eps), 1 if relu else 0, stats[0].data_ptr(),
                                        stats[1].data_ptr(), y.data_ptr(), _stream()), "slu_groupnorm_fwd")
    return (y, stats) if return_stats else y


def groupnorm_stats(x: torch.Tensor, groups: int, eps: float = 1e-5) -> torch.Tensor:
    """[2, N * groups] (mean, rstd) of nn.GroupNorm(groups, C, eps) over NCHW x: the statistics launch of `groupnorm` alone."""
    _req(x, "x")
    if x.dim() != 4 or int(groups) < 1 or x.shape[1] % int(groups):
        raise RuntimeError(f"groupnorm_stats: NCHW input with C divisible by groups={groups} expected, got {tuple(x.shape)}")
    n, c, h, w = x.shape
    stats = torch.empty((2, n * int(groups)), dtype=torch.float32, device=x.device)
    args = (x.data_ptr(), n, c, h * w, int(groups), float(eps), stats[0].data_ptr(), stats[1].data_ptr(), _stream())
    if TIMING is None:
        check(_lib.load().slu_groupnorm_stats(*args), "slu_groupnorm_stats")
        return stats
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(_lib.load().slu_groupnorm_stats(*args), "slu_groupnorm_stats")
    e1.record()
    nbytes = 4.0 * n * c * h * w
    TIMING.append(("groupnorm_stats_kernel", 3.0 * n * c * h * w, nbytes, e0, e1, nbytes))
    TIMING_TAGS.append(f"N{n} GroupNorm({groups}, {c}) statistics {h}x{w}")
    return stats


def head_mc_f32(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], passes: int, batch: int, eps: float = 1e-12,
                gn_stats: Optional[torch.Tensor] = None, gn_groups: int = 0, gn_gamma: Optional[torch.Tensor] = None,
                gn_beta: Optional[torch.Tensor] = None, relu: bool = False):
    """x fp32 [T*B, Cin, H, W] (pass-major) -> (p_bar [B,C,H,W], H_norm [B,H,W], MI_norm [B,H,W], preds int64 [B,H,W]): GroupNorm apply
    (gn_stats = groupnorm_stats(x, gn_groups); None: x is used as it is) [+ ReLU], the 1x1 head `weight` [C, Cin(, 1, 1)] + bias and the
    MC-dropout reduction of trainer.py:1143-1154 in one launch (slu_head_mc_f32); neither the normalised tensor nor logits are written."""
    _req(x, "x")
    if x.dim() != 4:
        raise RuntimeError(f"head_mc_f32: expected [T*B, Cin, H, W], got {tuple(x.shape)}")
    n, cin, h, w = x.shape
    passes, batch = int(passes), int(batch)
    if passes < 1 or batch < 1 or n != passes * batch:
        raise RuntimeError(f"head_mc_f32: {n} images != T * B = {passes} * {batch}")
    _req(weight, "weight")
    if weight.dim() not in (2, 4) or weight.shape[1] != cin or weight.numel() != weight.shape[0] * cin:
        raise RuntimeError(f"weight: expected [C, {cin}] or [C, {cin}, 1, 1], got {tuple(weight.shape)}")
    classes = weight.shape[0]
    if not 1 <= classes <= 32 or cin > 128:
        raise RuntimeError(f"head_mc_f32: covers 1..32 classes and up to 128 input channels, got {classes} and {cin}")
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != classes:
            raise RuntimeError(f"bias: expected {classes} elements, got {bias.numel()}")
    mean = rstd = None
    groups = 0
    if gn_stats is not None:
        groups = int(gn_groups)
        if groups < 1 or cin % groups:
            raise RuntimeError(f"head_mc_f32: gn_groups={gn_groups} must divide Cin={cin}")
        _req(gn_stats, "gn_stats")
        if tuple(gn_stats.shape) != (2, n * groups):
            raise RuntimeError(f"gn_stats: expected {(2, n * groups)}, got {tuple(gn_stats.shape)}")
        mean, rstd = gn_stats[0], gn_stats[1]
        for t, nme in ((gn_gamma, "gn_gamma"), (gn_beta, "gn_beta")):
            if t is not None:
                _req(t, nme)
                if t.numel() != cin:
                    raise RuntimeError(f"{nme}: expected {cin} elements")
    elif gn_gamma is not None or gn_beta is not None:
        raise RuntimeError("head_mc_f32: gn_gamma / gn_beta need gn_stats")
    dev = x.device
    p_bar = torch.empty((batch, classes, h, w), dtype=torch.float32, device=dev)
    hn = torch.empty((batch, h, w), dtype=torch.float32, device=dev)
    mi = torch.empty((batch, h, w), dtype=torch.float32, device=dev)
    preds = torch.empty((batch, h, w), dtype=torch.int64, device=dev)
    head_mc_f32_out(x, weight, bias, passes, batch, eps, mean, rstd, groups, gn_gamma if mean is not None else None,
                    gn_beta if mean is not None else None, relu, p_bar, hn, mi, preds)
    return p_bar, hn, mi, preds


def head_mc_f32_out(x, weight, bias, passes, batch, eps, mean, rstd, groups, gamma, beta, relu, p_bar, hn, mi, preds) -> None:
    """The launch of `head_mc_f32` into caller-owned outputs (shapes as `head_mc_f32` returns them; checked here)."""
    n, cin, h, w = x.shape
    classes = weight.shape[0]
    for t, nme, shape, dt in ((p_bar, "p_bar", (batch, classes, h, w), torch.float32), (hn, "h_norm", (batch, h, w), torch.float32),
                              (mi, "mi_norm", (batch, h, w), torch.float32), (preds, "preds", (batch, h, w), torch.int64)):
        _req(t, nme, dt)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{nme}: expected {shape}, got {tuple(t.shape)}")
    lib = _lib.load()
    args = (x.data_ptr(), passes, batch, cin, h * w, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), int(groups), 1 if relu else 0,
            weight.data_ptr(), _ptr(bias), classes, float(eps), p_bar.data_ptr(), hn.data_ptr(), mi.data_ptr(), preds.data_ptr(), _stream())
    if TIMING is None:
        check(lib.slu_head_mc_f32(*args), "slu_head_mc_f32")
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.slu_head_mc_f32(*args), "slu_head_mc_f32")
    e1.record()
    px = float(n * h * w)
    flops = 2.0 * cin * classes * px
    # layer-granular accounting of what it replaces: GroupNorm apply (read + write), the head conv (read, write logits), the reduction (read them)
    nbytes = px * 4.0 * (3 * cin + 2 * classes) + batch * h * w * (4.0 * classes + 16.0)
    # what the fused kernel must move: the conv output of every pass in, p_bar / H / MI / argmax of every scan out
    min_bytes = px * 4.0 * cin + batch * h * w * (4.0 * classes + 16.0) + 4.0 * classes * cin
    TIMING.append((f"head_mc_f32_kernel<{(classes + 7) // 8}>", flops, nbytes, e0, e1, min_bytes))
    TIMING_TAGS.append(f"N{n} {cin}->{classes} GroupNorm apply + 1x1 head + MC reduce T={passes} {h}x{w}")


def spatial_softmax_gate(x: torch.Tensor, score: torch.Tensor, return_stats: bool = False):
    """x * softmax(score over H*W) + x  (SpatialAttention of semanticFCN_opt): x [N,C,H,W], score [N,1,H,W]."""
    _req(x, "x")
    _req(score, "score")
    if x.dim() != 4 or tuple(score.shape) != (x.shape[0], 1, x.shape[2], x.shape[3]):
        raise RuntimeError(f"spatial_softmax_gate: x [N,C,H,W] / score [N,1,H,W] expected, got {tuple(x.shape)} / {tuple(score.shape)}")
    n, c, h, w = x.shape
    stats = torch.empty(2 * n, dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    check(_lib.load().slu_spatial_softmax_gate(x.data_ptr(), score.data_ptr(), stats.data_ptr(), out.data_ptr(), n, c, h * w, _stream()),
          "slu_spatial_softmax_gate")
    return (out, stats) if return_stats else out


# ------------------------------------------------------------------------------------------------
# training path of the FPN models (csrc/fpn_train.hip): forward / backward pieces of the autograd nodes in fpn_autograd.py
# ------------------------------------------------------------------------------------------------
POINTWISE_OPS = {"leaky": 0, "tanh": 1, "elu+1": 2, "silu": 3}


def pointwise_fwd(x: torch.Tensor, op: str, slope: float = 0.0) -> torch.Tensor:
    """LeakyReLU(slope) (0 = ReLU) / tanh / ELU + 1 / SiLU, elementwise."""
    _req(x, "x")
    y = torch.empty_like(x)
    if x.numel():
        check(_lib.load().slu_pointwise_fwd(x.data_ptr(), y.data_ptr(), x.numel(), POINTWISE_OPS[op], float(slope), _stream()), "slu_pointwise_fwd")
    return y


def pointwise_bwd(dy: torch.Tensor, y: torch.Tensor, op: str, slope: float = 0.0) -> torch.Tensor:
    """dx = dy * f'(x), from the forward's output y (op 'silu': from the forward's INPUT, passed as `y`)."""
    _req(dy, "dy")
    _req(y, "y")
    if dy.shape != y.shape:
        raise RuntimeError("pointwise_bwd: shape mismatch")
    dx = torch.empty_like(dy)
    if dy.numel():
        check(_lib.load().slu_pointwise_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), dy.numel(), POINTWISE_OPS[op], float(slope), _stream()),
              "slu_pointwise_bwd")
    return dx


def maxpool3s2_bwd(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    _req(x, "x")
    _req(dy, "dy")
    n, c, h, w = x.shape
    if tuple(dy.shape) != (n, c, (h + 1) // 2, (w + 1) // 2):
        raise RuntimeError("maxpool3s2_bwd: dy does not match the pooled shape")
    dx = torch.empty_like(x)
    check(_lib.load().slu_maxpool3s2_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, c, h, w, _stream()), "slu_maxpool3s2_bwd")
    return dx


def nearest_down_bwd(dy: torch.Tensor, factor: int) -> torch.Tensor:
    _req(dy, "dy")
    n, c, oh, ow = dy.shape
    dx = torch.empty((n, c, oh * int(factor), ow * int(factor)), dtype=torch.float32, device=dy.device)
    check(_lib.load().slu_nearest_down_bwd(dy.data_ptr(), dx.data_ptr(), n, c, oh * int(factor), ow * int(factor), int(factor), _stream()),
          "slu_nearest_down_bwd")
    return dx


def replace_tail(x: torch.Tensor, meta: torch.Tensor) -> torch.Tensor:
    """cat(x[:, :C-m], meta) with m = meta.shape[1]."""
    _req(x, "x")
    _req(meta, "meta")
    n, c, h, w = x.shape
    m = meta.shape[1]
    if tuple(meta.shape) != (n, m, h, w) or not 0 < m <= c:
        raise RuntimeError(f"replace_tail: x {tuple(x.shape)} / meta {tuple(meta.shape)}")
    out = torch.empty_like(x)
    check(_lib.load().slu_replace_tail_fwd(x.data_ptr(), meta.data_ptr(), out.data_ptr(), n, c, m, h, w, _stream()), "slu_replace_tail_fwd")
    return out


def replace_tail_bwd(dout: torch.Tensor, m: int, want_dx: bool = True, want_dmeta: bool = True):
    _req(dout, "dout")
    n, c, h, w = dout.shape
    dx = torch.empty_like(dout) if want_dx else None
    dmeta = torch.empty((n, m, h, w), dtype=torch.float32, device=dout.device) if want_dmeta else None
    if want_dx or want_dmeta:
        check(_lib.load().slu_replace_tail_bwd(dout.data_ptr(), _ptr(dx), _ptr(dmeta), n, c, int(m), h, w, _stream()), "slu_replace_tail_bwd")
    return dx, dmeta


def row_softmax_mul_bwd(score, value, dout, want_dscore: bool = True, want_dvalue: bool = True):
    _req(score, "score")
    _req(value, "value")
    _req(dout, "dout")
    n, c, h, w = value.shape
    if tuple(score.shape) != (n, 1, h, w) or dout.shape != value.shape:
        raise RuntimeError("row_softmax_mul_bwd: shape mismatch")
    dscore = torch.empty_like(score) if want_dscore else None
    dvalue = torch.empty_like(value) if want_dvalue else None
    if want_dscore or want_dvalue:
        check(_lib.load().slu_row_softmax_mul_bwd(score.data_ptr(), value.data_ptr(), dout.data_ptr(), _ptr(dscore), _ptr(dvalue), n, c, h, w, _stream()),
              "slu_row_softmax_mul_bwd")
    return dscore, dvalue


def depth_to_space_bwd(dy: torch.Tensor, cout: int, r: int, c_off: int = 0) -> torch.Tensor:
    """Gradient of depth_to_space w.r.t. its input from the channel slice [c_off, c_off + cout) of dy [N,Ctot,H*r,W*r]."""
    _req(dy, "dy")
    n, ctot, oh, ow = dy.shape
    if oh % r or ow % r or c_off < 0 or c_off + cout > ctot:
        raise RuntimeError("depth_to_space_bwd: shape mismatch")
    dx = torch.empty((n, cout * r * r, oh // r, ow // r), dtype=torch.float32, device=dy.device)
    check(_lib.load().slu_depth_to_space_bwd(dy.data_ptr(), dx.data_ptr(), n, int(cout), oh // r, ow // r, int(r), int(c_off), ctot, _stream()),
          "slu_depth_to_space_bwd")
    return dx


def bilinear_upsample_bwd(dy: torch.Tensor, scale: int) -> torch.Tensor:
    _req(dy, "dy")
    n, c, oh, ow = dy.shape
    if oh % scale or ow % scale:
        raise RuntimeError("bilinear_upsample_bwd: shape mismatch")
    dx = torch.empty((n, c, oh // scale, ow // scale), dtype=torch.float32, device=dy.device)
    check(_lib.load().slu_bilinear_upsample_bwd(dy.data_ptr(), dx.data_ptr(), n, c, oh // scale, ow // scale, int(scale), _stream()),
          "slu_bilinear_upsample_bwd")
    return dx


def groupnorm_bwd(x, y, dy, gamma, stats, groups: int, relu: bool, want_affine: bool = True):
    """(dx, dgamma f64[C] | None, dbeta f64[C] | None); stats = the [2, N*groups] (mean, rstd) tensor of groupnorm(return_stats=True)."""
    _req(x, "x")
    _req(dy, "dy")
    n, c, h, w = x.shape
    dx = torch.empty_like(x)
    dg = zeros_f64((c,), x.device) if want_affine else None
    db = zeros_f64((c,), x.device) if want_affine else None
    check(_lib.load().slu_groupnorm_bwd(x.data_ptr(), _ptr(y), dy.data_ptr(), _ptr(gamma), stats[0].data_ptr(), stats[1].data_ptr(), dx.data_ptr(),
                                        _ptr(dg), _ptr(db), n, c, h * w, int(groups), 1 if relu else 0, _stream()), "slu_groupnorm_bwd")
    return dx, dg, db


def spatial_softmax_gate_bwd(x, score, stats, dout):
    _req(x, "x")
    _req(score, "score")
    _req(dout, "dout")
    n, c, h, w = x.shape
    dx, dscore = torch.empty_like(x), torch.empty_like(score)
    ws = torch.empty((n, h * w), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_spatial_softmax_gate_bwd(x.data_ptr(), score.data_ptr(), stats.data_ptr(), dout.data_ptr(), dx.data_ptr(), dscore.data_ptr(),
                                                   ws.data_ptr(), n, c, h * w, _stream()), "slu_spatial_softmax_gate_bwd")
    return dx, dscore


# ------------------------------------------------------------------------------------------------
AUROC_MODES = {"alpha": 0, "logits": 1, "probs": 2}
AUROC_SCORES = {"entropy": 0, "entropy_norm": 1, "mi": 2, "mi_norm": 3, "1-maxprob": 4}


def auroc_scores(preds: torch.Tensor, labels: torch.Tensor, mode: str, score: str, ignore_index=None, eps: float = 1e-12,
                 score_override: Optional[torch.Tensor] = None):
    """(score[B,H,W] fp32, flag[B,H,W] uint8: 0 correct / 1 error / 2 ignored) -- slu_auroc_scores."""
    _req(preds, "preds")
    _req(labels, "labels", torch.int64)
    if preds.dim() != 4 or tuple(labels.shape) != (preds.shape[0], preds.shape[2], preds.shape[3]):
        raise RuntimeError(f"auroc_scores: preds [B,C,H,W] / labels [B,H,W] expected, got {tuple(preds.shape)} / {tuple(labels.shape)}")
    if mode not in AUROC_MODES or score not in AUROC_SCORES:
        raise ValueError(f"auroc_scores: unknown mode {mode!r} or score {score!r}")
    b, c, h, w = preds.shape
    if score_override is not None:
        _req(score_override, "score_override")
        if tuple(score_override.shape) != (b, h, w):
            raise RuntimeError(f"score_override: expected {(b, h, w)}, got {tuple(score_override.shape)}")
    s = torch.empty((b, h, w), dtype=torch.float32, device=preds.device)
    f = torch.empty((b, h, w), dtype=torch.uint8, device=preds.device)
    check(_lib.load().slu_auroc_scores(preds.data_ptr(), labels.data_ptr(), _ptr(score_override), b, c, h * w, AUROC_MODES[mode], AUROC_SCORES[score],
                                       0 if ignore_index is None else 1, 0 if ignore_index is None else int(ignore_index), float(eps),
                                       s.data_ptr(), f.data_ptr(), _stream()), "slu_auroc_scores")
    return s, f


def auroc_from_samples(scores: torch.Tensor, is_error: torch.Tensor, want_sorted: bool = False):
    """AUROC of 1-D device samples (score fp32, is_error uint8 in {0,1}) -> (auroc, P, N[, sorted_scores, sorted_is_error])."""
    _req(scores, "scores")
    _req(is_error, "is_error", torch.uint8)
    if scores.dim() != 1 or scores.shape != is_error.shape or scores.numel() == 0:
        raise RuntimeError("auroc_from_samples: two equally long, non-empty 1-D tensors expected")
    lib = _lib.load()
    n = scores.numel()
    ws = torch.empty(lib.slu_auroc_workspace_bytes(n), dtype=torch.uint8, device=scores.device)
    out = torch.empty(3, dtype=torch.float64, device=scores.device)
    ss = torch.empty_like(scores) if want_sorted else None
    se = torch.empty_like(is_error) if want_sorted else None
    check(lib.slu_auroc_compute(scores.data_ptr(), is_error.data_ptr(), n, ws.data_ptr(), ws.numel(), out.data_ptr(), _ptr(ss), _ptr(se), _stream()),
          "slu_auroc_compute")
    a, p, nn_ = (float(v) for v in out.cpu())
    return (a, int(p), int(nn_), ss, se) if want_sorted else (a, int(p), int(nn_))


# ------------------------------------------------------------------------------------------------
# AURC / E-AURC of selective prediction (metrics/aurc.py of the reference)
# ------------------------------------------------------------------------------------------------
AURC_KS = (1, 2, 5, 10, 20, 30, 40, 50)
AURC_MAX_KS = 16


class AurcResult(NamedTuple):
    aurc: float
    eaurc: float
    aurc_opt: float
    num_errors: int                               # E
    num_points: int                               # m: curve points after point 0, before the tail
    last_start: int                               # s_m (-1 when m == 0)
    recalls: "list[float]"                        # e_{m_k - 1} / max(E, 1) per entry of ks
    coverages: Optional[torch.Tensor] = None      # fp64 [m + 1] on the device (want_curve): points 0..m, the tail is the caller's
    rc_risks: Optional[torch.Tensor] = None
    sorted_confids: Optional[torch.Tensor] = None     # ascending, stable (want_sorted)
    sorted_is_error: Optional[torch.Tensor] = None


def aurc_samples(probs: torch.Tensor, labels: torch.Tensor, ignore_index: int, ent_mc: Optional[torch.Tensor] = None,
                 use_max_prob_confidence: bool = False):
    """(conf[B,H,W] fp32, flag[B,H,W] uint8: 0 correct / 1 error / 2 ignored) -- slu_aurc_samples."""
    _req(probs, "probs")
    _req(labels, "labels", torch.int64)
    if probs.dim() != 4 or tuple(labels.shape) != (probs.shape[0], probs.shape[2], probs.shape[3]) or probs.numel() == 0:
        raise RuntimeError(f"aurc_samples: probs [B,C,H,W] / labels [B,H,W] expected, got {tuple(probs.shape)} / {tuple(labels.shape)}")
    b, c, h, w = probs.shape
    if ent_mc is not None:
        _req(ent_mc, "ent_mc")
        if tuple(ent_mc.shape) != (b, h, w):
            raise RuntimeError(f"ent_mc: expected {(b, h, w)}, got {tuple(ent_mc.shape)}")
    conf = torch.empty((b, h, w), dtype=torch.float32, device=probs.device)
    flag = torch.empty((b, h, w), dtype=torch.uint8, device=probs.device)
    check(_lib.load().slu_aurc_samples(probs.data_ptr(), labels.data_ptr(), _ptr(ent_mc), b, c, h * w, int(ignore_index),
                                       1 if use_max_prob_confidence else 0, conf.data_ptr(), flag.data_ptr(), _stream()), "slu_aurc_samples")
    return conf, flag


def aurc_from_samples(confids: torch.Tensor, is_error: torch.Tensor, ks: Sequence[float] = AURC_KS, want_curve: bool = False,
                      want_sorted: bool = False) -> AurcResult:
    """AURC / E-AURC / top-k% error recall of 1-D device samples (conf fp32, is_error uint8 in {0,1}) -- slu_aurc_compute."""
    _req(confids, "confids")
    _req(is_error, "is_error", torch.uint8)
    if confids.dim() != 1 or confids.shape != is_error.shape or confids.numel() == 0:
        raise RuntimeError("aurc_from_samples: two equally long, non-empty 1-D tensors expected")
    ks = [float(k) for k in ks]
    if len(ks) > AURC_MAX_KS or any(not k >= 0.0 for k in ks):
        raise RuntimeError(f"aurc_from_samples: at most {AURC_MAX_KS} non-negative percentages expected, got {ks}")
    lib = _lib.load()
    n, dev = confids.numel(), confids.device
    ws = torch.empty(lib.slu_aurc_workspace_bytes(n), dtype=torch.uint8, device=dev)
    out = torch.empty(6 + len(ks), dtype=torch.float64, device=dev)            # out6, then the recalls
    cov = torch.empty(n, dtype=torch.float64, device=dev) if want_curve else None
    risk = torch.empty(n, dtype=torch.float64, device=dev) if want_curve else None
    ss = torch.empty_like(confids) if want_sorted else None
    se = torch.empty_like(is_error) if want_sorted else None
    ks_host = (C.c_double * max(len(ks), 1))(*ks)
    check(lib.slu_aurc_compute(confids.data_ptr(), is_error.data_ptr(), n, ws.data_ptr(), ws.numel(), C.addressof(ks_host), len(ks), out.data_ptr(),
                               out.data_ptr() + 6 * 8, _ptr(cov), _ptr(risk), _ptr(ss), _ptr(se), _stream()), "slu_aurc_compute")
    host = out.cpu().tolist()
    m = int(host[4])
    return AurcResult(host[0], host[1], host[2], int(host[3]), m, int(host[5]), host[6:],
                      cov[:m + 1] if want_curve else None, risk[:m + 1] if want_curve else None, ss, se)


# ------------------------------------------------------------------------------------------------
# accuracy vs uncertainty bins (models/evaluator.py UncertaintyAccuracyAggregator)
# ------------------------------------------------------------------------------------------------
def ua_samples(labels: torch.Tensor, preds: torch.Tensor, uncertainty: torch.Tensor, ignore_ids=()):
    """(u fp32 [n] clamped to [0,1], flag uint8 [n]: 1 correct / 0 wrong / 2 label in ignore_ids), flattened scan order."""
    _req(labels, "labels", torch.int64)
    _req(preds, "preds", torch.int64)
    _req(uncertainty, "uncertainty")
    if not (labels.shape == preds.shape == uncertainty.shape) or labels.numel() == 0:
        raise RuntimeError("ua_samples: labels, preds and uncertainty must have the same non-empty shape")
    n = labels.numel()
    ids = torch.tensor(list(ignore_ids), dtype=torch.int64, device=labels.device) if len(ignore_ids) else None
    u = torch.empty(n, dtype=torch.float32, device=labels.device)
    f = torch.empty(n, dtype=torch.uint8, device=labels.device)
    check(_lib.load().slu_ua_samples(labels.data_ptr(), preds.data_ptr(), uncertainty.data_ptr(), n, _ptr(ids), 0 if ids is None else ids.numel(),
                                     u.data_ptr(), f.data_ptr(), _stream()), "slu_ua_samples")
    return u, f


def binned_counts(u: torch.Tensor, correct: torch.Tensor, edges: torch.Tensor):
    """np.histogram(u, bins=edges) and the histogram of the correct ones, on the device: (count int64 [K], n_correct int64 [K])."""
    _req(u, "u")
    _req(correct, "correct", torch.uint8)
    _req(edges, "edges")
    if u.dim() != 1 or u.shape != correct.shape or u.numel() == 0 or edges.dim() != 1 or not 2 <= edges.numel() <= 257:
        raise RuntimeError("binned_counts: 1-D samples and 2..257 edges expected")
    k = edges.numel() - 1
    cnt = torch.zeros(k, dtype=torch.int64, device=u.device)
    ok = torch.zeros(k, dtype=torch.int64, device=u.device)
    check(_lib.load().slu_binned_counts(u.data_ptr(), correct.data_ptr(), u.numel(), edges.data_ptr(), k, cnt.data_ptr(), ok.data_ptr(), _stream()),
          "slu_binned_counts")
    return cnt, ok


def ece_samples(preds: torch.Tensor, labels: torch.Tensor, mode: str, ignore_index=None, eps: float = 1e-12):
    """(conf fp32 [B,H,W] in [0,1], flag uint8 [B,H,W]: 1 correct / 0 wrong / 2 ignored) -- slu_ece_samples (metrics/ece.py:55-84)."""
    _req(preds, "preds")
    _req(labels, "labels", torch.int64)
    if preds.dim() != 4 or tuple(labels.shape) != (preds.shape[0], preds.shape[2], preds.shape[3]):
        raise RuntimeError(f"ece_samples: preds [B,C,H,W] / labels [B,H,W] expected, got {tuple(preds.shape)} / {tuple(labels.shape)}")
    if mode not in AUROC_MODES:
        raise ValueError(f"ece_samples: unknown mode {mode!r}")
    b, c, h, w = preds.shape
    conf = torch.empty((b, h, w), dtype=torch.float32, device=preds.device)
    flag = torch.empty((b, h, w), dtype=torch.uint8, device=preds.device)
    check(_lib.load().slu_ece_samples(preds.data_ptr(), labels.data_ptr(), b, c, h * w, AUROC_MODES[mode], 0 if ignore_index is None else 1,
                                      0 if ignore_index is None else int(ignore_index), float(eps), conf.data_ptr(), flag.data_ptr(), _stream()),
          "slu_ece_samples")
    return conf, flag


def binned_stats(u: torch.Tensor, correct: torch.Tensor, edges: torch.Tensor):
    """The three np.histogram calls of metrics/ece.py:136-140 on the device: (count int64 [K], n_correct int64 [K], sum_u float64 [K])."""
    _req(u, "u")
    _req(correct, "correct", torch.uint8)
    _req(edges, "edges")
    if u.dim() != 1 or u.shape != correct.shape or u.numel() == 0 or edges.dim() != 1 or not 2 <= edges.numel() <= 257:
        raise RuntimeError("binned_stats: 1-D samples and 2..257 edges expected")
    k = edges.numel() - 1
    cnt = torch.zeros(k, dtype=torch.int64, device=u.device)
    ok = torch.zeros(k, dtype=torch.int64, device=u.device)
    su = torch.zeros(k, dtype=torch.float64, device=u.device)
    check(_lib.load().slu_binned_stats(u.data_ptr(), correct.data_ptr(), u.numel(), edges.data_ptr(), k, cnt.data_ptr(), ok.data_ptr(), su.data_ptr(),
                                       _stream()), "slu_binned_stats")
    return cnt, ok, su


# ------------------------------------------------------------------------------------------------
# Tversky loss (models/losses.py TverskyLoss)
# ------------------------------------------------------------------------------------------------
TVERSKY_ACTS = {"logits": 0, "probs": 1, "log_probs": 2}
TVERSKY_REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}


def tversky_fwd(x: torch.Tensor, labels: torch.Tensor, model_act: str, ignore_index, alpha: float, beta: float, smooth: float, reduction: str):
    """-> (loss [1] or [C], coef [2,C] for the backward, any_valid [1]) -- slu_tversky_fwd."""
    _req(x, "outputs")
    _req(labels, "labels", torch.int64)
    if x.dim() != 4 or tuple(labels.shape) != (x.shape[0], x.shape[2], x.shape[3]):
        raise RuntimeError(f"tversky: outputs [B,C,H,W] / labels [B,H,W] expected, got {tuple(x.shape)} / {tuple(labels.shape)}")
    b, c, h, w = x.shape
    red = TVERSKY_REDUCTIONS[reduction]
    sums = torch.empty(3 * c, dtype=torch.float64, device=x.device)
    coef = torch.empty((2, c), dtype=torch.float32, device=x.device)
    loss = torch.empty(c if red == 2 else 1, dtype=torch.float32, device=x.device)
    anyv = torch.empty(1, dtype=torch.float32, device=x.device)
    check(_lib.load().slu_tversky_fwd(x.data_ptr(), labels.data_ptr(), b, c, h * w, TVERSKY_ACTS[model_act], 0 if ignore_index is None else 1,
                                      0 if ignore_index is None else int(ignore_index), float(alpha), float(beta), float(smooth), red,
                                      sums.data_ptr(), coef.data_ptr(), loss.data_ptr(), anyv.data_ptr(), _stream()), "slu_tversky_fwd")
    return loss, coef, anyv


def tversky_bwd(x: torch.Tensor, labels: torch.Tensor, model_act: str, ignore_index, alpha: float, beta: float, coef: torch.Tensor,
                grad_out: torch.Tensor):
    _req(x, "outputs")
    _req(labels, "labels", torch.int64)
    _req(coef, "coef")
    _req(grad_out, "grad_out")
    b, c, h, w = x.shape
    if grad_out.numel() not in (1, c):
        raise RuntimeError("tversky_bwd: grad_out must have 1 or C elements")
    gx = torch.empty_like(x)
    check(_lib.load().slu_tversky_bwd(x.data_ptr(), labels.data_ptr(), b, c, h * w, TVERSKY_ACTS[model_act], 0 if ignore_index is None else 1,
                                      0 if ignore_index is None else int(ignore_index), float(alpha), float(beta), coef.data_ptr(),
                                      grad_out.data_ptr(), 1 if (grad_out.numel() == c and c > 1) else 0, gx.data_ptr(), _stream()), "slu_tversky_bwd")
    return gx


# ------------------------------------------------------------------------------------------------
# per-pixel Dirichlet losses (losses/dirichlet_losses.py, losses/regularizers.py)
# ------------------------------------------------------------------------------------------------
DIRICHLET_LOSS_KINDS = {"nll_dircat": 0, "digamma_ce": 1, "brier": 2, "mse": 3, "kl_off_uniform": 4, "complement_kl": 5, "wrong_low_evidence": 6,
                        "kl_off_uniform_weighted": 7}


def _dirichlet_loss_args(alpha, labels):
    _req(alpha, "alpha")
    _req(labels, "labels", torch.int64)
    if alpha.dim() != 4 or tuple(labels.shape) != (alpha.shape[0], alpha.shape[2], alpha.shape[3]):
        raise RuntimeError(f"dirichlet loss: alpha [B,C,H,W] / labels [B,H,W] expected, got {tuple(alpha.shape)} / {tuple(labels.shape)}")
    return alpha.shape


def dirichlet_loss_fwd(alpha: torch.Tensor, labels: torch.Tensor, kind: str, param: float, eps: float, ignore_index):
    """-> (sum float64 [1], count int64 [1]) over the valid pixels."""
    b, c, h, w = _dirichlet_loss_args(alpha, labels)
    s = torch.empty(1, dtype=torch.float64, device=alpha.device)
    n = torch.empty(1, dtype=torch.int64, device=alpha.device)
    check(_lib.load().slu_dirichlet_loss_fwd(alpha.data_ptr(), labels.data_ptr(), b, c, h * w, DIRICHLET_LOSS_KINDS[kind], float(param), float(eps),
                                             0 if ignore_index is None else 1, 0 if ignore_index is None else int(ignore_index), s.data_ptr(),
                                             n.data_ptr(), _stream()), "slu_dirichlet_loss_fwd")
    return s, n


def dirichlet_loss_bwd(alpha: torch.Tensor, labels: torch.Tensor, kind: str, param: float, eps: float, ignore_index, gscale: torch.Tensor):
    b, c, h, w = _dirichlet_loss_args(alpha, labels)
    _req(gscale, "gscale")
    g = torch.empty_like(alpha)
    check(_lib.load().slu_dirichlet_loss_bwd(alpha.data_ptr(), labels.data_ptr(), b, c, h * w, DIRICHLET_LOSS_KINDS[kind], float(param), float(eps),
                                             0 if ignore_index is None else 1, 0 if ignore_index is None else int(ignore_index),
                                             gscale.data_ptr(), g.data_ptr(), _stream()), "slu_dirichlet_loss_bwd")
    return g


def build_normals(xyz: torch.Tensor, norm_factor: float = 0.25):
    """xyz fp32 [H, W, C >= 3] on the GPU -> unit normals fp32 [H, W, 3] (Scharr derivatives, cross product, normalisation)."""
    _req(xyz, "xyz")
    if xyz.dim() != 3 or xyz.shape[2] < 3:
        raise RuntimeError(f"xyz: expected [H, W, C >= 3], got {tuple(xyz.shape)}")
    h, w, c = xyz.shape
    out = torch.empty((h, w, 3), dtype=torch.float32, device=xyz.device)
    check(_lib.load().slu_build_normals(xyz.data_ptr(), h, w, c, float(norm_factor), out.data_ptr(), _stream()), "slu_build_normals")
    return out


def group_by_class(labels: torch.Tensor, values: torch.Tensor, num_classes: int):
    """labels int64 [n], values fp32 [n] (device) -> (grouped fp32 [n]: class 0's samples, then class 1's, ... in scan order; the first
    counts.sum() entries are meaningful), counts int64 [C] (device)."""
    _req(labels, "labels", torch.int64)
    _req(values, "values")
    if labels.dim() != 1 or labels.shape != values.shape or labels.numel() == 0:
        raise RuntimeError(f"group_by_class: equally long non-empty 1-D labels / values expected, got {tuple(labels.shape)} / {tuple(values.shape)}")
    n = labels.numel()
    lib = _lib.load()
    ws = torch.empty(lib.slu_group_by_class_workspace_bytes(n), dtype=torch.uint8, device=labels.device)
    out = torch.empty(n, dtype=torch.float32, device=labels.device)
    counts = torch.empty(int(num_classes), dtype=torch.int64, device=labels.device)
    check(lib.slu_group_by_class(labels.data_ptr(), values.data_ptr(), n, int(num_classes), out.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                 ws.numel(), _stream()), "slu_group_by_class")
    return out, counts


# ------------------------------------------------------------------------------------------------
# temperature scaling (models/temp_scaling.py): the calibration cache and the fused NLL(T) closure
# ------------------------------------------------------------------------------------------------
CALIB_KINDS = {"logits": 0, "probs": 1, "log_probs": 2}


def calib_rows(out: torch.Tensor, kind: str, labels: torch.Tensor, ignore_index, rows: torch.Tensor, row_labels: torch.Tensor, count: torch.Tensor):
    """Append the log-probability rows of the pixels with label != ignore_index (all when None), in (b, h, w) order, to the cache
    `rows` fp32 [cap, C] / `row_labels` int64 [cap] at row count[0] (int64 [1] on the device, advanced by the launch; rows past cap are
    dropped and count[0] > cap tells).  out fp32 [B,C,H,W] of `kind` 'logits' | 'probs' | 'log_probs', labels int64 [B,H,W].  No host
    synchronisation."""
    _req(out, "out")
    _req(labels, "labels", torch.int64)
    _req(rows, "rows")
    _req(row_labels, "row_labels", torch.int64)
    _req(count, "count", torch.int64)
    if kind not in CALIB_KINDS:
        raise ValueError(f"Unknown output kind: {kind}")
    if out.dim() != 4 or tuple(labels.shape) != (out.shape[0], out.shape[2], out.shape[3]) or out.numel() == 0:
        raise RuntimeError(f"calib_rows: out [B,C,H,W] / labels [B,H,W] expected, got {tuple(out.shape)} / {tuple(labels.shape)}")
    b, c, h, w = out.shape
    if rows.dim() != 2 or rows.shape[1] != c or rows.shape[0] == 0 or tuple(row_labels.shape) != (rows.shape[0],) or count.numel() != 1:
        raise RuntimeError(f"calib_rows: rows [cap,{c}] / row_labels [cap] / count [1] expected, got {tuple(rows.shape)} / "
                           f"{tuple(row_labels.shape)} / {tuple(count.shape)}")
    lib = _lib.load()
    ws = torch.empty(lib.slu_calib_rows_workspace_bytes(b, h * w), dtype=torch.uint8, device=out.device)
    check(lib.slu_calib_rows(out.data_ptr(), CALIB_KINDS[kind], labels.data_ptr(), b, c, h * w, 0 if ignore_index is None else 1,
                             0 if ignore_index is None else int(ignore_index), rows.data_ptr(), row_labels.data_ptr(), rows.shape[0],
                             count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "slu_calib_rows")


def temp_nll(rows: torch.Tensor, row_labels: torch.Tensor, log_T: torch.Tensor, idx: Optional[torch.Tensor] = None):
    """rows fp32 [N,C], row_labels int64 [N], log_T fp32 [1] (all on the device), idx int64 [M] or None -> (loss_sum float64 [1],
    g_sum float64 [1], bad int64 [1]) on the device: the sums of NLL(rows[i] / T) and of its derivative by log T over i = idx[j] (None: all
    rows), T = max(exp(log_T), 1e-3); bad = rows skipped because their label is outside [0, C) or their index outside [0, N).  The
    temperature is read on the device: no host synchronisation."""
    _req(rows, "rows")
    _req(row_labels, "row_labels", torch.int64)
    _req(log_T, "log_T")
    if rows.dim() != 2 or rows.numel() == 0 or tuple(row_labels.shape) != (rows.shape[0],) or log_T.numel() != 1:
        raise RuntimeError(f"temp_nll: rows [N,C] / row_labels [N] / log_T [1] expected, got {tuple(rows.shape)} / {tuple(row_labels.shape)} / "
                           f"{tuple(log_T.shape)}")
    m = 0
    if idx is not None:
        _req(idx, "idx", torch.int64)
        if idx.dim() != 1 or idx.numel() == 0:
            raise RuntimeError(f"temp_nll: idx must be a non-empty 1-D tensor, got {tuple(idx.shape)}")
        m = idx.numel()
    n, c = rows.shape
    lib = _lib.load()
    ws = torch.empty(lib.slu_temp_nll_workspace_bytes(m or n), dtype=torch.uint8, device=rows.device)
    loss = torch.empty(1, dtype=torch.float64, device=rows.device)
    g = torch.empty(1, dtype=torch.float64, device=rows.device)
    bad = torch.empty(1, dtype=torch.int64, device=rows.device)
    check(lib.slu_temp_nll(rows.data_ptr(), row_labels.data_ptr(), n, c, _ptr(idx), m, log_T.data_ptr(), loss.data_ptr(), g.data_ptr(),
                           bad.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "slu_temp_nll")
    return loss, g, bad


def _c_params(params):
    import ctypes as C
    vals = [float(v) for v in params]
    return (C.c_float * max(1, len(vals)))(*vals), len(vals)


def dirichlet_loss_fwd_ex(alpha: torch.Tensor, labels: torch.Tensor, kind: str, params, eps: float, ignore_index):
    """-> (sums float64 [2] = {sum of values, sum of gates (kind "wrong_low_evidence")}, count int64 [1]); `params` per include/slu.h."""
    b, c, h, w = _dirichlet_loss_args(alpha, labels)
    s = torch.empty(2, dtype=torch.float64, device=alpha.device)
    n = torch.empty(1, dtype=torch.int64, device=alpha.device)
    arr, k = _c_params(params)
    check(_lib.load().slu_dirichlet_loss_fwd_ex(alpha.data_ptr(), labels.data_ptr(), b, c, h * w, DIRICHLET_LOSS_KINDS[kind], arr, k, float(eps),
                                                0 if ignore_index is None else 1, 0 if ignore_index is None else int(ignore_index), s.data_ptr(),
                                                n.data_ptr(), _stream()), "slu_dirichlet_loss_fwd_ex")
    return s, n


def dirichlet_loss_bwd_ex(alpha: torch.Tensor, labels: torch.Tensor, kind: str, params, eps: float, ignore_index, gscale: torch.Tensor):
    b, c, h, w = _dirichlet_loss_args(alpha, labels)
    _req(gscale, "gscale")
    g = torch.empty_like(alpha)
    arr, k = _c_params(params)
    check(_lib.load().slu_dirichlet_loss_bwd_ex(alpha.data_ptr(), labels.data_ptr(), b, c, h * w, DIRICHLET_LOSS_KINDS[kind], arr, k, float(eps),
                                                0 if ignore_index is None else 1, 0 if ignore_index is None else int(ignore_index),
                                                gscale.data_ptr(), g.data_ptr(), _stream()), "slu_dirichlet_loss_bwd_ex")
    return g


# ------------------------------------------------------------------------------------------------
# spherical projection (dataset/utils.py of the reference)
# ------------------------------------------------------------------------------------------------
def spherical_projection(pc: torch.Tensor, height: int, width: int, theta_range=None, bins_h: Optional[torch.Tensor] = None,
                         bins_increasing: bool = False, keep_farthest: bool = False, flip: bool = False, out: Optional[torch.Tensor] = None):
    """pc float64 [N, C >= 3] on the GPU -> (img fp32 [H, W, C], theta_range float64 [2] on the device).  Default: the nearest point of a
    pixel survives; keep_farthest = the reference's sort_largest_first=True; bins_h: float64 [H] explicit monotone row bins on the device;
    flip: columns reversed and y negated while writing (the dataloaders' flip augmentation)."""
    _req(pc, "pc", torch.float64)
    if pc.dim() != 2 or pc.shape[1] < 3 or pc.shape[0] == 0:
        raise RuntimeError(f"pc: expected [N, C >= 3], got {tuple(pc.shape)}")
    n, c = pc.shape
    lib = _lib.load()
    if bins_h is not None:
        _req(bins_h, "bins_h", torch.float64)
        if bins_h.dim() != 1 or bins_h.numel() != int(height):
            raise RuntimeError(f"bins_h: expected {int(height)} row bins, got {tuple(bins_h.shape)}")
    ws = torch.empty(lib.slu_spherical_projection_workspace_bytes(n, int(height), int(width)), dtype=torch.uint8, device=pc.device)
    if out is None:
        img = torch.empty((int(height), int(width), c), dtype=torch.float32, device=pc.device)
    else:
        img = _req(out, "out")
        if tuple(img.shape) != (int(height), int(width), c):
            raise RuntimeError(f"out: expected {(int(height), int(width), c)}, got {tuple(img.shape)}")
    tr = torch.empty(2, dtype=torch.float64, device=pc.device)
    use_data = theta_range is None
    tmin, tmax = (0.0, 0.0) if use_data else (float(theta_range[0]), float(theta_range[1]))
    check(lib.slu_spherical_projection_ex(pc.data_ptr(), n, c, int(height), int(width), 1 if use_data else 0, tmin, tmax, _ptr(bins_h),
                                          1 if bins_increasing else 0, 1 if keep_farthest else 0, 1 if flip else 0, ws.data_ptr(), ws.numel(),
                                          img.data_ptr(), tr.data_ptr(), _stream()), "slu_spherical_projection_ex")
    return img, tr


def resize_nearest_hwc(img: torch.Tensor, out_h: int, out_w: int, flip: bool = False) -> torch.Tensor:
    """cv2.resize(img, (out_w, out_h), interpolation=cv2.INTER_NEAREST) of an [H, W, C] fp32 image [+ the dataloader's flip afterwards]."""
    _req(img, "img")
    if img.dim() != 3:
        raise RuntimeError(f"resize_nearest_hwc: [H, W, C] expected, got {tuple(img.shape)}")
    h, w, c = img.shape
    out = torch.empty((int(out_h), int(out_w), c), dtype=torch.float32, device=img.device)
    check(_lib.load().slu_resize_nearest_hwc(img.data_ptr(), h, w, c, out.data_ptr(), int(out_h), int(out_w), 1 if flip else 0, _stream()),
          "slu_resize_nearest_hwc")
    return out


def kitti_decode(xyzi: torch.Tensor, label: torch.Tensor, lut: torch.Tensor, bad_count: torch.Tensor, rotate_deg: Optional[float] = None):
    """.bin contents fp32 [N, 4] + .label contents int32 [N] (the uint32 words) + id_map LUT int32 -> float64 [N, 5] (x, y, z, i, class);
    rotate_deg: yaw of dataset.utils.rotate_z.  bad_count int32 [1] accumulates labels without a LUT entry."""
    import math
    _req(xyzi, "xyzi")
    _req(label, "label", torch.int32)
    _req(lut, "lut", torch.int32)
    _req(bad_count, "bad_count", torch.int32)
    if xyzi.dim() != 2 or xyzi.shape[1] != 4 or label.dim() != 1 or label.numel() != xyzi.shape[0] or xyzi.shape[0] == 0:
        raise RuntimeError(f"kitti_decode: xyzi [N, 4] / label [N] expected, got {tuple(xyzi.shape)} / {tuple(label.shape)}")
    n = xyzi.shape[0]
    pc = torch.empty((n, 5), dtype=torch.float64, device=xyzi.device)
    ang = 0.0 if rotate_deg is None else math.radians(float(rotate_deg))
    if rotate_deg is not None:
        import numpy as np                      # the reference builds the matrix with numpy's cos / sin of np.radians(angle)
        ang = float(np.radians(float(rotate_deg)))
        ca, sa = float(np.cos(ang)), float(np.sin(ang))
    else:
        ca, sa = 1.0, 0.0
    check(_lib.load().slu_kitti_decode(xyzi.data_ptr(), label.data_ptr(), n, lut.data_ptr(), lut.numel(), 0 if rotate_deg is None else 1, ca, sa,
                                       pc.data_ptr(), bad_count.data_ptr(), _stream()), "slu_kitti_decode")
    return pc


def range_image_split(img: torch.Tensor, normals: Optional[torch.Tensor], range_out, refl_out, xyz_out, normals_out, labels_out) -> None:
    """Projected image fp32 [H, W, C >= 5] (+ normals [H, W, 3]) -> the dataloader's outputs written into the given (slices of batch)
    tensors: range [1,H,W], reflectivity [1,H,W], xyz [3,H,W], normals [3,H,W], labels int64 [1,H,W]."""
    _req(img, "img")
    h, w, c = img.shape
    for t, nme, shape, dt in ((range_out, "range_out", (1, h, w), torch.float32), (refl_out, "refl_out", (1, h, w), torch.float32),
                              (xyz_out, "xyz_out", (3, h, w), torch.float32), (labels_out, "labels_out", (1, h, w), torch.int64)):
        _req(t, nme, dt)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{nme}: expected {shape}, got {tuple(t.shape)}")
    if normals is not None:
        _req(normals, "normals")
        _req(normals_out, "normals_out")
        if tuple(normals.shape) != (h, w, 3) or tuple(normals_out.shape) != (3, h, w):
            raise RuntimeError("normals: expected [H, W, 3] in and [3, H, W] out")
    check(_lib.load().slu_range_image_split(img.data_ptr(), _ptr(normals), h, w, c, range_out.data_ptr(), refl_out.data_ptr(), xyz_out.data_ptr(),
                                            _ptr(normals_out) if normals is not None else None, labels_out.data_ptr(), _stream()), "slu_range_image_split")


def _yaw(rotate_deg):
    """(flag, cos, sin) of dataset.utils.rotate_z: numpy's cos / sin of np.radians(angle), as the reference builds its matrix."""
    if rotate_deg is None:
        return 0, 1.0, 0.0
    import numpy as np
    ang = float(np.radians(float(rotate_deg)))
    return 1, float(np.cos(ang)), float(np.sin(ang))


def point_decode(records: torch.Tensor, label: torch.Tensor, bad_count: torch.Tensor, lut: Optional[torch.Tensor] = None, intensity_div: float = 0.0,
                 mask_labels: bool = True, remap=None, clip_min: Optional[float] = None, rotate_deg: Optional[float] = None):
    """File contents fp32 [N, 4 or 5] + label int32 [N] (the uint32 words) -> (cloud float64 [N, 5] = (x, y, z, i, class), valid uint8 [N] or
    None).  intensity_div: float32 division of the intensity (0: none); mask_labels: label & 0xFFFF; lut: int32 id_map table (None: raw
    labels); remap: (from, to) applied to the class; clip_min: valid[i] = float32 |xyz| >= clip_min, taken before the yaw `rotate_deg`."""
    _req(records, "records")
    _req(label, "label", torch.int32)
    _req(bad_count, "bad_count", torch.int32)
    if lut is not None:
        _req(lut, "lut", torch.int32)
    if records.dim() != 2 or records.shape[1] not in (4, 5) or label.dim() != 1 or label.numel() != records.shape[0] or records.shape[0] == 0:
        raise RuntimeError(f"point_decode: records [N, 4 or 5] / label [N] expected, got {tuple(records.shape)} / {tuple(label.shape)}")
    if bad_count.numel() < 1 or not float(intensity_div) >= 0.0:
        raise RuntimeError("point_decode: bad_count needs one element and intensity_div must be >= 0")
    if remap is not None and (len(remap) != 2 or int(remap[0]) < 0):
        raise RuntimeError(f"point_decode: remap is (from >= 0, to), got {remap!r}")
    n, stride = records.shape
    pc = torch.empty((n, 5), dtype=torch.float64, device=records.device)
    valid = None if clip_min is None else torch.empty(n, dtype=torch.uint8, device=records.device)
    rot, ca, sa = _yaw(rotate_deg)
    rf, rt = (-1, 0) if remap is None else (int(remap[0]), int(remap[1]))
    check(_lib.load().slu_point_decode(records.data_ptr(), stride, label.data_ptr(), n, float(intensity_div), 1 if mask_labels else 0, _ptr(lut),
                                       0 if lut is None else lut.numel(), rf, rt, 0 if clip_min is None else 1,
                                       0.0 if clip_min is None else float(clip_min), rot, ca, sa, pc.data_ptr(), _ptr(valid), bad_count.data_ptr(),
                                       _stream()), "slu_point_decode")
    return pc, valid


def spherical_projection_valid(pc: torch.Tensor, valid: torch.Tensor, height: int, width: int, theta_range=None, flip: bool = False,
                               empty_count: Optional[torch.Tensor] = None) -> torch.Tensor:
    """spherical_projection over the points with valid[i] != 0 (the others take no part in the data theta range and win no pixel) -> img fp32
    [H, W, C].  empty_count int32 [1]: += 1 when theta_range is None and no point is valid (the reference's theta.min() raises there)."""
    _req(pc, "pc", torch.float64)
    _req(valid, "valid", torch.uint8)
    if pc.dim() != 2 or pc.shape[1] < 3 or pc.shape[0] == 0 or valid.dim() != 1 or valid.numel() != pc.shape[0]:
        raise RuntimeError(f"spherical_projection_valid: pc [N, C >= 3] / valid [N] expected, got {tuple(pc.shape)} / {tuple(valid.shape)}")
    if empty_count is not None:
        _req(empty_count, "empty_count", torch.int32)
    n, c = pc.shape
    lib = _lib.load()
    ws = torch.empty(lib.slu_spherical_projection_workspace_bytes(n, int(height), int(width)), dtype=torch.uint8, device=pc.device)
    img = torch.empty((int(height), int(width), c), dtype=torch.float32, device=pc.device)
    use_data = theta_range is None
    tmin, tmax = (0.0, 0.0) if use_data else (float(theta_range[0]), float(theta_range[1]))
    check(lib.slu_spherical_projection_valid(pc.data_ptr(), valid.data_ptr(), n, c, int(height), int(width), 1 if use_data else 0, tmin, tmax,
                                             1 if flip else 0, ws.data_ptr(), ws.numel(), img.data_ptr(), _ptr(empty_count), _stream()),
          "slu_spherical_projection_valid")
    return img


def organised_scan(records: torch.Tensor, label: torch.Tensor, lut: torch.Tensor, bad_count: torch.Tensor, height: int, width: int, flip: bool = False,
                   shift: int = 0, rotate_deg: Optional[float] = None):
    """An organised scan's file contents fp32 [H*W, 4] + label int32 [H*W] -> (img fp32 [H, W, 5], range fp32 [H, W]): id_map, flip, np.roll by
    `shift` columns, yaw, in float64 and in that order; range is the float64 norm rounded to float32 (SemanticTHAB.__getitem__)."""
    _req(records, "records")
    _req(label, "label", torch.int32)
    _req(lut, "lut", torch.int32)
    _req(bad_count, "bad_count", torch.int32)
    h, w = int(height), int(width)
    if h < 1 or w < 1 or records.dim() != 2 or tuple(records.shape) != (h * w, 4) or label.dim() != 1 or label.numel() != h * w:
        raise RuntimeError(f"organised_scan: records [{h * w}, 4] / label [{h * w}] expected for a {h} x {w} scan, got {tuple(records.shape)} / "
                           f"{tuple(label.shape)}")
    img = torch.empty((h, w, 5), dtype=torch.float32, device=records.device)
    rng = torch.empty((h, w), dtype=torch.float32, device=records.device)
    rot, ca, sa = _yaw(rotate_deg)
    check(_lib.load().slu_organised_scan(records.data_ptr(), label.data_ptr(), h, w, lut.data_ptr(), lut.numel(), 1 if flip else 0, int(shift), rot, ca,
                                         sa, img.data_ptr(), rng.data_ptr(), bad_count.data_ptr(), _stream()), "slu_organised_scan")
    return img, rng


def nonempty_rows(img: torch.Tensor) -> torch.Tensor:
    """[H, W, C] fp32 image -> int32 [2 H + 1] on the device: [0] = H' = number of rows with a non-zero pixel, [1 .. H'] = their indices."""
    _req(img, "img")
    if img.dim() != 3 or img.numel() == 0:
        raise RuntimeError(f"nonempty_rows: a non-empty [H, W, C] image expected, got {tuple(img.shape)}")
    h, w, c = img.shape
    rows = torch.empty(2 * h + 1, dtype=torch.int32, device=img.device)
    check(_lib.load().slu_nonempty_rows(img.data_ptr(), h, w, c, rows.data_ptr(), _stream()), "slu_nonempty_rows")
    return rows


def resize_nearest_rows_hwc(img: torch.Tensor, rows: torch.Tensor, out_h: int, out_w: int, no_row_count: torch.Tensor, flip: bool = False) -> torch.Tensor:
    """resize_nearest_hwc of the rows `nonempty_rows` kept [+ flip]; the kept-row count is read on the device.  No row kept: no_row_count
    int32 [1] += 1 and zeros come back (the reference's cv2.resize raises; the caller raises when it reads the counter)."""
    _req(img, "img")
    _req(rows, "rows", torch.int32)
    _req(no_row_count, "no_row_count", torch.int32)
    if img.dim() != 3 or rows.numel() != 2 * img.shape[0] + 1 or no_row_count.numel() < 1 or int(out_h) < 1 or int(out_w) < 1:
        raise RuntimeError(f"resize_nearest_rows_hwc: [H, W, C] image and its nonempty_rows table expected, got {tuple(img.shape)} / {tuple(rows.shape)}")
    h, w, c = img.shape
    out = torch.empty((int(out_h), int(out_w), c), dtype=torch.float32, device=img.device)
    check(_lib.load().slu_resize_nearest_rows_hwc(img.data_ptr(), h, w, c, rows.data_ptr(), out.data_ptr(), int(out_h), int(out_w), 1 if flip else 0,
                                                  no_row_count.data_ptr(), _stream()), "slu_resize_nearest_rows_hwc")
    return out


def channel_max(img: torch.Tensor, channel: int) -> torch.Tensor:
    """Maximum of img[..., channel] of an [H, W, C] fp32 image as the uint32 key (held in an int32 [1] tensor) range_image_split takes."""
    _req(img, "img")
    if img.dim() != 3 or img.numel() == 0 or not 0 <= int(channel) < img.shape[2]:
        raise RuntimeError(f"channel_max: a non-empty [H, W, C] image and a channel below C expected, got {tuple(img.shape)} / {channel}")
    h, w, c = img.shape
    key = torch.empty(1, dtype=torch.int32, device=img.device)
    check(_lib.load().slu_channel_max(img.data_ptr(), h, w, c, int(channel), key.data_ptr(), _stream()), "slu_channel_max")
    return key


def channel_max_value(key: torch.Tensor) -> float:
    """The float32 value a channel_max key stands for (a host read: for tests and tools)."""
    import numpy as np
    k = np.array([int(key.item()) & 0xFFFFFFFF], dtype=np.uint32)
    u = np.where(k >> 31, k & np.uint32(0x7FFFFFFF), ~k)
    return float(u.astype(np.uint32).view(np.float32)[0])


def range_image_split_ex(img: torch.Tensor, normals: Optional[torch.Tensor], range_out, refl_out, xyz_out, normals_out, labels_out,
                         range_in: Optional[torch.Tensor] = None, refl_max_key: Optional[torch.Tensor] = None) -> None:
    """range_image_split with range_in fp32 [H, W] (copied instead of |xyz|: organised_scan's range) and / or refl_max_key (channel_max of
    channel 3: reflectivity / max(maximum, 1) as a float32 division, SemanticCUDAL)."""
    _req(img, "img")
    h, w, c = img.shape
    for t, nme, shape, dt in ((range_out, "range_out", (1, h, w), torch.float32), (refl_out, "refl_out", (1, h, w), torch.float32),
                              (xyz_out, "xyz_out", (3, h, w), torch.float32), (labels_out, "labels_out", (1, h, w), torch.int64)):
        _req(t, nme, dt)
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{nme}: expected {shape}, got {tuple(t.shape)}")
    if normals is not None:
        _req(normals, "normals")
        _req(normals_out, "normals_out")
        if tuple(normals.shape) != (h, w, 3) or tuple(normals_out.shape) != (3, h, w):
            raise RuntimeError("normals: expected [H, W, 3] in and [3, H, W] out")
    if range_in is not None:
        _req(range_in, "range_in")
        if tuple(range_in.shape) != (h, w):
            raise RuntimeError(f"range_in: expected {(h, w)}, got {tuple(range_in.shape)}")
    if refl_max_key is not None:
        _req(refl_max_key, "refl_max_key", torch.int32)
    check(_lib.load().slu_range_image_split_ex(img.data_ptr(), _ptr(normals), h, w, c, _ptr(range_in), _ptr(refl_max_key), range_out.data_ptr(),
                                               refl_out.data_ptr(), xyz_out.data_ptr(), _ptr(normals_out) if normals is not None else None,
                                               labels_out.data_ptr(), _stream()), "slu_range_image_split_ex")


# ------------------------------------------------------------------------------------------------
# Dropout2d multipliers of a whole MC evaluation in one launch (csrc/dropout_draw.hip)
# ------------------------------------------------------------------------------------------------
class DropoutPlan:
    """Device tables for slu_dropout_draw: `sites` = [(C, p, active)], `outs` = [(key, C, (site, offset) x <= 3, shuffled)] for batch size n
    (shuffled: 0 / 1, or 2 = shuffled and written in the stored order of a tensor read through PixelShuffle in place)."""

    def __init__(self, n: int, sites, outs, device):
        import numpy as np
        self.n, self.device = int(n), device
        st = np.zeros(len(sites), dtype=np.dtype([("begin", "<i8"), ("C", "<i4"), ("active", "<i4"), ("p", "<f4"), ("reserved", "<i4")]))
        g = 0
        for i, (c, p, active) in enumerate(sites):
            st[i] = (g, c, 1 if active else 0, p, 0)
            if active:
                g += self.n * c
        self.draws = g
        ot = np.zeros(len(outs), dtype=np.dtype([("begin", "<i8"), ("C", "<i4"), ("site_a", "<i4"), ("off_a", "<i4"), ("site_b", "<i4"), ("off_b", "<i4"),
                                                 ("site_c", "<i4"), ("off_c", "<i4"), ("shuffled", "<i4")]))
        e, self.slices = 0, []
        for i, (key, c, refs, shuffled) in enumerate(outs):
            refs = list(refs) + [(-1, 0)] * (3 - len(refs))
            ot[i] = (e, c, refs[0][0], refs[0][1], refs[1][0], refs[1][1], refs[2][0], refs[2][1], int(shuffled))
            self.slices.append((key, e, c))
            e += self.n * c
        self.total = e
        assert st.dtype.itemsize == 24 and ot.dtype.itemsize == 40
        self.sites = torch.from_numpy(st.view(np.uint8).copy()).to(device)
        self.outs = torch.from_numpy(ot.view(np.uint8).copy()).to(device)
        self.nsites, self.nout = len(sites), len(outs)

    def run(self, out: Optional[torch.Tensor] = None):
        """{key: [n, C] multiplier}: one launch; consumes ceil(draws / 4) (rounded up to a multiple of 4) counters of torch's CUDA generator.
        out: a float32 buffer of `self.total` elements to draw into (a captured HIP graph reads the multipliers from fixed addresses)."""
        gen = torch.cuda.default_generators[self.device.index if self.device.index is not None else torch.cuda.current_device()]
        seed, off = int(gen.initial_seed()), int(gen.get_offset())
        adv = ((self.draws + 3) // 4 + 3) // 4 * 4
        gen.set_offset(off + adv)
        if out is None:
            buf = torch.empty(self.total, dtype=torch.float32, device=self.device)
        else:
            buf = _req(out, "out")
            if buf.numel() != self.total:
                raise RuntimeError(f"DropoutPlan.run: out holds {buf.numel()} elements, the plan needs {self.total}")
        check(_lib.load().slu_dropout_draw(self.sites.data_ptr(), self.nsites, self.outs.data_ptr(), self.nout, self.n, seed & (2 ** 64 - 1), off, buf.data_ptr(),
                                           self.total, _stream()), "slu_dropout_draw")
        return {key: buf[b:b + self.n * c].view(self.n, c) for key, b, c in self.slices}


# ------------------------------------------------------------------------------------------------
# EfficientNetV2 pieces (csrc/effnet_ops.hip)
# ------------------------------------------------------------------------------------------------
def dwconv3x3(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1, act: str = "none") -> torch.Tensor:
    """Depthwise 3x3 (padding 1, stride 1 / 2) + bias [+ SiLU]; w [C, 9] (eval BatchNorm already folded in)."""
    _req(x, "x")
    _req(w, "w")
    n, c, h, wd = x.shape
    if tuple(w.shape) != (c, 9) or (bias is not None and bias.numel() != c):
        raise RuntimeError(f"dwconv3x3: weight {tuple(w.shape)} / bias do not match {c} channels")
    if bias is not None:
        _req(bias, "bias")
    oh, ow = (h + stride - 1) // stride, (wd + stride - 1) // stride
    y = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_dwconv3x3_fwd(x.data_ptr(), w.data_ptr(), _ptr(bias), y.data_ptr(), n, c, h, wd, int(stride), {"none": 0, "silu": 3}[act],
                                        _stream()), "slu_dwconv3x3_fwd")
    return y


def dwconv3x3_wgrad(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dL/dw [C, 9] of the stride-1 depthwise 3x3 conv y = dwconv3x3(x, w)."""
    _req(x, "x")
    _req(dy, "dy")
    if x.shape != dy.shape:
        raise RuntimeError("dwconv3x3_wgrad: x / dy shape mismatch")
    n, c, h, w = x.shape
    dw = torch.empty((c, 9), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_dwconv3x3_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), n, c, h, w, _stream()), "slu_dwconv3x3_wgrad")
    return dw


def global_avgpool(x: torch.Tensor) -> torch.Tensor:
    """mean over H W -> [N, C]."""
    _req(x, "x")
    n, c, h, w = x.shape
    avg = torch.empty((n, c), dtype=torch.float32, device=x.device)
    check(_lib.load().slu_global_avgpool(x.data_ptr(), avg.data_ptr(), n, c, h * w, _stream()), "slu_global_avgpool")
    return avg


def se_scale(x: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor]) -> torch.Tensor:
    """SqueezeExcitation's multiplier [N, C] = sigmoid(fc2(SiLU(fc1(mean_HW(x))))); w1 [S, C], w2 [C, S]."""
    _req(x, "x")
    n, c, h, w = x.shape
    s = w1.shape[0]
    _req_shapes((w1, "w1", (s, c)), (w2, "w2", (c, s)))
    lib = _lib.load()
    avg = torch.empty((n, c), dtype=torch.float32, device=x.device)
    check(lib.slu_global_avgpool(x.data_ptr(), avg.data_ptr(), n, c, h * w, _stream()), "slu_global_avgpool")
    scale = torch.empty((n, c), dtype=torch.float32, device=x.device)
    check(lib.slu_se_gate(avg.data_ptr(), w1.data_ptr(), _ptr(b1), w2.data_ptr(), _ptr(b2), scale.data_ptr(), n, c, s, _stream()), "slu_se_gate")
    return scale


def dwconv3x3_se(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, stride: int = 1):
    """The depthwise conv of an MBConv in one launch (slu_dwconv3x3_se_fwd, csrc/mbconv_unit.hip): y = SiLU(depthwise conv3x3 / pad 1 / stride (x)
    + bias) with w [C, 9] (eval BatchNorm folded in by the caller).  Returns (y [N, C, Ho, Wo], psum [N, C, T]): psum holds the per-tile sums of y,
    which se_gate_psum turns into the SqueezeExcitation's mean without reading y back.  y equals dwconv3x3(x, w, bias, stride, "silu") bit for
    bit; exact fp32 under every conv precision; bit-identical run to run."""
    _req(x, "x")
    if x.dim() != 4:
        raise RuntimeError(f"x: expected NCHW, got {tuple(x.shape)}")
    n, c, h, wd = x.shape
    _req(w, "w")
    _req(bias, "bias")
    if tuple(w.shape) != (c, 9) or tuple(bias.shape) != (c,):
        raise RuntimeError(f"dwconv3x3_se: weight {tuple(w.shape)} / bias {tuple(bias.shape)} do not match {c} channels")
    if stride not in (1, 2):
        raise RuntimeError("dwconv3x3_se: stride must be 1 or 2")
    lib = _lib.load()
    t = lib.slu_dwconv3x3_se_tiles(h, wd, int(stride))
    if t <= 0:
        raise RuntimeError(f"dwconv3x3_se: a {h} x {wd} map is outside what slu_dwconv3x3_se_fwd takes")
    y = torch.empty((n, c, (h + stride - 1) // stride, (wd + stride - 1) // stride), dtype=torch.float32, device=x.device)
    psum = torch.empty((n, c, t), dtype=torch.float32, device=x.device)
    check(lib.slu_dwconv3x3_se_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), psum.data_ptr(), n, c, h, wd, int(stride), _stream()),
          "slu_dwconv3x3_se_fwd")
    return y, psum


SE_GATE_MAX_C, SE_GATE_MAX_S = 1536, 96


def _se_gate_from_psum(fn: str, entry: str, psum, count, w1, b1, w2, b2, limit, mean_arg: bool, want_mean: bool = False):
    """se_gate_psum / regnet_se_gate: validation, allocation and the call of `entry` (csrc/se_gate.hip).  limit(c, s): the entry point's range as
    an error text or None; mean_arg: the entry point takes the nullable mean output after the gate."""
    _req(psum, "psum")
    if psum.dim() == 2:
        psum = psum.unsqueeze(2)
    if psum.dim() != 3 or psum.numel() == 0:
        raise RuntimeError(f"psum: expected [N, C, T], got {tuple(psum.shape)}")
    n, c, t = psum.shape
    if int(count) < 1:
        raise RuntimeError(f"{fn}: count must be positive")
    _req(w1, "w1")
    if w1.dim() != 2 or w1.shape[1] != c or w1.shape[0] == 0:
        raise RuntimeError(f"w1: expected [S, {c}], got {tuple(w1.shape)}")
    s = w1.shape[0]
    _req_shapes((b1, "b1", (s,)), (w2, "w2", (c, s)), (b2, "b2", (c,)))
    refusal = limit(c, s)
    if refusal:
        raise RuntimeError(f"{fn}: {refusal}")
    gate = torch.empty((n, c), dtype=torch.float32, device=psum.device)
    mean = torch.empty((n, c), dtype=torch.float32, device=psum.device) if want_mean else None
    outs = (gate.data_ptr(), _ptr(mean)) if mean_arg else (gate.data_ptr(),)
    check(getattr(_lib.load(), entry)(psum.data_ptr(), t, 1.0 / float(count), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), *outs,
                                      n, c, s, _stream()), entry)
    return (gate, mean) if want_mean else gate


def se_gate_psum(psum: torch.Tensor, count: int, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """SqueezeExcitation's multiplier [N, C] = sigmoid(fc2(SiLU(fc1(mean)))) with mean = psum.sum(-1) / count (summed in tile order on the device);
    psum [N, C, T] from dwconv3x3_se with count = Ho Wo, or a plain mean as [N, C, 1] (or [N, C]) with count = 1.  w1 [S, C], b1 [S], w2 [C, S],
    b2 [C]; C <= 1536 and S <= 96, the range of se_scale."""
    def limit(c, s):
        if c > SE_GATE_MAX_C or s > SE_GATE_MAX_S:
            return f"C = {c}, S = {s} is outside the kernel's C <= {SE_GATE_MAX_C}, S <= {SE_GATE_MAX_S}"
    return _se_gate_from_psum("se_gate_psum", "slu_se_gate_psum", psum, count, w1, b1, w2, b2, limit, False)


# ------------------------------------------------------------------------------------------------
# The two-source input of the encoder unit kernels (slu_cat2, csrc/encoder_unit.h)
# ------------------------------------------------------------------------------------------------
def _channel_range(t: torch.Tensor, name: str, coff: int, cuse: int):
    """(coff, c) of t[:, coff:coff + cuse] of an NCHW tensor (cuse = 0: every channel from coff on), checked."""
    _req(t, name)
    if t.dim() != 4:
        raise RuntimeError(f"{name}: expected NCHW, got {tuple(t.shape)}")
    ct = t.shape[1]
    coff, cuse = int(coff), int(cuse)
    c = cuse if cuse else ct - coff
    if coff < 0 or c <= 0 or coff + c > ct:
        raise RuntimeError(f"{name}: channel range [{coff}, {coff + c}) is outside the tensor's {ct} channels")
    return coff, c


def _two_sources(src: torch.Tensor, coff: int, cuse: int, src2: Optional[torch.Tensor]):
    """cat(src[:, coff:coff + cuse], src2) (cuse = 0: every channel from coff on), checked: (its _lib.Cat2, (n, h, w, c))."""
    coff, c0 = _channel_range(src, "src", coff, cuse)
    n, ct0, h, w = src.shape
    ct1 = 0
    if src2 is not None:
        _req(src2, "src2")
        if src2.dim() != 4 or (src2.shape[0], src2.shape[2], src2.shape[3]) != (n, h, w) or src2.shape[1] == 0:
            raise RuntimeError(f"src2: expected [{n}, > 0, {h}, {w}], got {tuple(src2.shape)}")
        ct1 = src2.shape[1]
    return _lib.Cat2(src.data_ptr(), _ptr(src2), ct0, coff, c0, ct1, ct1), (n, h, w, c0 + ct1)


# ------------------------------------------------------------------------------------------------
# ShuffleNetV2 unit tail (csrc/shuffle_unit.hip)
# ------------------------------------------------------------------------------------------------
def pack_shuffle_tail_weight(w: torch.Tensor) -> torch.Tensor:
    """[Co, C] fp32 pointwise weight -> the MFMA A-fragment image slu_shuffle_tail_fwd streams (re-run after every weight update)."""
    _req(w, "w")
    if w.dim() != 2:
        raise RuntimeError(f"pack_shuffle_tail_weight: expected [Co, C], got {tuple(w.shape)}")
    lib = _lib.load()
    co, c = w.shape
    n = lib.slu_shuffle_tail_packed_floats(co, c)
    if n == 0:
        raise _lib.SluError(f"slu_shuffle_tail_pack: {lib.slu_strerror(-2).decode()} (code -2): Co={co}")
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    check(lib.slu_shuffle_tail_pack(w.data_ptr(), co, c, out.data_ptr(), _stream()), "slu_shuffle_tail_pack")
    return out


def shuffle_tail(src: torch.Tensor, wdw: torch.Tensor, bdw: torch.Tensor, wpack: torch.Tensor, bpw: torch.Tensor, co: int, stride: int,
                 out: Optional[torch.Tensor] = None, parity: int = 1, coff: int = 0, cuse: int = 0, src2: Optional[torch.Tensor] = None,
                 passthrough: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The tail of a ShuffleNetV2 unit in one launch (slu_shuffle_tail_fwd): y = relu(W_pw . (dw3x3_stride(src) + bdw) + bpw) with both eval
    BatchNorms folded into the weights, stored as out[:, 2 j + parity] = y[j] -- the unit's concat + channel_shuffle(., 2) -- and, with
    `passthrough`, out[:, 2 j] = passthrough[:, j] for j < co.  src is cat(src[:, coff:coff + cuse], src2) (cuse = 0: every channel from coff on;
    src2 optional), wdw [C, 9], bdw [C], wpack = pack_shuffle_tail_weight(W_pw [co, C]), bpw [co].  out [N, 2 co, Ho, Wo] is allocated when not
    given; without `passthrough` its channels of the other parity are left as they were.  The depthwise result stays on chip.  The pointwise
    product is the exact-fp32 MFMA under every conv precision ('fp32' and 'f16x3' alike): the kernel is bandwidth-bound, split products buy nothing."""
    cat, (n, h, w, c) = _two_sources(src, coff, cuse, src2)
    if stride not in (1, 2) or parity not in (0, 1) or co <= 0:
        raise RuntimeError("shuffle_tail: stride must be 1 or 2, parity 0 or 1, co positive")
    lib = _lib.load()
    _req_shapes((wdw, "wdw", (c, 9)), (bdw, "bdw", (c,)), (bpw, "bpw", (co,)))
    _req(wpack, "wpack")
    want = lib.slu_shuffle_tail_packed_floats(co, c)
    if want and wpack.numel() != want:
        raise RuntimeError(f"wpack: {wpack.numel()} floats does not match Co={co} C={c}")
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    d = _lib.ShuffleTailDesc()
    if passthrough is not None:
        _req(passthrough, "passthrough")
        if passthrough.dim() != 4 or (passthrough.shape[0], passthrough.shape[2], passthrough.shape[3]) != (n, ho, wo) or passthrough.shape[1] < co:
            raise RuntimeError(f"passthrough: expected [{n}, >= {co}, {ho}, {wo}], got {tuple(passthrough.shape)}")
        if parity != 1:
            raise RuntimeError("shuffle_tail: the pass-through half takes the even channels, so parity must be 1")
        d.pass_, d.pass_ct = passthrough.data_ptr(), passthrough.shape[1]
    out = _out_or_new("shuffle_tail", out, (n, 2 * co, ho, wo), (src, src2, passthrough))
    d.in_ = cat
    d.N, d.H, d.W, d.stride, d.Co, d.parity = n, h, w, int(stride), int(co), int(parity)
    d.wdw, d.bdw, d.wpack, d.bpw, d.out = wdw.data_ptr(), bdw.data_ptr(), wpack.data_ptr(), bpw.data_ptr(), out.data_ptr()
    check(lib.slu_shuffle_tail_fwd(C.byref(d), _stream()), "slu_shuffle_tail_fwd")
    return out


# ------------------------------------------------------------------------------------------------
# SqueezeNet Fire module and ceil-mode max-pool (csrc/fire_unit.hip)
# ------------------------------------------------------------------------------------------------
def pack_fire_weight(wsq: torch.Tensor, w1: torch.Tensor, w3: torch.Tensor) -> torch.Tensor:
    """wsq [S, Cin], w1 [E1, S], w3 [E3, S, 3, 3] fp32 -> the MFMA A-fragment images slu_fire_fwd streams (re-run after every weight update)."""
    for t, nme in ((wsq, "wsq"), (w1, "w1"), (w3, "w3")):
        _req(t, nme)
    if wsq.dim() != 2 or w1.dim() != 2 or w3.dim() != 4:
        raise RuntimeError(f"pack_fire_weight: expected [S, Cin], [E1, S], [E3, S, 3, 3], got {tuple(wsq.shape)}, {tuple(w1.shape)}, {tuple(w3.shape)}")
    s, cin = wsq.shape
    e1, e3 = w1.shape[0], w3.shape[0]
    if w1.shape[1] != s or tuple(w3.shape[1:]) != (s, 3, 3):
        raise RuntimeError(f"pack_fire_weight: w1 {tuple(w1.shape)} / w3 {tuple(w3.shape)} do not match S = {s}")
    lib = _lib.load()
    n = lib.slu_fire_packed_floats(cin, s, e1, e3)
    if n == 0:
        raise _lib.SluError(f"slu_fire_pack: {lib.slu_strerror(-2).decode()} (code -2): Cin={cin} S={s} E1={e1} E3={e3}")
    out = torch.empty(n, dtype=torch.float32, device=wsq.device)
    check(lib.slu_fire_pack(wsq.data_ptr(), w1.data_ptr(), w3.data_ptr(), cin, s, e1, e3, out.data_ptr(), _stream()), "slu_fire_pack")
    return out


def fire(src: torch.Tensor, wpack: torch.Tensor, bsq: torch.Tensor, b1: torch.Tensor, b3: torch.Tensor, out: Optional[torch.Tensor] = None,
         coff: int = 0, cuse: int = 0, src2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One SqueezeNet Fire module in one launch (slu_fire_fwd): s = relu(squeeze 1x1), out = cat(relu(expand 1x1 (s)), relu(expand 3x3 / pad 1 (s)));
    the squeeze map stays in LDS.  src is cat(src[:, coff:coff + cuse], src2) (cuse = 0: every channel from coff on; src2 optional),
    wpack = pack_fire_weight(wsq, w1, w3), bsq [S], b1 [E1], b3 [E3].  out [N, E1 + E3, H, W] is allocated when not given and must not overlap an
    input.  Every product is the exact-fp32 MFMA under every conv precision ('fp32' and 'f16x3' alike)."""
    cat, (n, h, w, cin) = _two_sources(src, coff, cuse, src2)
    for t, nme in ((bsq, "bsq"), (b1, "b1"), (b3, "b3")):
        _req(t, nme)
        if t.dim() != 1 or t.numel() == 0:
            raise RuntimeError(f"{nme}: expected a non-empty vector, got {tuple(t.shape)}")
    s, e1, e3 = bsq.numel(), b1.numel(), b3.numel()
    lib = _lib.load()
    _req(wpack, "wpack")
    want = lib.slu_fire_packed_floats(cin, s, e1, e3)
    if want == 0:
        raise RuntimeError(f"fire: Cin={cin} S={s} E1={e1} E3={e3} is outside what slu_fire_fwd takes (S <= 64, E1 and E3 <= 256)")
    if wpack.numel() != want:
        raise RuntimeError(f"wpack: {wpack.numel()} floats does not match Cin={cin} S={s} E1={e1} E3={e3}")
    out = _out_or_new("fire", out, (n, e1 + e3, h, w), (src, src2))
    d = _lib.FireDesc()
    d.in_ = cat
    d.N, d.H, d.W, d.S, d.E1, d.E3 = n, h, w, s, e1, e3
    d.wpack, d.bsq, d.b1, d.b3, d.out = wpack.data_ptr(), bsq.data_ptr(), b1.data_ptr(), b3.data_ptr(), out.data_ptr()
    check(lib.slu_fire_fwd(C.byref(d), _stream()), "slu_fire_fwd")
    return out


def maxpool3s2_ceil(src: torch.Tensor, coff: int = 0, cuse: int = 0, src2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.MaxPool2d(3, 2, padding=0, ceil_mode=True) of cat(src[:, coff:coff + cuse], src2) -> [N, C, ceil((H - 3) / 2) + 1, ceil((W - 3) / 2) + 1]."""
    cat, (n, h, w, c) = _two_sources(src, coff, cuse, src2)
    if h < 3 or w < 3:
        raise RuntimeError(f"maxpool3s2_ceil: H and W must be at least 3, got {h} x {w}")
    y = torch.empty((n, c, (h - 2) // 2 + 1, (w - 2) // 2 + 1), dtype=torch.float32, device=src.device)
    check(_lib.load().slu_maxpool3s2_ceil_fwd(C.byref(cat), y.data_ptr(), n, h, w, _stream()), "slu_maxpool3s2_ceil_fwd")
    return y


# ------------------------------------------------------------------------------------------------
# RegNetY block: grouped 3x3 conv + SE mean, ReLU SE gate, stride-2 sampling (csrc/regnet_unit.hip)
# ------------------------------------------------------------------------------------------------
REGNET_GROUP_WIDTHS = (8, 16, 24)


def pack_regnet_gconv_weight(w: torch.Tensor, gw: int) -> torch.Tensor:
    """[C, gw, 3, 3] weight of a grouped 3x3 conv (groups = C / gw) -> [C / gw, gw (c), 9, gw (o)], the order slu_regnet_gconv_fwd reads: the
    9 gw weights one input channel of a group feeds are consecutive (re-run after every weight update)."""
    _req(w, "w")
    gw = int(gw)
    if gw not in REGNET_GROUP_WIDTHS:
        raise RuntimeError(f"pack_regnet_gconv_weight: group width {gw} is not one of {REGNET_GROUP_WIDTHS}")
    if w.dim() != 4 or tuple(w.shape[1:]) != (gw, 3, 3) or w.shape[0] % gw:
        raise RuntimeError(f"pack_regnet_gconv_weight: expected [C, {gw}, 3, 3] with C a multiple of {gw}, got {tuple(w.shape)}")
    return w.reshape(w.shape[0] // gw, gw, gw, 9).permute(0, 2, 3, 1).contiguous()


def regnet_gconv(x: torch.Tensor, wg: torch.Tensor, bias: torch.Tensor, stride: int = 1, coff: int = 0, cuse: int = 0,
                 out: Optional[torch.Tensor] = None):
    """RegNet's f.b in one launch (slu_regnet_gconv_fwd): y = relu(grouped conv3x3 / pad 1 / stride (x[:, coff:coff + cuse]) + bias) with
    wg = pack_regnet_gconv_weight(w, gw) (eval BatchNorm folded in by the caller), cuse = 0: every channel from coff on.  Returns (y [N, C, Ho, Wo],
    psum [N, C, T]): psum holds the per-tile sums of y, which regnet_se_gate turns into the SqueezeExcitation's mean without reading y back.
    Exact fp32 under every conv precision; bit-identical run to run."""
    coff, c = _channel_range(x, "x", coff, cuse)
    n, ct, h, w = x.shape
    _req(wg, "wg")
    if wg.dim() != 4 or wg.shape[1] != wg.shape[3] or wg.shape[2] != 9 or wg.shape[1] not in REGNET_GROUP_WIDTHS:
        raise RuntimeError(f"wg: expected [G, gw, 9, gw] with gw in {REGNET_GROUP_WIDTHS}, got {tuple(wg.shape)}")
    gw = wg.shape[1]
    if wg.shape[0] * gw != c:
        raise RuntimeError(f"wg: {wg.shape[0]} groups of {gw} do not make the {c} input channels")
    _req_shapes((bias, "bias", (c,)))
    if stride not in (1, 2):
        raise RuntimeError("regnet_gconv: stride must be 1 or 2")
    lib = _lib.load()
    out = _out_or_new("regnet_gconv", out, (n, c, (h + stride - 1) // stride, (w + stride - 1) // stride), (x,))
    t = lib.slu_regnet_gconv_tiles(h, w, int(stride))
    if t <= 0:
        raise RuntimeError(f"regnet_gconv: a {h} x {w} map is outside what slu_regnet_gconv_fwd takes")
    psum = torch.empty((n, c, t), dtype=torch.float32, device=x.device)
    check(lib.slu_regnet_gconv_fwd(x.data_ptr(), ct, coff, wg.data_ptr(), bias.data_ptr(), out.data_ptr(), psum.data_ptr(), n, c, gw, h, w, int(stride),
                                   _stream()), "slu_regnet_gconv_fwd")
    return out, psum


def regnet_se_gate(psum: torch.Tensor, count: int, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, want_mean: bool = False):
    """RegNet's SqueezeExcitation multiplier [N, C] = sigmoid(fc2(relu(fc1(mean)))) with mean = psum.sum(-1) / count (summed in tile order on the
    device); psum [N, C, T] from regnet_gconv with count = Ho Wo, or a plain mean as [N, C, 1] (or [N, C]) with count = 1.  w1 [S, C], b1 [S],
    w2 [C, S], b2 [C].  want_mean: returns (gate, mean)."""
    def limit(c, s):
        if (c + s) * 4 > 64 * 1024:
            return f"C + S = {c + s} does not fit the kernel's 64 KiB of LDS"
    return _se_gate_from_psum("regnet_se_gate", "slu_regnet_se_gate", psum, count, w1, b1, w2, b2, limit, True, want_mean)


def regnet_sample2(src: torch.Tensor, coff: int = 0, cuse: int = 0, src2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cat(src[:, coff:coff + cuse], src2)[:, :, ::2, ::2] -> [N, C, ceil(H / 2), ceil(W / 2)]: the input of a 1x1 / stride-2 projection."""
    cat, (n, h, w, c) = _two_sources(src, coff, cuse, src2)
    y = torch.empty((n, c, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=src.device)
    check(_lib.load().slu_regnet_sample2(C.byref(cat), y.data_ptr(), n, h, w, _stream()), "slu_regnet_sample2")
    return y


# ------------------------------------------------------------------------------------------------
# CENet decoder (baselines/CENet/CENet_ResNet34.py:165-184)
def bilinear_ac_cat(srcs: Sequence[torch.Tensor], size, out: Optional[torch.Tensor] = None, c_offs: Optional[Sequence[int]] = None) -> torch.Tensor:
    """cat([F.interpolate(s, size=size, mode='bilinear', align_corners=True) for s in srcs], 1) in one launch; 1..3 sources [N, C_k, h_k, w_k].
    With `out` [N, C_tot, H, W] source k goes to channels [c_offs[k], c_offs[k] + C_k) (default: one after the other from 0) and every other
    channel keeps its content."""
    if not 1 <= len(srcs) <= 3:
        raise RuntimeError(f"bilinear_ac_cat: 1..3 sources supported, got {len(srcs)}")
    hh, ww = (int(v) for v in size)
    if hh < 1 or ww < 1:
        raise RuntimeError("bilinear_ac_cat: size must be positive")
    n = None
    for i, s in enumerate(srcs):
        _req(s, f"srcs[{i}]")
        if s.dim() != 4 or s.numel() == 0 or (n is not None and s.shape[0] != n):
            raise RuntimeError(f"srcs[{i}]: expected a non-empty [N, C, h, w] tensor with the batch of srcs[0], got {tuple(s.shape)}")
        n = s.shape[0]
    if c_offs is None:
        c_offs, at = [], 0
        for s in srcs:
            c_offs.append(at)
            at += s.shape[1]
    c_offs = [int(v) for v in c_offs]
    if len(c_offs) != len(srcs):
        raise RuntimeError("bilinear_ac_cat: one channel offset per source expected")
    if out is None:
        out = torch.empty((n, max(o + s.shape[1] for o, s in zip(c_offs, srcs)), hh, ww), dtype=torch.float32, device=srcs[0].device)
    else:
        _req(out, "out")
        if out.dim() != 4 or out.shape[0] != n or tuple(out.shape[2:]) != (hh, ww):
            raise RuntimeError(f"out: expected [{n}, C_tot, {hh}, {ww}], got {tuple(out.shape)}")
        if any(_overlaps(out, s) for s in srcs):
            raise RuntimeError("bilinear_ac_cat: out must not overlap a source")
    ctot = out.shape[1]
    arr = (_lib.BilinearSrc * 3)()
    for k, (s, o) in enumerate(zip(srcs, c_offs)):
        if o < 0 or o + s.shape[1] > ctot:
            raise RuntimeError(f"bilinear_ac_cat: channels [{o}, {o + s.shape[1]}) of source {k} leave the {ctot} channels of out")
        if any(o < c_offs[j] + srcs[j].shape[1] and c_offs[j] < o + s.shape[1] for j in range(k)):
            raise RuntimeError(f"bilinear_ac_cat: the channel slice of source {k} overlaps an earlier one")
        arr[k].ptr, arr[k].C, arr[k].h, arr[k].w, arr[k].c_off = s.data_ptr(), s.shape[1], s.shape[2], s.shape[3], o
    check(_lib.load().slu_bilinear_ac_cat(arr, len(srcs), out.data_ptr(), n, ctot, hh, ww, _stream()), "slu_bilinear_ac_cat")
    return out


def bilinear_ac_softmax(logits: torch.Tensor, size=None) -> torch.Tensor:
    """softmax(F.interpolate(logits, size=size, mode='bilinear', align_corners=True), dim=1) in one launch; logits [N, C <= 32, h, w].
    size None (or the logits' own): the plain class softmax."""
    _req(logits, "logits")
    if logits.dim() != 4 or logits.numel() == 0:
        raise RuntimeError(f"logits: expected a non-empty [N, C, h, w] tensor, got {tuple(logits.shape)}")
    n, c, h, w = logits.shape
    if c > 32:
        raise RuntimeError(f"bilinear_ac_softmax: at most 32 classes supported, got {c}")
    hh, ww = (h, w) if size is None else (int(v) for v in size)
    if hh < 1 or ww < 1:
        raise RuntimeError("bilinear_ac_softmax: size must be positive")
    y = torch.empty((n, c, hh, ww), dtype=torch.float32, device=logits.device)
    check(_lib.load().slu_bilinear_ac_softmax(logits.data_ptr(), y.data_ptr(), n, c, h, w, hh, ww, _stream()), "slu_bilinear_ac_softmax")
    return y


def bilinear_ac_sum(srcs: Sequence[torch.Tensor], size) -> torch.Tensor:
    """sum(F.interpolate(s, size=size, mode='bilinear', align_corners=True) for s in srcs) in one launch, the terms added in source order;
    1..3 sources [N, C, h_k, w_k] of one N and C.  One source at the output size comes back bit for bit."""
    if not 1 <= len(srcs) <= 3:
        raise RuntimeError(f"bilinear_ac_sum: 1..3 sources supported, got {len(srcs)}")
    hh, ww = (int(v) for v in size)
    if hh < 1 or ww < 1:
        raise RuntimeError("bilinear_ac_sum: size must be positive")
    n = c = None
    for i, s in enumerate(srcs):
        _req(s, f"srcs[{i}]")
        if s.dim() != 4 or s.numel() == 0 or (n is not None and s.shape[0] != n):
            raise RuntimeError(f"srcs[{i}]: expected a non-empty [N, C, h, w] tensor with the batch of srcs[0], got {tuple(s.shape)}")
        if c is not None and s.shape[1] != c:
            raise RuntimeError(f"srcs[{i}]: expected the {c} channels of srcs[0], got {s.shape[1]}")
        n, c = s.shape[0], s.shape[1]
    out = torch.empty((n, c, hh, ww), dtype=torch.float32, device=srcs[0].device)
    arr = (_lib.BilinearSrc * 3)()
    for k, s in enumerate(srcs):
        arr[k].ptr, arr[k].C, arr[k].h, arr[k].w, arr[k].c_off = s.data_ptr(), c, s.shape[2], s.shape[3], 0
    check(_lib.load().slu_bilinear_ac_sum(arr, len(srcs), out.data_ptr(), n, c, hh, ww, _stream()), "slu_bilinear_ac_sum")
    return out


# ------------------------------------------------------------------------------------------------
# FIDNet's point-MLP stem (csrc/point_mlp.hip; baselines/FIDNet/ResNet.py:469-502, 563-576)
POINT_MLP_MAX_LAYERS, POINT_MLP_MAX_C0, POINT_MLP_MAX_WIDTH = 4, 32, 512


def point_mlp_packed_floats(cout: int, cin: int) -> int:
    """Floats of the packed image of one layer's weight [cout, cin] (include/slu.h, slu_point_mlp)."""
    return (cout // 32) * ((cin + 15) // 16) * 8 * 64


def _point_mlp_chain(fn: str, c0: int, widths) -> None:
    if not 1 <= len(widths) <= POINT_MLP_MAX_LAYERS:
        raise RuntimeError(f"{fn}: 1..{POINT_MLP_MAX_LAYERS} layers supported, got {len(widths)}")
    if not 1 <= c0 <= POINT_MLP_MAX_C0:
        raise RuntimeError(f"{fn}: 1..{POINT_MLP_MAX_C0} input channels supported, got {c0}")
    if any(w < 32 or w % 32 or w > POINT_MLP_MAX_WIDTH for w in widths):
        raise RuntimeError(f"{fn}: every layer width must be a multiple of 32 and at most {POINT_MLP_MAX_WIDTH}, got {tuple(widths)}")


def pack_point_mlp(weights: Sequence[torch.Tensor]) -> torch.Tensor:
    """The 1x1 weights [C_l, C_{l-1}] (or [C_l, C_{l-1}, 1, 1]) of a chain of 1..4 layers -> the MFMA A-fragment images slu_point_mlp streams, one
    after the other (re-run after every weight update)."""
    ws = []
    for i, w in enumerate(weights):
        _req(w, f"weights[{i}]")
        if w.dim() == 4 and tuple(w.shape[2:]) == (1, 1):
            w = w.view(w.shape[0], w.shape[1])
        if w.dim() != 2 or w.numel() == 0:
            raise RuntimeError(f"weights[{i}]: expected [Cout, Cin] or [Cout, Cin, 1, 1], got {tuple(w.shape)}")
        if ws and w.shape[1] != ws[-1].shape[0]:
            raise RuntimeError(f"weights[{i}]: {w.shape[1]} input channels do not follow the {ws[-1].shape[0]} outputs of the layer before")
        ws.append(w)
    if not ws:
        raise RuntimeError("pack_point_mlp: 1..4 layers supported, got 0")
    _point_mlp_chain("pack_point_mlp", ws[0].shape[1], [w.shape[0] for w in ws])
    sizes = [point_mlp_packed_floats(w.shape[0], w.shape[1]) for w in ws]
    out = torch.empty(sum(sizes), dtype=torch.float32, device=ws[0].device)
    lib, at = _lib.load(), 0
    for w, sz in zip(ws, sizes):
        check(lib.slu_point_mlp_pack(w.data_ptr(), w.shape[0], w.shape[1], out.data_ptr() + 4 * at, _stream()), "slu_point_mlp_pack")
        at += sz
    return out


def point_mlp(x: torch.Tensor, packed: torch.Tensor, biases, widths: Sequence[int], slope: float, act_last: bool = True) -> torch.Tensor:
    """y = act(W_L ... act(W_1 x + b_1) ... + b_L) per pixel in one launch (slu_point_mlp): x [N, C0 <= 32, H, W] -> [N, widths[-1], H, W],
    packed = pack_point_mlp(weights), biases the L bias vectors (a sequence, or one tensor holding them one after the other),
    act(v) = v > 0 ? v : slope v, on the last layer only with act_last.  The intermediate maps stay on chip.  Every product is the exact-fp32 MFMA
    under every conv precision; bit-identical run to run."""
    _req(x, "x")
    if x.dim() != 4 or x.numel() == 0:
        raise RuntimeError(f"x: expected a non-empty [N, C0, H, W] tensor, got {tuple(x.shape)}")
    widths = [int(w) for w in widths]
    n, c0, h, w = x.shape
    _point_mlp_chain("point_mlp", c0, widths)
    if not isinstance(biases, torch.Tensor):
        for i, b in enumerate(biases):
            _req(b, f"biases[{i}]")
        if [b.numel() for b in biases] != widths:
            raise RuntimeError(f"biases: expected vectors of {widths} elements, got {[b.numel() for b in biases]}")
        biases = torch.cat([b.reshape(-1) for b in biases])
    _req(biases, "biases")
    if biases.numel() != sum(widths):
        raise RuntimeError(f"biases: expected {sum(widths)} elements (the widths {widths}), got {biases.numel()}")
    _req(packed, "packed")
    want = sum(point_mlp_packed_floats(co, ci) for co, ci in zip(widths, [c0] + widths[:-1]))
    if packed.numel() != want:
        raise RuntimeError(f"packed: {packed.numel()} floats does not match C0={c0} widths={widths} ({want})")
    if n > 65535 or h * w >= 2 ** 31 - 1:
        raise _lib.SluError(f"slu_point_mlp: {_lib.load().slu_strerror(-2).decode()} (code -2): N={n} H*W={h * w}")
    out = torch.empty((n, widths[-1], h, w), dtype=torch.float32, device=x.device)
    arr = (C.c_int * len(widths))(*widths)
    check(_lib.load().slu_point_mlp(x.data_ptr(), packed.data_ptr(), biases.data_ptr(), arr, len(widths), n, c0, h * w, float(slope),
                                    1 if act_last else 0, out.data_ptr(), _stream()), "slu_point_mlp")
    return out
