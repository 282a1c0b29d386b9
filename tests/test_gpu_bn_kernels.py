"""GPU: the per-channel training kernels of csrc/backward.hip -- bn_stats / bn_bwd_reduce (chan_reduce_kernel), bn_apply_fwd,
bn_act_bwd, act_affine_bwd -- against torch fp64 on the CPU, at launch shapes that give gx = cap((N HW + 8191) / 8192, 64) = 1 ... 64
workgroups per channel (fp64 atomics from many workgroups, the last-workgroup ticket of dbias, workgroup 0 publishing mean / invstd /
running statistics), on both the 16-byte (VEC = 4) and the scalar (VEC = 1: HW % 4 != 0, or a misaligned view) paths.

Bars (u = 2^-24, one fp32 rounding):
  sums of fp32 values accumulated in fp64 (bn_stats, sum dz)         1e-12 sum|terms|
  sums of fp32 products (bn_bwd_reduce's sum dz xhat)                4u sum|terms|
  mean / invstd / running statistics (fp64 math, rounded once)        2u |ref|
  z = a y + b [+ r], da = (k1 dz + k2 + k3 y) leaky'(y)               4u (|a y| + |b| + |r|), 4u (|k1 dz| + |k2| + |k3 y|) |leaky'|
  dgamma / dbeta (the fp64 sums rounded once)                         exact
  dbias against the fp64 sum of the kernel's OWN da                   u |sum| + 1e-9 sum|da|  (a lost workgroup: ~ sum|da| / gx)"""
import pytest
import torch

from semanticlidarunc_amd import ops

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _gx(n, hw):
    return min(max((n * hw + 8191) // 8192, 1), 64)


# (N, C, H, W, misaligned view): gx from 1 to the cap of 64 (and past it), C in {1, 40, 256}, both VEC paths
SHAPES = [
    (3, 40, 6, 66, False),          # gx = 1, VEC = 4
    (2, 256, 16, 260, False),       # gx = 2
    (5, 40, 13, 777, False),        # gx = 7, HW odd: VEC = 1
    (3, 1, 61, 999, False),         # gx = 23, HW odd
    (2, 40, 64, 1024, True),        # gx = 16, HW % 4 == 0 but a view 4 bytes off: VEC = 1
    (4, 40, 64, 2048, False),       # gx = 64: the training step's full-resolution layers
    (4, 1, 64, 2047, True),         # gx = 64, VEC = 1
    (5, 1, 64, 2048, False),        # N HW / 8192 = 80: capped at 64
]


def _dev(t, dev, misaligned):
    """t on the device; misaligned: as a view one float past a 16-byte boundary."""
    if not misaligned:
        return t.to(dev).contiguous()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _rows(t):
    return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)


def _close(got, want, bar, what):
    err = (got.double().cpu() - want).abs()
    bad = err > bar
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements over the bar, worst excess {float((err - bar).max()):.3e}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}x{s[3]}{'-view' if s[4] else ''}-gx{_gx(s[0], s[2] * s[3])}")
def test_channel_kernels_against_fp64(cuda, shape):
    n, c, h, w, mis = shape
    g = torch.Generator().manual_seed(n * 1000 + c + h + w)
    y = torch.randn(n, c, h, w, generator=g) * 2.0 + 0.5
    dz = torch.randn(n, c, h, w, generator=g)
    r = torch.randn(n, c, h, w, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    rm0, rv0 = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    yd, dzd, rd = _dev(y, cuda, mis), _dev(dz, cuda, mis), _dev(r, cuda, mis)
    y64, dz64, r64 = y.double(), dz.double(), r.double()
    m = n * h * w
    eps, mom = 1e-5, float(torch.tensor(0.1, dtype=torch.float32))      # the kernels take eps / momentum as fp32

    # ---- batch statistics ----
    s, q = ops.bn_stats(yd)
    _close(s, y64.sum((0, 2, 3)), 1e-12 * _rows(y64.abs()).sum(1), "bn_stats sum")
    _close(q, (y64 ** 2).sum((0, 2, 3)), 1e-12 * _rows(y64 ** 2).sum(1), "bn_stats sumsq")
    s64, q64 = y64.sum((0, 2, 3)), (y64 ** 2).sum((0, 2, 3))

    # ---- BatchNorm apply (train: from the sums, eval: from the running statistics), with and without a residual ----
    mu64 = s64 / m
    var64 = (q64 / m - mu64 ** 2).clamp_min(0)
    live = []
    for train in (True, False):
        for resid in (None, rd):
            rm, rv = rm0.clone().to(cuda), rv0.clone().to(cuda)
            sums = (s64.to(cuda), q64.to(cuda)) if train else None
            z, mean, invstd = ops.bn_apply_fwd(yd, sums, float(m), gamma.to(cuda), beta.to(cuda), eps, mom, rm, rv, train, resid=resid)
            live.append((train, resid is not None, z, mean, invstd, rm, rv))
    for train, has_r, z, mean, invstd, rm, rv in live:
        mu, var = (mu64, var64) if train else (rm0.double(), rv0.double())
        is64 = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
        a64, b64 = gamma.double() * is64, beta.double() - mu * gamma.double() * is64
        want = y64 * a64[None, :, None, None] + b64[None, :, None, None] + (r64 if has_r else 0.0)
        bar = 4 * U * ((y64 * a64[None, :, None, None]).abs() + b64.abs()[None, :, None, None] + (r64.abs() if has_r else 0.0))
        _close(z, want, bar, f"bn_apply_fwd z train={train} resid={has_r}")
        _close(mean, mu, 2 * U * mu.abs(), "bn_apply_fwd mean")
        _close(invstd, is64, 2 * U * is64, "bn_apply_fwd invstd")
        if train:
            want_rm = (1 - mom) * rm0.double() + mom * mu64
            want_rv = (1 - mom) * rv0.double() + mom * var64 * m / (m - 1)     # unbiased variance into the running estimate
            _close(rm, want_rm, 2 * U * want_rm.abs() + 1e-12, "running_mean")
            _close(rv, want_rv, 2 * U * want_rv.abs(), "running_var")
        else:
            assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)

    # ---- BatchNorm backward reduction ----
    mean32, invstd32 = mu64.float(), (1.0 / torch.sqrt(var64 + float(torch.tensor(eps, dtype=torch.float32)))).float()
    s1, s2 = ops.bn_bwd_reduce(dzd, yd, mean32.to(cuda), invstd32.to(cuda))
    xh = (y64 - mean32.double()[None, :, None, None]) * invstd32.double()[None, :, None, None]
    _close(s1, dz64.sum((0, 2, 3)), 1e-12 * _rows(dz64.abs()).sum(1), "bn_bwd_reduce sum dz")
    _close(s2, (dz64 * xh).sum((0, 2, 3)), 4 * U * _rows((dz64 * xh).abs()).sum(1), "bn_bwd_reduce sum dz xhat")
    s1_64, s2_64 = dz64.sum((0, 2, 3)), (dz64 * xh).sum((0, 2, 3))

    # ---- fused BatchNorm + LeakyReLU backward: every flag combination, all launched before any is checked ----
    runs = []
    for has_bn in (True, False):
        for train in ((True, False) if has_bn else (False,)):
            for slope in (0.01, None):
                for with_y in (True, False):
                    if not with_y and (slope is not None or (has_bn and train)):
                        continue                 # y is needed there
                    for want_dbias in (True, False):
                        args = (s1_64.to(cuda), s2_64.to(cuda), float(m), gamma.to(cuda), mean32.to(cuda), invstd32.to(cuda)) if has_bn else ()
                        kw = dict(train=train, slope=slope, want_dbias=want_dbias)
                        out = ops.bn_act_bwd(dzd, yd if with_y else None, *args, **kw) if has_bn else ops.bn_act_bwd(dzd, yd if with_y else None, **kw)
                        runs.append((has_bn, train, slope, with_y, want_dbias, out))
    for has_bn, train, slope, with_y, want_dbias, (da, dbias, dgamma, dbeta) in runs:
        what = f"bn_act_bwd bn={has_bn} train={train} slope={slope} y={with_y} dbias={want_dbias}"
        if has_bn:
            gm, is_ = gamma.double(), invstd32.double()
            k1 = (gm * is_).float().double()
            k3 = (-gm * is_ * is_ * s2_64 / m if train else torch.zeros(c, dtype=torch.float64))
            k2 = (-gm * is_ * s1_64 / m - k3 * mean32.double()).float().double() if train else torch.zeros(c, dtype=torch.float64)
            k3 = k3.float().double()
        else:
            k1, k2, k3 = torch.ones(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
        yy = y64 if with_y else torch.zeros_like(y64)
        t1, t2, t3 = k1[None, :, None, None] * dz64, k2[None, :, None, None].expand_as(dz64), k3[None, :, None, None] * yy
        fac = torch.where(yy > 0, 1.0, slope).double() if slope is not None else torch.ones_like(y64)
        _close(da, (t1 + t2 + t3) * fac, 4 * U * (t1.abs() + t2.abs() + t3.abs()) * fac, what + " da")
        if want_dbias:
            own = _rows(da.double().cpu())
            _close(dbias, own.sum(1), U * own.sum(1).abs() + 1e-9 * own.abs().sum(1), what + " dbias")
        else:
            assert dbias is None
        if has_bn:
            assert torch.equal(dgamma.cpu(), s2_64.float()) and torch.equal(dbeta.cpu(), s1_64.float()), what
        else:
            assert dgamma is None and dbeta is None

    # ---- act_affine_bwd: explicit coefficients ----
    k1, k2, k3 = torch.randn(c, generator=g), torch.randn(c, generator=g), torch.randn(c, generator=g)
    runs = []
    for slope in (0.01, None):
        for coeffs in ((k1, k2, k3), (k1, None, None), (None, None, None)):
            for want_dbias in (True, False):
                dk = [None if k is None else k.to(cuda) for k in coeffs]
                runs.append((slope, coeffs, want_dbias, ops.act_affine_bwd(dzd, yd, *dk, slope=slope, want_dbias=want_dbias)))
    for slope, coeffs, want_dbias, (da, db) in runs:
        what = f"act_affine_bwd slope={slope} k={[k is not None for k in coeffs]} dbias={want_dbias}"
        c1, c2, c3 = [(torch.full((c,), dflt) if k is None else k).double()[None, :, None, None] for k, dflt in zip(coeffs, (1.0, 0.0, 0.0))]
        t1, t2, t3 = c1 * dz64, c2.expand_as(dz64), c3 * y64
        fac = torch.where(y64 > 0, 1.0, slope).double() if slope is not None else torch.ones_like(y64)
        _close(da, (t1 + t2 + t3) * fac, 4 * U * (t1.abs() + t2.abs() + t3.abs()) * fac, what + " da")
        if want_dbias:
            own = _rows(da.double().cpu())
            _close(db, own.sum(1), U * own.sum(1).abs() + 1e-9 * own.abs().sum(1), what + " dbias")
        else:
            assert db is None
