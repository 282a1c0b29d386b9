"""GPU: one real SalsaNext training step, recorded node by node, every project autograd node checked against float64.

test_gpu_backward.py checks the weight- and data-gradient kernels tightly, but only at toy sizes, where the launchers build grids unlike
the training step's (one pixel run per wave instead of ~16, other LDS-reduce + atomic flush counts); at full size its only check is
whole-network and loose.  Here the step of tools/train_bench.py runs as the bench runs it: seeded_model(SalsaNext), synthetic_scan, a
plain model(x) (the dropout kernel draws the multipliers), salsanext_loss, AdamW.  One whole step including opt.step(), then the SECOND
step's backward is recorded: arena slices reused, weights repacked after the in-place update, BatchNorm momentum as in the bench.  A
prehook on every ConvLayerFn / AvgPoolFn / loss node clones the gradient the node receives and its saved tensors, a hook clones what
it produces; the clones stay on the GPU and are converted node by node.

Reference per ConvLayerFn node, from its saved state, in float64 with torch's own ops on the GPU (faster than the CPU: 0.17 s against
~1.7 s for one 32->32 3x3 layer at 4x64x2048) and never with a project kernel: train-mode F.batch_norm backward of the saved y with dz,
times leaky'(y) from the sign of the saved y, gives da; dbias = sum da; dW and every dsrc from autograd of conv2d over the sources
rebuilt as the forward reads them (stored tensor x multiplier, PixelShuffle, concat).  d_resid must be dz exactly.  The saved mean and
invstd are checked against float64 statistics of y (the conv kernel's fused statistics at full size).  AvgPool: float64 backward of
oracle.salsanext.avgpool3s2.  Loss: dlogits against autograd of the float64 oracle loss, with the tie allowance of
test_gpu_loss.test_lovasz_training_size_against_oracle (equal Lovasz errors sort either way).

Every check is per element, |got - fp64| <= bar * magnitude, the magnitude being what the operation sums:
  |da|    |gamma| invstd (|dz| + |mean dz| + |xhat| |mean(dz xhat)|) leaky'(y)    (the BatchNorm backward's terms)
  dW      the float64 weight gradient of |X| and |da|        dsrc   the float64 data gradient of |W| and |da|
  dbias   sum |da|       dgamma  sum |dz xhat|      dbeta  sum |dz|       avgpool dx  the same pool backward of |dy|
  mean    |mean| + std   invstd  invstd
Bars: BARS below, 4x to 8x the measured maxima and far inside the small-shape bars they extend (1e-4 for weight and data gradients,
2e-4 for the node's other outputs).  Measured maxima of error / magnitude on MI355X over all nodes of a kind, worst of two runs:
                  bar     fp32 4x64x2048   f16x3 4x64x2048   fp32 3x48x1040
  dW nchw kxk     1e-6    1.6e-7           1.4e-7            1.6e-7          wgradk_nchw_kernel
  dW nchw 1x1     1e-6    2.4e-7           2.0e-7            1.0e-7          wgrad1x1_nchw_kernel
  dW cl kxk       2e-6    -                -                 4.2e-7          wgrad_kernel (W % 16 != 0; W = 65 odd)
  dW cl 1x1       1e-6    -                -                 2.3e-7          wgrad1x1_kernel (H W % 32 != 0; odd pixel count)
  dsrc            4e-6    1.0e-6           8.6e-7            7.3e-7          data-gradient conv + view / split_grad
  dbias           2e-7    2.9e-8           3.4e-8            3.5e-8
  dgamma          1e-7    1.1e-8           1.3e-8            2.0e-8
  dbeta           5e-8    5.8e-9           6.2e-9            8.5e-9
  mean            2e-7    4.0e-8           3.7e-8            4.0e-8          fused conv statistics (fp32), bn_stats (f16x3)
  invstd          4e-7    8.0e-8           5.9e-8            9.1e-8
  avgpool dx      1e-6    2.1e-7           2.1e-7            2.0e-7
  dlogits: fraction of the elements beyond 1e-4 of max|dlogits| 9.7e-4 / 9.8e-4 / 3.3e-7 (LOSS_TIE_FRACTION 4e-3), worst 4.1e-4 /
  4.1e-4 / 1.1e-4 of max|dlogits| (LOSS_MAX 2e-3); max|dlogits| is 1.9e-6 at 4x64x2048, so 1e-4 of it is 1.9e-10.

Sensitivity, asserted on every run: for each weight-gradient node the float64 contribution of ONE work unit of the kernel that ran
(wgradk_nchw_kernel: a run of 4 units of 16 pixels, 64 pixels of a row at W = 2048; wgrad_kernel / wgrad1x1_kernel: a run of 64
consecutive pixels of the flattened batch; wgrad1x1_nchw_kernel: one unit of 32 pixels) must move at least one dW element by more than
4x its bar, and one 16-pixel row segment must move one dgamma by more than 4x its bar: a wave that drops a unit fails this test.
Measured minima over the nodes, in bars: wgradk_nchw_kernel 135, wgrad1x1_nchw_kernel 89, wgrad_kernel 1.3e3, wgrad1x1_kernel 2.6e4,
dgamma 201.

Chain consistency, no rounding model: every param.grad equals bit for bit the gradient its node produced, and the dz a node receives
equals the sum of what its consumers produced (bit for bit with one or two consumers, within the fp32 sum's rounding with more): an
aliased dcat view or an arena slice overwritten after it was produced fails here.

Configurations: BASELINE configs[1] (B = 4, 64x2048) with exact-fp32 and split-fp16 (f16x3) forward products, and a ragged fp32 step
(B = 3, 48x1040: lowest level 3x65, so the channel-last weight-gradient kernels run at odd W and an odd pixel count, and at W / 2 ... W / 8
where W % 16 != 0 and H W % 32 != 0).  test_backward_path_coverage spies on the weight-gradient and split entry points and names any
backward path of ConvLayerFn that none of the recorded nodes took."""
import collections

import pytest
import torch
import torch.nn.functional as F

from oracle import losses as olosses
from oracle import salsanext as osalsa
from semanticlidarunc_amd import ops
from semanticlidarunc_amd import salsanext as sn
from semanticlidarunc_amd.loss import salsanext_loss
from semanticlidarunc_amd.salsanext import SalsaNext
from semanticlidarunc_amd.testing import seeded_model, synthetic_scan

pytestmark = pytest.mark.gpu

# name -> (batch, H, W, training conv precision)
CONFIGS = {
    "b4_64x2048_fp32": (4, 64, 2048, "fp32"),
    "b4_64x2048_f16x3": (4, 64, 2048, "f16x3"),
    "b3_48x1040_fp32": (3, 48, 1040, "fp32"),
}
# per element: |got - fp64| <= bar * magnitude (module docstring)
BARS = {
    "dW nchw kxk": 1e-6, "dW nchw 1x1": 1e-6, "dW cl kxk": 2e-6, "dW cl 1x1": 1e-6, "dsrc": 4e-6,
    "dbias": 2e-7, "dgamma": 1e-7, "dbeta": 5e-8, "mean": 2e-7, "invstd": 4e-7, "avgpool dx": 1e-6,
}
# loss node: |dlogits - fp64| <= LOSS_BAR * max|fp64| except on a fraction < LOSS_TIE_FRACTION of the elements (Lovasz errors that sort
# in another order in fp32 and in fp64), and <= LOSS_MAX * max|fp64| everywhere
LOSS_BAR, LOSS_TIE_FRACTION, LOSS_MAX = 1e-4, 4e-3, 2e-3
U32 = 2.0 ** -24
_TINY = 1e-30
_PATHS = {}          # config -> Counter of the backward paths its recorded nodes took (test_backward_path_coverage)


def _kind(node):
    return type(node).__name__


_PROJECT = ("ConvLayerFnBackward", "AvgPoolFnBackward", "SalsaNextLossFnBackward")


def _walk(root):
    """Every node reachable from root (references held, so ids stay unique)."""
    seen, order, stack = set(), [], [root]
    while stack:
        n = stack.pop()
        if n is None or id(n) in seen:
            continue
        seen.add(id(n))
        order.append(n)
        stack.extend(f for f, _ in n.next_functions)
    return order


def _conv_inputs(r):
    """Names of the tensor inputs of a recorded ConvLayerFn node, in the order of its next_functions / the hook's grad_inputs."""
    node = r["node"]
    names = ["weight"] + (["bias"] if node.has_bias else []) + (["gamma", "beta"] if node.has_bn else [])
    names += (["resid"] if node.has_resid else []) + [f"src{i}" for i in range(len(node.src_shapes))]
    assert len(names) == len(r["next"]) == len(r["grads"]), (names, len(r["next"]), len(r["grads"]))
    return names


class _Recorder:
    """Hooks on the project nodes and spies on the backward's entry points (ops.* are looked up at call time by autograd.py)."""

    SPIED = ("conv2d_wgrad_nchw", "conv1x1_wgrad_nchw", "conv2d_wgrad", "split_grad")

    def __init__(self, nodes):
        self.rec, self.cur, self.orig = {}, [None], {}
        for n in nodes:
            if _kind(n) in _PROJECT:
                # the edges, read now: a node's next_functions cannot be read once backward has freed the graph
                nxt = [(None, None) if f is None else (f, f.variable if _kind(f) == "AccumulateGrad" else None) for f, _ in n.next_functions]
                self.rec[id(n)] = {"node": n, "kind": _kind(n), "calls": [], "next": nxt}
                n.register_prehook(self._pre(n))
                n.register_hook(self._post(n))

    def _pre(self, node):
        def fn(grad_outputs):
            r = self.rec[id(node)]
            self.cur[0] = r
            r["dz"] = [None if g is None else g.detach().clone() for g in grad_outputs]
            if r["kind"] == "ConvLayerFnBackward":
                r["saved"] = [t.detach().clone() for t in node.saved_tensors]
            elif r["kind"] == "AvgPoolFnBackward":
                r["scale"] = node.saved_tensors[0].detach().clone() if node.has_scale else None
        return fn

    def _post(self, node):
        def fn(grad_inputs, grad_outputs):
            r = self.rec[id(node)]
            r["grads"] = [None if g is None else g.detach().clone() for g in grad_inputs]
            r["views"] = [g is not None and g._is_view() for g in grad_inputs]
            self.cur[0] = None
        return fn

    def _spy(self, name):
        f = self.orig[name]

        def spy(*a, **k):
            out = f(*a, **k)
            r = self.cur[0]
            assert r is not None, f"ops.{name} called outside a recorded node"
            r["calls"].append((name, out is not None, a))
            return out
        return spy

    def __enter__(self):
        for name in self.SPIED:
            self.orig[name] = getattr(ops, name)
            setattr(ops, name, self._spy(name))
        return self

    def __exit__(self, *exc):
        for name, f in self.orig.items():
            setattr(ops, name, f)


def _wgrad_path(r):
    """Which weight-gradient kernel produced the node's dW."""
    cfg = r["node"].cfg
    for name, took, _ in r["calls"]:
        if name == "conv2d_wgrad_nchw" and took:
            return "dW nchw kxk"
        if name == "conv1x1_wgrad_nchw" and took:
            return "dW nchw 1x1"
        if name == "conv2d_wgrad":
            return "dW cl 1x1" if cfg.ksize == 1 else "dW cl kxk"
    raise AssertionError(f"no weight-gradient entry point ran for a node: {r['calls']}")


def _path_names(r, path):
    """The backward paths of ConvLayerFn one node took (test_backward_path_coverage)."""
    node, cfg = r["node"], r["node"].cfg
    out = {path}
    if path == "dW nchw kxk":
        out.add(f"dW nchw kxk {(cfg.ksize, cfg.dil, cfg.pad)}")
        if any(cfg.shuffles) and any(s is not None for s in cfg.scales):
            out.add("dW nchw kxk PixelShuffle + multiplier sources")
    if path == "dW nchw 1x1":
        out.add("dW nchw 1x1 one source" if len(node.src_shapes) == 1 else "dW nchw 1x1 concatenated sources")
    names = _conv_inputs(r)
    if any(v for n, v in zip(names, r["views"]) if n.startswith("src")):
        out.add("dsrc as a view of dcat")
    if any(name == "split_grad" for name, _, _ in r["calls"]):
        out.add("dsrc through split_grad")
    out.add("with BatchNorm" if node.has_bn else "without BatchNorm")
    if node.has_resid:
        out.add("with residual")
    return out


def _rebuild(ts, cfg):
    """The conv input as the forward reads it: stored tensor x multiplier, PixelShuffle, concat (osalsa.fused_conv)."""
    parts = []
    for t, sc, ps in zip(ts, cfg.scales, cfg.shuffles):
        if sc is not None:
            t = t * sc.double()[:, :, None, None]
        if ps:
            t = F.pixel_shuffle(t, 2)
        parts.append(t)
    return torch.cat(parts, 1) if len(parts) > 1 else parts[0]


def _err(got, ref, mag):
    return float(((got.double() - ref).abs() / (mag + _TINY)).max())


def _unit_pixels(path, n, h, w):
    """(image, row, column) index tensors of one work unit of the weight-gradient kernel that ran, near the middle of the last image."""
    hw = h * w
    if path == "dW nchw kxk":                    # wgradk_nchw_kernel: units of 16 pixels of a row, runs of 4 consecutive units
        upr = w // 16
        u = ((n - 1) * h + h // 2) * upr + (w // 2) // 16
        units = torch.arange(u // 4 * 4, min(u // 4 * 4 + 4, n * h * upr))
        flat = ((units // upr) * w + (units % upr) * 16)[:, None] + torch.arange(16)[None, :]
        flat = flat.reshape(-1)                  # (n h + y) w + x
    elif path == "dW nchw 1x1":                  # wgrad1x1_nchw_kernel: units of 32 pixels of one image's H W
        start = (n - 1) * hw + (hw // 2) // 32 * 32
        flat = torch.arange(start, start + 32)
    else:                                        # wgrad_kernel / wgrad1x1_kernel: runs of 32 pixel pairs of the flattened batch
        start = ((n - 1) * hw + hw // 2) // 64 * 64
        flat = torch.arange(start, min(start + 64, n * hw))
    return flat // hw, (flat % hw) // w, flat % w


def _unit_dw(da, xin, cfg, pix):
    """float64 contribution of the unit's pixels to dW: sum over the unit of da (x) the tap-shifted input, zero padded."""
    k, dil, pad = cfg.ksize, cfg.dil, cfg.pad
    xp = F.pad(xin, (pad, pad, pad, pad))
    ni, yi, xi = (t.to(da.device) for t in pix)
    a = da[ni, :, yi, xi]                                             # [P, Cout]
    out = torch.empty(da.shape[1], xin.shape[1], k, k, dtype=torch.float64, device=da.device)
    for ti in range(k):
        for tj in range(k):
            out[:, :, ti, tj] = a.t() @ xp[ni, :, yi + ti * dil, xi + tj * dil]
    return out


def _check_conv_node(r, errs, sens, failures):
    node, cfg = r["node"], r["node"].cfg
    names = _conv_inputs(r)
    grads = dict(zip(names, r["grads"]))
    nsrc = len(node.src_shapes)
    saved = r["saved"]
    w32, y32, srcs = saved[0], saved[1], saved[2:2 + nsrc]
    dz32 = r["dz"][0].contiguous().float()
    dz, y = dz32.double(), y32.double()
    n, c, h, w = y.shape
    tag = f"{cfg.ksize}x{cfg.ksize} d{cfg.dil} {tuple(w32.shape[:2])} at {n}x{h}x{w}"

    def bar(kind, e):
        errs[kind] = max(errs.get(kind, 0.0), e)
        if e > BARS[kind]:
            failures.append(f"{kind} {tag}: {e:.3g} > {BARS[kind]:.3g}")

    if node.has_bn:
        gamma32, mean32, invstd32 = saved[2 + nsrc:5 + nsrc]
        eps = cfg.bn.eps
        yl = y.clone().requires_grad_(True)
        g64 = gamma32.double().requires_grad_(True)
        b64 = torch.zeros_like(g64).requires_grad_(True)
        F.batch_norm(yl, None, None, g64, b64, True, 0.0, eps).backward(dz)
        dy = yl.grad
        m64 = y.mean((0, 2, 3))
        var64 = y.var((0, 2, 3), unbiased=False)
        inv64 = (var64 + eps).rsqrt()
        bar("mean", float(((mean32.double() - m64).abs() / (m64.abs() + var64.sqrt())).max()))
        bar("invstd", float(((invstd32.double() - inv64).abs() / inv64).max()))
        xhat = (y - m64[:, None, None]) * inv64[:, None, None]
        dzx = dz * xhat
        mag_dy = (g64.detach().abs() * inv64)[:, None, None] * (dz.abs() + dz.mean((0, 2, 3)).abs()[:, None, None]
                                                                 + xhat.abs() * dzx.mean((0, 2, 3)).abs()[:, None, None])
        mag_dgamma, mag_dbeta = dzx.abs().sum((0, 2, 3)), dz.abs().sum((0, 2, 3))
        bar("dgamma", _err(grads["gamma"], g64.grad, mag_dgamma))
        bar("dbeta", _err(grads["beta"], b64.grad, mag_dbeta))
        # one 16-pixel row segment of dz xhat must move some dgamma by more than 4 x its bar
        seg = dzx[n - 1, :, h // 2, (w // 2) // 16 * 16:(w // 2) // 16 * 16 + 16].sum(-1)
        s = float((seg.abs() / (mag_dgamma + _TINY)).max()) / BARS["dgamma"]
        sens["dgamma"] = min(sens.get("dgamma", float("inf")), s)
        if s <= 4.0:
            failures.append(f"dgamma {tag}: a 16-pixel segment moves it by only {s:.3g} x its bar")
        del yl, dzx, xhat
    else:
        dy, mag_dy = dz, dz.abs()
    if cfg.slope is not None:
        lk = torch.where(y > 0, 1.0, float(cfg.slope)).to(torch.float64)
        da, mag_da = dy * lk, mag_dy * lk
    else:
        da, mag_da = dy, mag_dy
    del dy, mag_dy
    if node.has_resid and grads["resid"] is not None and not torch.equal(grads["resid"], dz32):
        failures.append(f"d_resid {tag}: not dz bit for bit")
    if grads.get("bias") is not None:
        bar("dbias", _err(grads["bias"], da.sum((0, 2, 3)), mag_da.sum((0, 2, 3))))
    # dW and dsrc: autograd of the float64 conv over the rebuilt sources; magnitudes from the same conv of |W|, |sources| and |da|
    leaves = [t.double().requires_grad_(True) for t in srcs]
    w64 = w32.double().requires_grad_(True)
    xin = _rebuild(leaves, cfg)
    F.conv2d(xin, w64, None, padding=cfg.pad, dilation=cfg.dil).backward(da)
    aleaves = [t.double().abs().requires_grad_(True) for t in srcs]
    aw = w32.double().abs().requires_grad_(True)
    F.conv2d(_rebuild(aleaves, cfg), aw, None, padding=cfg.pad, dilation=cfg.dil).backward(mag_da)
    path = _wgrad_path(r)
    bar(path, _err(grads["weight"], w64.grad, aw.grad))
    for i in range(nsrc):
        g = grads[f"src{i}"]
        if g is not None:
            bar("dsrc", _err(g, leaves[i].grad, aleaves[i].grad))
    # one work unit of the kernel that ran must move some dW element by more than 4 x its bar
    unit = _unit_dw(da, xin.detach(), cfg, _unit_pixels(path, n, h, w))
    s = float((unit.abs() / (aw.grad + _TINY)).max()) / BARS[path]
    sens[path] = min(sens.get(path, float("inf")), s)
    if s <= 4.0:
        failures.append(f"{path} {tag}: one work unit moves dW by only {s:.3g} x its bar")
    return path


def _check_pool_node(r, errs, failures):
    node = r["node"]
    dy = r["dz"][0].double()
    sc = None if r["scale"] is None else r["scale"].double()
    xl = torch.zeros(node.shape, dtype=torch.float64, device=dy.device, requires_grad=True)
    osalsa.avgpool3s2(xl, sc).backward(dy)
    xa = torch.zeros(node.shape, dtype=torch.float64, device=dy.device, requires_grad=True)
    osalsa.avgpool3s2(xa, None if sc is None else sc.abs()).backward(dy.abs())
    e = _err(r["grads"][0], xl.grad, xa.grad)
    errs["avgpool dx"] = max(errs.get("avgpool dx", 0.0), e)
    if e > BARS["avgpool dx"]:
        failures.append(f"avgpool dx {tuple(node.shape)}: {e:.3g} > {BARS['avgpool dx']:.3g}")


def _check_chain(rec, params, failures):
    """param.grad == the gradient its node produced, and every node's dz == the sum of what its consumers produced."""
    into = collections.defaultdict(list)
    for r in rec.values():
        for j, (f, p) in enumerate(r["next"]):
            if f is None:
                continue
            if id(f) in rec:
                into[id(f)].append(r["grads"][j])
            elif p is not None:
                if r["grads"][j] is None or p.grad is None or not torch.equal(p.grad, r["grads"][j]):
                    failures.append(f"param.grad of {params.get(id(p), '?')} differs from what its node produced")
    checked = 0
    for rid, gs in into.items():
        gs = [g for g in gs if g is not None]
        if not gs or rec[rid]["kind"] == "SalsaNextLossFnBackward":
            continue
        dz = rec[rid]["dz"][0]
        total = gs[0].clone()
        for g in gs[1:]:
            total += g
        checked += 1
        if len(gs) <= 2:
            if not torch.equal(total, dz):
                failures.append(f"dz of a {rec[rid]['kind']} is not the bit-exact sum of its {len(gs)} consumers' gradients")
        else:
            tol = (len(gs) - 1) * U32 * sum(g.abs().double() for g in gs)
            if bool(((total.double() - dz.double()).abs() > tol).any()):
                failures.append(f"dz of a {rec[rid]['kind']} differs from the sum of its {len(gs)} consumers' gradients")
    return checked


def _run_step(name, dev):
    b, h, w, prec = CONFIGS[name]
    sn.set_train_conv_precision(prec)
    try:
        model = seeded_model(SalsaNext).to(dev).train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
        x, y = synthetic_scan(b, h, w, seed=1234)
        x, y = x.to(dev), y.to(dev)
        torch.manual_seed(7)
        opt.zero_grad(set_to_none=True)
        salsanext_loss(model(x), y, 1.0, 1.0, 0)[0].backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        out = model(x)
        loss = salsanext_loss(out, y, 1.0, 1.0, 0)[0]
        nodes = _walk(loss.grad_fn)
        other = sorted({_kind(nd) for nd in nodes} - set(_PROJECT) - {"AccumulateGrad"})
        assert not other, f"nodes outside the project's autograd functions in the step's graph: {other}"
        rec = _Recorder(nodes)
        with rec:
            loss.backward()
        torch.cuda.synchronize()
        return model, out.detach(), y, rec.rec
    finally:
        sn.set_train_conv_precision("fp32")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_training_step_nodes_against_fp64(cuda, name):
    model, logits, labels, rec = _run_step(name, cuda)
    params = {id(p): k for k, p in model.named_parameters()}
    errs, sens, failures, paths = {}, {}, [], collections.Counter()
    kinds = collections.Counter(r["kind"] for r in rec.values())
    assert kinds["SalsaNextLossFnBackward"] == 1 and kinds["AvgPoolFnBackward"] == 4 and kinds["ConvLayerFnBackward"] == 51, kinds
    assert all("grads" in r for r in rec.values()), "a recorded node did not run"
    n_chain = _check_chain(rec, params, failures)
    for r in rec.values():
        if r["kind"] == "ConvLayerFnBackward":
            path = _check_conv_node(r, errs, sens, failures)
            paths.update(_path_names(r, path))
        elif r["kind"] == "AvgPoolFnBackward":
            _check_pool_node(r, errs, failures)
        else:
            lg = logits.double().requires_grad_(True)
            olosses.salsanext_loss(lg, labels)[0].backward()
            d = (r["grads"][0].double() - lg.grad).abs() / float(lg.grad.abs().max())
            frac, worst = float((d > LOSS_BAR).double().mean()), float(d.max())
            errs["loss dlogits (fraction beyond LOSS_BAR)"] = frac
            errs["loss dlogits (max)"] = worst
            errs["loss max|dlogits|"] = float(lg.grad.abs().max())
            if frac >= LOSS_TIE_FRACTION or worst > LOSS_MAX:
                failures.append(f"dlogits: {frac:.3g} of the elements beyond {LOSS_BAR} of scale, worst {worst:.3g}")
            del lg, d
        for k in ("saved", "dz"):
            r.pop(k, None)
        torch.cuda.empty_cache()
    _PATHS[name] = paths
    print(f"\n{name}: {n_chain} node inputs chain-checked; max error / magnitude:",
          {k: f"{v:.3g}" for k, v in sorted(errs.items())}, "\nsensitivity (unit's move / bar, min over nodes):",
          {k: f"{v:.3g}" for k, v in sorted(sens.items())})
    assert not failures, "\n".join(failures[:40])


REQUIRED_PATHS = (
    "dW nchw kxk (3, 1, 1)", "dW nchw kxk (3, 2, 2)", "dW nchw kxk (2, 2, 1)", "dW nchw kxk PixelShuffle + multiplier sources",
    "dW nchw 1x1 one source", "dW nchw 1x1 concatenated sources", "dW cl kxk", "dW cl 1x1",
    "dsrc as a view of dcat", "dsrc through split_grad", "without BatchNorm", "with residual",
)


def test_backward_path_coverage(cuda):
    """Across the recorded steps, every backward path of ConvLayerFn handled at least one checked node."""
    for name in CONFIGS:
        if name not in _PATHS:
            test_training_step_nodes_against_fp64(cuda, name)
    seen = collections.Counter()
    for c in _PATHS.values():
        seen.update(c)
    print("\nbackward paths (nodes over all configurations):", dict(sorted(seen.items())))
    missing = [p for p in REQUIRED_PATHS if not seen[p]]
    assert not missing, f"backward paths no recorded node took: {missing}"
