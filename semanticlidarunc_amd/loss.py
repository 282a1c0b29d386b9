"""Autograd glue for the loss kernels (one `torch.autograd.Function` per fused op).

Backward functions only read tensors saved in forward, so `torch.autograd.grad(..., retain_graph=True)`
can be called repeatedly on the same graph (the reference's GradNorm probes do, utils/grad_norm.py:52).
"""
from __future__ import annotations

import torch

from . import ops


def _labels(labels: torch.Tensor, device) -> torch.Tensor:
    return labels.to(device=device, dtype=torch.int64).contiguous()


class SoftmaxFn(torch.autograd.Function):
    """probs = softmax(logits, dim=1) on the HIP path."""

    @staticmethod
    def forward(ctx, logits):
        probs, _, _ = ops.softmax_entropy(logits.detach().float().contiguous())
        ctx.save_for_backward(probs)
        return probs

    @staticmethod
    def backward(ctx, g):
        (probs,) = ctx.saved_tensors
        return ops.softmax_loss_bwd(probs, None, g.float().contiguous(), 1.0, 0.0, 0.0, None)


class LovaszFn(torch.autograd.Function):
    """Lovasz-Softmax of probabilities; d loss / d probs is produced by the forward kernels."""

    @staticmethod
    def forward(ctx, probs, labels, ignore_index, classes="present"):
        need = probs.requires_grad
        loss, _, grad = ops.lovasz_fwd(probs.detach().float().contiguous(), _labels(labels, probs.device), ignore_index, need, classes)
        ctx.save_for_backward(grad if need else torch.empty(0, device=probs.device))
        ctx.need = need
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        if not ctx.need:
            return None, None, None, None
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None


class NllFn(torch.autograd.Function):
    """mean over counted pixels of the per-pixel NLL (kinds: ops.NLL_*)."""

    @staticmethod
    def forward(ctx, x, labels, kind, param, ignore_index):
        xd = x.detach().float().contiguous()
        lab = _labels(labels, x.device)
        acc, cnt = ops.nll_fwd(xd, lab, kind, param, ignore_index)
        ctx.save_for_backward(xd, lab, cnt)
        ctx.cfg = (kind, param, ignore_index)
        return (acc / cnt.to(torch.float64)).to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, g):
        xd, lab, cnt = ctx.saved_tensors
        kind, param, ignore_index = ctx.cfg
        gscale = (g.reshape(1).to(torch.float64) / cnt.to(torch.float64)).to(torch.float32)
        return ops.nll_bwd(xd, lab, kind, param, ignore_index, gscale), None, None, None, None


class SalsaNextLossFn(torch.autograd.Function):
    """w_nll * NLL(log clamp(softmax(z), 1e-8), y)  +  w_ls * Lovasz(softmax(z), y, ignore)   (trainer.py:508-516),
    softmax / NLL / Lovasz / backward fused over one read of the logits."""

    @staticmethod
    def forward(ctx, logits, labels, w_nll, w_ls, lovasz_ignore):
        z = logits.detach().float().contiguous()
        lab = _labels(labels, z.device)
        probs, nll_sum = ops.softmax_nll(z, lab, clamp=1e-8, want_probs=True)
        ls, _, grad_ls = ops.lovasz_fwd(probs, lab, lovasz_ignore, want_grad=True)
        n = lab.numel()
        nll = (nll_sum / n).to(torch.float32)
        ctx.save_for_backward(probs, lab, grad_ls)
        ctx.cfg = (float(w_nll), float(w_ls), n)
        total = (w_nll * nll + w_ls * ls).reshape(())
        nll, ls = nll.reshape(()), ls.reshape(())
        # the two terms are returned for logging only: the backward below is that of `total`, so differentiating through
        # either of them raises instead of silently returning zeros
        ctx.mark_non_differentiable(nll, ls)
        return total, nll, ls

    @staticmethod
    def backward(ctx, g, _g_nll, _g_ls):
        probs, lab, grad_ls = ctx.saved_tensors
        w_nll, w_ls, n = ctx.cfg
        gout = g.reshape(1).float().contiguous()
        return ops.softmax_loss_bwd(probs, lab, grad_ls, w_ls, w_nll / n, 1e-8, gout), None, None, None, None


def salsanext_loss(logits, labels, w_nll: float = 1.0, w_ls: float = 1.0, lovasz_ignore=0):
    """(loss, nll, lovasz) of the reference's "SalsaNext" loss branch; `loss` is differentiable w.r.t. logits, the two terms are
    values only (marked non-differentiable)."""
    return SalsaNextLossFn.apply(logits, labels, w_nll, w_ls, lovasz_ignore)


class TempNllFn(torch.autograd.Function):
    """(log_T, rows, row_labels, idx, denom, chunk_size) -> (loss_sum / denom, bad): the objective of temperature scaling
    (models/temp_scaling.py:145-151) with T = max(exp(log_T), 1e-3) read on the device; d / d log_T = g_sum / denom comes out of the
    same pass (ops.temp_nll), so the backward launches nothing.  At most `chunk_size` rows per launch, the chunks' fp64 sums added in
    chunk order.  loss is float64; bad (int64 [1], rows whose label is outside [0, C)) is not differentiable."""

    @staticmethod
    def forward(ctx, log_T, rows, row_labels, idx, denom, chunk_size):
        lt = log_T.detach().float().contiguous()
        n = rows.shape[0] if idx is None else idx.numel()
        step = n if not chunk_size or chunk_size <= 0 else int(chunk_size)
        loss = g = bad = None
        for i in range(0, n, step):
            j = min(i + step, n)
            if idx is None:
                part = ops.temp_nll(rows[i:j], row_labels[i:j], lt)
            else:
                part = ops.temp_nll(rows, row_labels, lt, idx[i:j])
            loss, g, bad = part if loss is None else (loss + part[0], g + part[1], bad + part[2])
        ctx.save_for_backward(g / float(denom))
        ctx.like = (log_T.shape, log_T.dtype)
        ctx.mark_non_differentiable(bad)
        return (loss / float(denom)).reshape(()), bad

    @staticmethod
    def backward(ctx, gout, _gbad):
        (g,) = ctx.saved_tensors
        shape, dtype = ctx.like
        return (g * gout.to(torch.float64)).to(dtype).reshape(shape), None, None, None, None, None


def temp_nll_loss(log_T, rows, row_labels, idx=None, denom=None, chunk_size=None):
    """(loss, bad) of TempNllFn; denom defaults to the number of rows evaluated."""
    if denom is None:
        denom = rows.shape[0] if idx is None else idx.numel()
    return TempNllFn.apply(log_T, rows, row_labels, idx, denom, chunk_size)
