"""Mirror of the reference's ``models.temp_scaling`` (src/models/temp_scaling.py:37-177): post-hoc temperature scaling.

Same two entry points, signatures, defaults, start-value rule, optimiser settings, JSON file and ``ValueError``s.  What differs is where
the data lives (DESIGN "Temperature scaling on the device"):

* ``cache_calib_logits`` keeps the cache on the GPU.  Each batch's valid pixels are turned into ``log p`` rows and appended by one
  fused pass (``ops.calib_rows``); the row count stays on the device and is read back once, after the last batch.
* ``calibrate_temperature_from_cache`` evaluates the objective and its derivative by ``log T`` in one streaming pass over the resident
  cache (``ops.temp_nll`` behind ``loss.TempNllFn``) instead of re-uploading it in chunks for every optimiser evaluation; the stock
  ``torch.optim.LBFGS`` / ``Adam`` drive it unchanged.
"""
from __future__ import annotations

import json
import os

import torch

from semanticlidarunc_amd import ops
from semanticlidarunc_amd.loss import temp_nll_loss
from semanticlidarunc_amd.models.losses import classify_output_kind
from semanticlidarunc_amd.utils.mc_dropout import _stacked_passes, set_dropout_mode

EPS = 1e-12


def _progress(iterable, desc):
    try:
        import tqdm
    except ImportError:
        return iterable
    return tqdm.tqdm(iterable, desc=desc)


def _output_kind(model, out, kind_cache):
    """'logits' | 'probs' | 'log_probs', detected once per model instance."""
    if kind_cache is None:
        return classify_output_kind(out, class_dim=1)
    kind = kind_cache.get(id(model))
    if kind is None:
        kind = kind_cache[id(model)] = classify_output_kind(out, class_dim=1)
    return kind


def _to_probs(out, kind):
    if kind == "logits":
        return ops.softmax_entropy(out.float().contiguous())[0]
    if kind == "probs":
        return out
    if kind == "log_probs":
        return out.exp()
    raise ValueError(f"Unknown output kind: {kind}")


@torch.no_grad()
def _forward_to_probs(model: torch.nn.Module, inputs, kind_cache: dict | None = None):
    """(probabilities [B,C,H,W], output kind) of one forward; the kind is detected once per model when a cache is given."""
    out = model(*inputs)
    kind = _output_kind(model, out, kind_cache)
    return _to_probs(out, kind), kind


def _mc_mean_probs(model, inputs, mc_samples, kind_cache):
    """Mean over `mc_samples` stochastic passes of the probability maps; the passes are stacked along the batch axis
    (utils.mc_dropout), dropout is already switched on by the caller."""
    total = None
    for group in _stacked_passes(model, inputs, int(mc_samples)):             # [t,B,C,H,W]
        t, b = group.shape[:2]
        flat = group.reshape(t * b, *group.shape[2:])
        kind = _output_kind(model, flat, kind_cache)
        part = _to_probs(flat, kind).reshape(group.shape).sum(dim=0)
        total = part if total is None else total + part
    return total / float(mc_samples)


class _RowCache:
    """rows fp32 [cap, C] / labels int64 [cap] on the device with the row count next to them.  The host only knows an upper bound of
    the count (every pixel so far valid) and grows the buffers by it, so appending never waits for the device."""

    def __init__(self):
        self.rows = self.labels = self.count = None
        self.bound = 0                                     # rows the cache holds at most

    def append(self, out, kind, labels, ignore_index):
        b, c, h, w = out.shape
        need = self.bound + b * h * w
        if self.rows is None or need > self.rows.shape[0]:
            cap = need if self.rows is None else max(need, 2 * self.rows.shape[0])
            rows = torch.empty((cap, c), dtype=torch.float32, device=out.device)
            lab = torch.empty(cap, dtype=torch.int64, device=out.device)
            if self.rows is None:
                self.count = torch.zeros(1, dtype=torch.int64, device=out.device)
            else:
                rows[: self.bound].copy_(self.rows[: self.bound])
                lab[: self.bound].copy_(self.labels[: self.bound])
            self.rows, self.labels = rows, lab
        ops.calib_rows(out, kind, labels, ignore_index, self.rows, self.labels, self.count)
        self.bound = need

    def finish(self):
        n = 0 if self.count is None else int(self.count.item())           # the one read-back
        if n == 0:
            raise ValueError("No valid pixels found in calibration loader.")
        return self.rows[:n].clone(), self.labels[:n].clone()


@torch.no_grad()
def cache_calib_logits(model, val_loader, device, cfg,
                       ignore_index: int = 255,
                       mode: str = "default",  # {"default","mc"}
                       mc_samples: int = 30,
                       *, keep_on_device: bool = True):
    """log p rows [N,C] and labels [N] of every pixel with label != ignore_index, in loader and (b, h, w) order.
    default: one forward per batch, rows = log(clamp(p, 1e-12)) with p by the model's output kind.
    mc: dropout layers on, p = mean of `mc_samples` probability maps.
    The tensors stay on `device` (keep_on_device=False: CPU copies, as the reference returns)."""
    from semanticlidarunc_amd.utils.inputs import set_model_inputs
    model.eval()
    kind_cache: dict[int, str] = {}
    if mode == "mc":
        set_dropout_mode(model, True)
    cache = _RowCache()
    for range_img, reflectivity, xyz, normals, labels in _progress(val_loader, f"TS cache ({mode})"):
        range_img, reflectivity = range_img.to(device), reflectivity.to(device)
        xyz, normals = xyz.to(device), normals.to(device)
        if labels.ndim == 4 and labels.shape[1] == 1:      # [B,1,H,W] or [B,H,W] -> [B,H,W]
            labels = labels.squeeze(1)
        labels = labels.long().to(device).contiguous()
        inputs = set_model_inputs(range_img, reflectivity, xyz, normals, cfg)
        if mode == "default":
            out = model(*inputs)
            kind = _output_kind(model, out, kind_cache)
            if kind not in ops.CALIB_KINDS:
                raise ValueError(f"Unknown output kind: {kind}")
        else:
            out, kind = _mc_mean_probs(model, inputs, mc_samples, kind_cache), "probs"
        cache.append(out.detach().float().contiguous(), kind, labels, ignore_index)
    if mode == "mc":
        set_dropout_mode(model, False)
    rows, row_labels = cache.finish()
    return (rows, row_labels) if keep_on_device else (rows.cpu(), row_labels.cpu())


def _start_temperature(init_T, prev_T):
    """init_T='auto': the previous temperature when there is one, else 1; a number: that number."""
    return (prev_T if (init_T == "auto" and prev_T is not None) else
            (float(init_T) if init_T != "auto" else 1.0))


def _save_temperature(save_path, T_value):
    if save_path:
        if os.path.dirname(save_path):
            os.makedirs(os.path.dirname(save_path), exist_ok=True)
        with open(save_path, "w") as f:
            json.dump({"temperature": T_value}, f)


def calibrate_temperature_from_cache(
    logits_cpu: torch.Tensor, labels_cpu: torch.Tensor,
    device, init_T: float | str = "auto",
    optimizer_type: str = "lbfgs", lr: float = 0.05, epochs: int = 2,
    chunk_size: int = 1_000_000, max_iter_lbfgs: int = 100,
    prev_T: float | None = None, save_path: str | None = None
) -> float:
    """Fit the scalar T that minimises NLL(softmax(rows / T)) on the cached rows (CPU tensors are uploaded once, device tensors
    are used in place); `chunk_size` bounds the rows of one launch.  Returns T; a label outside [0, C) raises ValueError after the
    first evaluation."""
    if labels_cpu.dtype != torch.long:
        labels_cpu = labels_cpu.long()
    rows = logits_cpu.detach().to(device=device, dtype=torch.float32).contiguous()
    row_labels = labels_cpu.to(device).contiguous()

    # the parameter is float64 (the kernel reads its float32 rounding): ten Adam steps on a float32 parameter already end an ulp or
    # two from where the float64 iteration ends
    log_T = torch.nn.Parameter(torch.log(torch.tensor([_start_temperature(init_T, prev_T)], dtype=torch.float64, device=device)))
    N = row_labels.numel()
    evaluations = [0]

    def check_labels(bad):
        evaluations[0] += 1
        if evaluations[0] == 1 and int(bad.item()) > 0:
            raise ValueError(f"calibrate_temperature_from_cache: {int(bad.item())} cached labels are outside [0, {rows.shape[1]})")

    if optimizer_type.lower() == "lbfgs":
        opt = torch.optim.LBFGS(
            [log_T], lr=1.0, max_iter=max_iter_lbfgs,
            line_search_fn="strong_wolfe", history_size=100,
            tolerance_grad=1e-10, tolerance_change=1e-12
        )

        @torch.enable_grad()
        def closure():
            opt.zero_grad(set_to_none=True)
            loss, bad = temp_nll_loss(log_T, rows, row_labels, None, N, chunk_size)
            loss.backward()
            check_labels(bad)
            return loss.detach()
        opt.step(closure)
    else:
        opt = torch.optim.Adam([log_T], lr=lr)
        for _ in range(epochs):
            perm = torch.randperm(N).to(device)            # drawn from the CPU generator, as the reference; the kernel gathers
            for i in range(0, N, chunk_size):
                j = min(i + chunk_size, N)
                loss, bad = temp_nll_loss(log_T, rows, row_labels, perm[i:j], j - i, None)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                check_labels(bad)

    T_value = float(log_T.exp().item())
    _save_temperature(save_path, T_value)
    return T_value


# drop-in mode (this file shadows the reference's module of the same import path): names it does not define come from there
from semanticlidarunc_amd._shadow import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(__name__, __file__, globals())
