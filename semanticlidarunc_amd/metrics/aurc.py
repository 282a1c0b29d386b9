"""Drop-in for ``metrics.aurc`` of the reference (``src/metrics/aurc.py``): ``UncertaintyAggregator`` with the same constructor,
``add_batch`` / ``finalize`` and result keys, and ``compute_batch_uncertainty_metrics`` with the same arguments and result dict --
but predictions, confidences, error flags, the sort, the risk-coverage curve, AURC, the optimal curve and the top-k% error recall
run in HIP kernels (``csrc/aurc.hip``); the samples stay on the GPU and nothing is copied to the host per batch.  The reservoir
is this module's own policy (merge, then ``rng.choice(merged, size=reservoir_size, replace=False)``): its draws are made on the
host with ``np.random.RandomState(seed)`` (the global ``np.random`` without a seed) exactly as the reference makes them and applied
as an index to the device buffers, so the kept sample set is the reference's.

Tie order.  A curve point sits at the FIRST element of every group of equal confidences (the reference's rule), so the selective
risk at that point depends on which of the tied samples is sorted first.  Here the sort is stable: tied samples keep their sample
order (NCHW scan order, batches in the order they were added; -0.0 == +0.0).  The reference's order inside a group is whatever
numpy's default argsort yields, which is not stable for large arrays; on tie-free confidences the two agree.  NaN confidences are
unspecified, as they are there.  The recalls are the fp64 quotient ``e / max(E, 1)`` of exact counts; the reference divides the
same two counts in fp32.

``rc_curve_stats``, ``aurc_from_risks_confids`` and the stand-alone plot functions are the reference's own (numpy / matplotlib on
host arrays) and come from the shadowed module when it is on the path."""
from __future__ import annotations

import math

import numpy as np
import torch

from semanticlidarunc_amd import ops
from semanticlidarunc_amd._reservoir import MergedReservoir


def entropy_from_probs(probs: torch.Tensor, eps=1e-12):
    """Normalized entropy from probs [B,C,H,W] -> [B,H,W] in [0,1]."""
    p = probs.clamp_min(eps)
    return -(p * torch.log(p)).sum(dim=1) / math.log(probs.shape[1])


def _samples(outputs_semantic, semantic, ent_mc, ignore_index, use_max_prob_confidence):
    """Valid pixels of one batch in NCHW order: (conf fp32 [n], is_error uint8 [n], valid-mask shape)."""
    assert outputs_semantic.ndim == 4 and semantic.ndim == 4 and semantic.shape[1] == 1
    ent = None if (ent_mc is None or use_max_prob_confidence) else ent_mc.to(torch.float32).contiguous()
    conf, flag = ops.aurc_samples(outputs_semantic.contiguous().float(), semantic[:, 0].long().contiguous(), ignore_index, ent,
                                  use_max_prob_confidence)
    keep = flag != 2                                        # boolean-mask order == the reference's conf[valid]
    return conf[keep], flag[keep], tuple(keep.shape)


def _with_tail(res: ops.AurcResult, n: int):
    """Host curve arrays: the device's points 0..m plus the reference's tail point (0, R_m) when samples remain behind s_m."""
    cov, risk = res.coverages.cpu().numpy(), res.rc_risks.cpu().numpy()
    if res.num_points and n - 2 - res.last_start > 0:
        cov, risk = np.append(cov, 0.0), np.append(risk, risk[-1])
    return cov, risk


@torch.no_grad()
def compute_batch_uncertainty_metrics(outputs_semantic: torch.Tensor, semantic: torch.Tensor, ent_mc: torch.Tensor = None,
                                      ignore_index: int = 255, use_max_prob_confidence: bool = False, ks=(1, 2, 5, 10, 20, 30, 40, 50)):
    """AURC / E-AURC and the full curve data for ONE batch (all valid pixels in it)."""
    conf, err, mask_shape = _samples(outputs_semantic, semantic, ent_mc, int(ignore_index), bool(use_max_prob_confidence))
    n = int(conf.numel())
    if n == 0:
        raise RuntimeError("compute_batch_uncertainty_metrics: the batch has no valid pixel")
    res = ops.aurc_from_samples(conf, err, ks=ks, want_curve=True)
    coverages, rc_risks = _with_tail(res, n)
    return {
        "AURC": res.aurc,
        "EAURC": res.eaurc,
        "coverages": coverages,
        "rc_risks": rc_risks,
        "ks": np.asarray(ks),
        "recalls": np.asarray(res.recalls),
        "num_pixels": n,
        "num_errors": res.num_errors,
        "valid_mask_shape": mask_shape,
    }


class UncertaintyAggregator:
    """Stream batches with ``add_batch(...)``, then ``finalize()`` for AURC / E-AURC over every valid pixel seen (or over a uniform
    subsample of at most ``reservoir_size`` of them) and, optionally, the two plots."""

    def __init__(self, ignore_index: int = 255, use_max_prob_confidence: bool = False, reservoir_size: int | None = None,
                 seed: int | None = None):
        self.ignore_index = int(ignore_index)
        self.use_max_prob_confidence = bool(use_max_prob_confidence)
        self.reservoir_size = None if reservoir_size is None else int(reservoir_size)
        self._buf = MergedReservoir(self.reservoir_size, seed)       # columns: conf fp32, is_error uint8 (device)
        self._added = False

    @property
    def _rng(self):
        return self._buf.rng

    @torch.no_grad()
    def add_batch(self, outputs_semantic: torch.Tensor, semantic: torch.Tensor, ent_mc: torch.Tensor = None):
        conf, err, _ = _samples(outputs_semantic, semantic, ent_mc, self.ignore_index, self.use_max_prob_confidence)
        self._buf.push(conf, err)
        self._added = True

    def _materialize(self):
        if not self._added:
            raise RuntimeError("No batches added. Call add_batch(...) first.")
        conf, err = self._buf.materialize()
        if conf.numel() == 0:
            raise RuntimeError("No valid pixel in the batches added.")
        return conf, err

    def finalize(self, make_plots: bool = True, title_suffix: str = "", save_dir: str | None = None, epoch: int | None = None,
                 filename_prefix: str = "", dpi: int = 150, show: bool = False, close: bool = True):
        conf, err = self._materialize()
        n = int(conf.numel())
        res = ops.aurc_from_samples(conf, err, want_curve=bool(make_plots))     # the curve is allocated only for the plots
        rc_path = er_path = None
        if make_plots:
            import os
            if save_dir:
                os.makedirs(save_dir, exist_ok=True)
                tag = (f"{filename_prefix}epoch_{int(epoch):06d}_" if epoch is not None else filename_prefix)
                rc_path = os.path.join(save_dir, f"{tag}rc_curve.png")
                er_path = os.path.join(save_dir, f"{tag}uncertainty_error_recall.png")
            coverages, rc_risks = _with_tail(res, n)
            self._plot_xy(coverages, rc_risks, None, "Coverage (fraction kept)", "Risk (error rate on kept)",
                          f"Risk-Coverage (dataset){title_suffix}", rc_path, dpi, show, close)
            self._plot_xy(ops.AURC_KS, res.recalls, "o", "Top-k% most-uncertain pixels", "Recall of errors",
                          f"Uncertainty Error-Recall{title_suffix}", er_path, dpi, show, close)
        return {
            "AURC": res.aurc,
            "EAURC": res.eaurc,
            "num_pixels": n,
            "rc_curve_path": rc_path,
            "error_recall_path": er_path,
        }

    @staticmethod
    def _plot_xy(x, y, marker, xlabel, ylabel, title, save_path, dpi, show, close):
        import matplotlib
        if not show:
            matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        fig = plt.figure()
        plt.plot(x, y, marker=marker)
        plt.xlabel(xlabel)
        plt.ylabel(ylabel)
        plt.title(title)
        plt.grid(True, linestyle=":")
        fig.tight_layout()
        if save_path:
            fig.savefig(save_path, bbox_inches="tight", dpi=dpi)
        if show:
            plt.show()
        if close:
            plt.close(fig)


# drop-in mode (this file shadows the reference's module of the same import path): names it does not define come from there
from semanticlidarunc_amd._shadow import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(__name__, __file__, globals())
