"""MC-dropout prediction of a scan STREAM replayed as one HIP graph (`inference_ouster.py` processes one scan at a time).

At one scan per step the T stacked passes are 8 images per launch: 45 kernels of ~40 us each, where the gaps between eager launches are a
tenth of the step.  Nothing on the path synchronises with the host, so the forward + fused head / MC reduction is captured once into a
``torch.cuda.CUDAGraph`` (a hipGraph on ROCm) on a static input buffer.  The one thing that must NOT be frozen into the graph is the dropout
draw -- its Philox offset is a launch argument -- so the multipliers live in a persistent buffer that `slu_dropout_draw` refills eagerly
before every replay (one launch; torch's CUDA generator advances as in the eager path, `torch.manual_seed` reproduces a stream).

    stream = GraphedMCPredict(model, example_scan, T=8)
    for scan in scans:                       # [1, 5, 64, 2048] each, on the GPU
        p_bar, h_norm, mi_norm, preds = stream(scan)     # STATIC tensors: consume (or clone) them before the next call

Half-precision SalsaNext only (the fused head path: `SalsaNext.mc_fused_ok`); results equal `utils.mc_dropout.mc_predict` with the same seed."""
from __future__ import annotations

import torch

from semanticlidarunc_amd.utils.mc_dropout import dropout_sampling


class GraphedMCPredict:
    def __init__(self, model: torch.nn.Module, example: torch.Tensor, T: int = 8, eps: float = 1e-12, warmup: int = 2):
        if not example.is_cuda or example.dim() != 4:
            raise RuntimeError("GraphedMCPredict: a [B, C, H, W] example tensor on the GPU is needed")
        model.eval()
        with torch.no_grad():
            ok = hasattr(model, "mc_fused_ok") and model.mc_fused_ok(example, T)
        if not ok:
            raise RuntimeError("GraphedMCPredict covers the fused half-precision MC path of SalsaNext (set_conv_precision('f16'), eval BatchNorm)")
        self.model, self.T, self.eps = model, int(T), float(eps)
        self._x = example.clone()
        n = self.T * example.shape[0]
        with dropout_sampling(model, enable=True):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():      # warm-up: packed weights, folded BatchNorm, the dropout plan, allocator
                for _ in range(max(1, warmup)):
                    model.mc_predict_fused(self._x, self.T, self.eps, False)
            torch.cuda.current_stream().wait_stream(side)
            self._scales = None
            self._plan = None
            # (tables in the order the captured forward reads them; None: no Dropout2d site is active, a deterministic model)
            drawn = model._predraw_dropout(n, example.device, sx_stored=model._in_place_blocks(n, example.shape[2], example.shape[3]))
            if drawn is not None:
                plan = model.__dict__.get("_drop_plan")
                if plan is None:
                    raise RuntimeError("GraphedMCPredict needs the one-launch dropout draw (SLU_DROPOUT_KERNEL=1)")
                self._plan, flags = plan[1], plan[2]
                self._buf = torch.empty(self._plan.total, dtype=torch.float32, device=example.device)
                self._scales = self._plan.run(out=self._buf)               # views of the persistent buffer
                for k in flags:
                    self._scales[k] = True
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph), torch.no_grad():
                self._out = model.mc_predict_fused(self._x, self.T, self.eps, False, scales=self._scales if self._scales is not None else {})

    @torch.no_grad()
    def __call__(self, x: torch.Tensor):
        if x.shape != self._x.shape:
            raise RuntimeError(f"GraphedMCPredict: captured for {tuple(self._x.shape)}, got {tuple(x.shape)}")
        self._x.copy_(x)
        if self._plan is not None:
            self._plan.run(out=self._buf)          # fresh masks into the addresses the graph reads
        self.graph.replay()
        return self._out
