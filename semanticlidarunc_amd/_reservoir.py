"""Device-resident sample columns with the capped-buffer policy of the reference's aggregators
(``metrics/auroc.py:125-141``, ``models/evaluator.py:681-700``): unlimited append when ``cap`` is None; otherwise fill up to
``cap`` (a random subset of the incoming batch when it does not fit), and once full keep each incoming sample with
probability ``cap / seen`` and let the kept ones overwrite random slots.  The random choices come from a numpy Generator on
the host -- the same calls, in the same order, as the reference makes -- and are applied to tensors that stay on the GPU."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch


class CappedColumns:
    def __init__(self, cap: Optional[int], seed: int = 0):
        self.cap = cap
        self.rng = np.random.default_rng(seed)
        self.clear()

    def clear(self) -> None:
        self.columns: Optional[List[torch.Tensor]] = None
        self.seen = 0

    def __len__(self) -> int:
        return 0 if self.columns is None else int(self.columns[0].numel())

    def _extend(self, cols: Sequence[torch.Tensor]) -> None:
        self.columns = list(cols) if self.columns is None else [torch.cat([old, new]) for old, new in zip(self.columns, cols)]

    def push(self, *cols: torch.Tensor) -> None:
        """Add one batch of equally long 1-D columns."""
        incoming = int(cols[0].numel())
        if incoming == 0:
            return
        self.seen += incoming
        if self.cap is None:
            self._extend(cols)
            return
        dev = cols[0].device
        room = self.cap - len(self)
        if room > 0:
            if incoming > room:                                    # keep a uniformly drawn subset that fits
                pick = torch.from_numpy(self.rng.choice(incoming, size=room, replace=False)).to(dev)
                cols = [c[pick] for c in cols]
            self._extend(cols)
            return
        accept = self.rng.random(incoming) < min(1.0, float(self.cap) / float(self.seen + 1e-9))
        if accept.any():
            accept_t = torch.from_numpy(accept).to(dev)
            cols = [c[accept_t] for c in cols]
            slots = torch.from_numpy(self.rng.choice(self.cap, size=int(cols[0].numel()), replace=False)).to(dev)
            for buf, c in zip(self.columns, cols):
                buf[slots] = c


class MergedReservoir:
    """The reservoir of the reference's ``metrics/aurc.py`` (``UncertaintyAggregator._append_reservoir``, :250-270): unlimited append
    when ``size`` is None; otherwise the incoming batch is concatenated BEHIND what is kept and, when the result exceeds ``size``,
    ``rng.choice(merged, size=size, replace=False)`` picks what stays (in the drawn order).  ``rng`` is
    ``np.random.RandomState(seed)``, or the global ``np.random`` when ``seed`` is None; the draw is made on the host with the same
    call, in the same order, as the reference's, and applied as an index to columns that stay on their device."""

    def __init__(self, size: Optional[int], seed: Optional[int] = None):
        self.size = None if size is None else int(size)
        self.rng = np.random.RandomState(seed) if seed is not None else np.random
        self.clear()

    def clear(self) -> None:
        self.columns: Optional[List[torch.Tensor]] = None
        self._pending: List[Sequence[torch.Tensor]] = []        # size None: concatenated once, on first read

    def __len__(self) -> int:
        cols = self.materialize()
        return 0 if cols is None else int(cols[0].numel())

    def materialize(self) -> Optional[List[torch.Tensor]]:
        if self._pending:
            parts = ([self.columns] if self.columns is not None else []) + self._pending
            self.columns = [torch.cat(col) for col in zip(*parts)]
            self._pending = []
        return self.columns

    def push(self, *cols: torch.Tensor) -> None:
        """Add one batch of equally long 1-D columns (an empty batch is kept too: the reference then has storage, if no samples)."""
        if self.size is None:
            self._pending.append(cols)
            return
        merged = list(cols) if self.columns is None else [torch.cat([old, new]) for old, new in zip(self.columns, cols)]
        total = int(merged[0].numel())
        if total > self.size:
            pick = torch.from_numpy(self.rng.choice(total, size=self.size, replace=False)).to(merged[0].device)
            merged = [c[pick] for c in merged]
        self.columns = merged
