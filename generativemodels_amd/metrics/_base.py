"""The small part of a metric framework the four metrics need: a callable base, and a cumulative base that buffers per-batch values and
reduces them over their not-NaN entries.  The buffers are a handful of numbers per batch; reducing them is host-side torch arithmetic."""
from __future__ import annotations

from enum import Enum

import torch


class MetricReduction(str, Enum):
    NONE = "none"
    MEAN = "mean"
    SUM = "sum"
    MEAN_BATCH = "mean_batch"
    SUM_BATCH = "sum_batch"
    MEAN_CHANNEL = "mean_channel"
    SUM_CHANNEL = "sum_channel"

    def __str__(self) -> str:
        return self.value


def _safe_mean(total: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    return torch.where(count > 0, total / count.clamp(min=1), torch.zeros_like(total))


def reduce_not_nans(values: torch.Tensor, reduction: MetricReduction | str):
    """values: (batch, channel).  -> (reduced, not_nans): the reduction runs over the entries that are not NaN, `not_nans` counts them along
    the reduced dimensions ("mean" averages each row over its channels first, then the rows that had any entry)."""
    mode = MetricReduction(str(reduction))
    ok = ~torch.isnan(values)
    counts = ok.to(values.dtype)
    if mode is MetricReduction.NONE:
        return values, counts
    clean = torch.where(ok, values, torch.zeros_like(values))
    if mode is MetricReduction.MEAN:
        per_row = counts.sum(dim=1)
        rows = _safe_mean(clean.sum(dim=1), per_row)
        live = (per_row > 0).to(values.dtype).sum(dim=0)
        return _safe_mean(rows.sum(dim=0), live), live
    if mode is MetricReduction.SUM:
        return clean.sum(), counts.sum()
    dim = 0 if mode in (MetricReduction.MEAN_BATCH, MetricReduction.SUM_BATCH) else 1
    n = counts.sum(dim=dim)
    total = clean.sum(dim=dim)
    if mode in (MetricReduction.MEAN_BATCH, MetricReduction.MEAN_CHANNEL):
        return _safe_mean(total, n), n
    return total, n


class Metric:
    """A metric is called with two tensors and returns a tensor."""

    def __call__(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} does not implement __call__")


class CumulativeRegressionMetric(Metric):
    """`metric(y_pred, y)` computes the per-batch-item values (`_compute_metric`, (batch, channel)), keeps them and returns them;
    `aggregate()` reduces everything kept since the last `reset()`."""

    def __init__(self, reduction: MetricReduction | str = MetricReduction.MEAN, get_not_nans: bool = False) -> None:
        self.reduction = reduction
        self.get_not_nans = get_not_nans
        self._buffer: list[torch.Tensor] = []

    def _compute_metric(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def __call__(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        if not isinstance(y_pred, torch.Tensor) or not isinstance(y, torch.Tensor):
            raise ValueError("y_pred and y must be torch tensors")
        if y_pred.shape != y.shape:
            raise ValueError(f"y_pred and y shapes dont match, received y_pred: [{y_pred.shape}] and y: [{y.shape}]")
        if y_pred.dim() < 2:
            raise ValueError("either channel or spatial dimensions required, found only batch")
        value = self._compute_metric(y_pred, y)
        self._buffer.append(value.detach())
        return value

    def reset(self) -> None:
        self._buffer = []

    def get_buffer(self):
        """Everything computed since the last reset, concatenated along the batch dimension (None when empty)."""
        return torch.cat(self._buffer, dim=0) if self._buffer else None

    def aggregate(self, reduction: MetricReduction | str | None = None):
        data = self.get_buffer()
        if not isinstance(data, torch.Tensor):
            raise ValueError("the metric has no values to aggregate: call it first")
        value, not_nans = reduce_not_nans(data, reduction or self.reduction)
        return (value, not_nans) if self.get_not_nans else value
