"""Maximum mean discrepancy with a linear kernel (Gretton et al. 2012, eq. 3 under Lemma 6), as the reference's MMDMetric states it: the plain
means of the three Gram matrices.  mean(Y Y^T) is |sum_i y_i|^2 / B^2, so ops.mmd_terms needs the column sums only."""
from __future__ import annotations

from collections.abc import Callable

import torch

from .. import ops
from ._base import Metric


class MMDMetric(Metric):
    """Args:
        y_transform: applied to y first (a filter, a feature extractor, ...), or None.
        y_pred_transform: applied to y_pred first, or None.
    """

    def __init__(self, y_transform: Callable | None = None, y_pred_transform: Callable | None = None) -> None:
        self.y_transform = y_transform
        self.y_pred_transform = y_pred_transform

    def __call__(self, y: torch.Tensor, y_pred: torch.Tensor) -> torch.Tensor:
        """y, y_pred: (B, C, ...) samples of the two distributions -> 0-dim fp32 tensor."""
        if self.y_transform is not None:
            y = self.y_transform(y)
        if self.y_pred_transform is not None:
            y_pred = self.y_pred_transform(y_pred)
        if y_pred.shape != y.shape:
            raise ValueError("y_pred and y shapes dont match after being processed by their transforms, received y_pred: "
                             f"{y_pred.shape} and y: {y.shape}")
        batch = y.shape[0]
        return ops.mmd_terms(y.reshape(batch, -1), y_pred.reshape(batch, -1))
