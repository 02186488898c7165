"""Multi-scale SSIM (Wang, Simoncelli, Bovik 2003) with the reference's MultiScaleSSIMMetric interface: one fused SSIM / cs launch per scale
and one pooling launch between scales; nothing of image size is kept besides the pooled pair."""
from __future__ import annotations

from collections.abc import Sequence

import torch

from .. import autograd, ops
from ._base import CumulativeRegressionMetric, MetricReduction
from .ssim import KernelType, _check_dims, _constants, _per_axis, _wants_grad, window_taps


class MultiScaleSSIMMetric(CumulativeRegressionMetric):
    """prod_j relu(cs_j) ** w_j over the scales j, the last factor being relu(ssim) of the coarsest scale; each scale halves every extent
    (2x average pooling, floor).  One value per batch item, differentiable in both images.

    Args: as SSIMMetric, plus
        weights: one exponent per scale.
    """

    def __init__(self, spatial_dims: int, data_range: float = 1.0, kernel_type: KernelType | str = KernelType.GAUSSIAN,
                 kernel_size: int | Sequence[int] = 11, kernel_sigma: float | Sequence[float] = 1.5, k1: float = 0.01, k2: float = 0.03,
                 weights: Sequence[float] = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), reduction: MetricReduction | str = MetricReduction.MEAN,
                 get_not_nans: bool = False) -> None:
        super().__init__(reduction=reduction, get_not_nans=get_not_nans)
        self.spatial_dims = spatial_dims
        self.data_range = data_range
        self.kernel_type = kernel_type
        self.kernel_size = _per_axis(kernel_size, spatial_dims)
        self.kernel_sigma = _per_axis(kernel_sigma, spatial_dims)
        self.k1 = k1
        self.k2 = k2
        self.weights = weights

    def _compute_metric(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        _check_dims(y_pred, self.spatial_dims)
        if y.shape != y_pred.shape:
            raise ValueError(f"y_pred and y should have same shapes, got {y_pred.shape} and {y.shape}.")
        # the size rule of the reference, as it is: the divisor is (number of scales - 1) SQUARED
        divisor = max(1, len(self.weights) - 1) ** 2
        for extent, k in zip(y_pred.shape[2:], self.kernel_size):
            if extent // divisor <= k - 1:
                raise ValueError(f"For a given number of `weights` parameters {len(self.weights)} and kernel size {k}, the image height must be "
                                 f"larger than {(k - 1) * divisor}.")
        taps = window_taps(self.spatial_dims, self.kernel_type, self.kernel_size, self.kernel_sigma)
        c1, c2 = _constants(self.data_range, self.k1, self.k2)
        if _wants_grad(y_pred, y):
            stacked = autograd.ms_ssim_factors(y_pred, y, taps, c1, c2, len(self.weights))
        else:
            factors = []
            last = len(self.weights) - 1
            for scale in range(len(self.weights)):
                ssim_mean, cs_mean, _, _ = ops.ssim_cs(y_pred, y, taps, c1, c2)
                factors.append(ssim_mean if scale == last else cs_mean)
                if scale != last:
                    y_pred, y = ops.avgpool2_pair(y_pred, y)
            stacked = torch.stack(factors)
        # (scales, batch) numbers: combined in fp64 on the device, rounded once
        stacked = torch.relu(stacked.double())
        weights = torch.tensor(self.weights, dtype=torch.float32, device=stacked.device).double().view(-1, 1)
        return torch.prod(stacked ** weights, dim=0).float().view(-1, 1)
