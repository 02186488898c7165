"""Structural similarity (Wang et al. 2004) with the constructor and call signature of the reference's SSIMMetric, evaluated by one fused
separable kernel (ops.ssim_cs): the Gaussian / uniform window is an outer product of 1-D tables, so the five local moments take
k taps per axis instead of k^d per output, and only the per-batch means (or, on request, the two maps) leave the chip."""
from __future__ import annotations

from collections.abc import Sequence
from enum import Enum

import torch

from .. import autograd, ops
from ._base import CumulativeRegressionMetric, MetricReduction


class KernelType(str, Enum):
    GAUSSIAN = "gaussian"
    UNIFORM = "uniform"

    def __str__(self) -> str:
        return self.value


def _per_axis(value, spatial_dims: int) -> tuple:
    if isinstance(value, Sequence) and not isinstance(value, str):
        return tuple(value)
    return (value,) * spatial_dims


def gaussian_taps(size: int, sigma: float) -> torch.Tensor:
    """Normalised fp32 samples of a Gaussian at the `size` unit-spaced points centred on 0 (half-integers for an even size)."""
    offsets = torch.arange(size, dtype=torch.float32) - (size - 1) / 2
    g = torch.exp(-0.5 * (offsets / sigma) ** 2)
    return g / g.sum()


def window_taps(spatial_dims: int, kernel_type, kernel_size, kernel_sigma) -> list[list[float]]:
    """One normalised 1-D table per spatial axis whose outer product is the SSIM window."""
    sizes, sigmas = _per_axis(kernel_size, spatial_dims), _per_axis(kernel_sigma, spatial_dims)
    if len(sizes) != spatial_dims or len(sigmas) != spatial_dims:
        raise ValueError(f"kernel_size and kernel_sigma need one entry per spatial dimension ({spatial_dims}), got {sizes} and {sigmas}")
    limit = ops.ssim_max_window()
    if any(int(k) != k or k < 1 or k > limit for k in sizes):
        raise ValueError(f"kernel_size entries must be integers in 1..{limit} (the limit the SSIM kernel is built for), got {sizes}")
    if str(kernel_type) == KernelType.GAUSSIAN.value:
        return [gaussian_taps(int(k), float(s)).tolist() for k, s in zip(sizes, sigmas)]
    if str(kernel_type) == KernelType.UNIFORM.value:
        return [[1.0 / int(k)] * int(k) for k in sizes]
    raise ValueError(f"kernel_type must be 'gaussian' or 'uniform', got {kernel_type!r}")


def _check_dims(y_pred: torch.Tensor, spatial_dims: int) -> None:
    dims = y_pred.dim()
    if spatial_dims == 2 and dims != 4:
        raise ValueError(f"y_pred should have 4 dimensions (batch, channel, height, width) when using 2 spatial dimensions, got {dims}.")
    if spatial_dims == 3 and dims != 5:
        raise ValueError(f"y_pred should have 5 dimensions (batch, channel, height, width, depth) when using 3 spatial dimensions, got {dims}.")


def _constants(data_range: float, k1: float, k2: float) -> tuple[float, float]:
    return (k1 * data_range) ** 2, (k2 * data_range) ** 2


def _wants_grad(y_pred: torch.Tensor, y: torch.Tensor) -> bool:
    """The differentiable route (autograd.ssim_cs / ms_ssim_factors: the same forward launches, plus a graph node) is taken only where a gradient can flow."""
    return torch.is_grad_enabled() and (y_pred.requires_grad or y.requires_grad)


def compute_ssim_and_cs(y_pred: torch.Tensor, y: torch.Tensor, spatial_dims: int, data_range: float = 1.0,
                        kernel_type: KernelType | str = KernelType.GAUSSIAN, kernel_size: int | Sequence[int] = 11,
                        kernel_sigma: float | Sequence[float] = 1.5, k1: float = 0.01, k2: float = 0.03) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (ssim, cs): fp32 maps of shape (batch, channel, *(n - k + 1)) over the positions where the window fits; differentiable in both images."""
    if y.shape != y_pred.shape:
        raise ValueError(f"y_pred and y should have same shapes, got {y_pred.shape} and {y.shape}.")
    taps = window_taps(spatial_dims, kernel_type, kernel_size, kernel_sigma)
    c1, c2 = _constants(data_range, k1, k2)
    _, _, ssim_map, cs_map = (autograd if _wants_grad(y_pred, y) else ops).ssim_cs(y_pred, y, taps, c1, c2, want_maps=True)
    return ssim_map, cs_map


class SSIMMetric(CumulativeRegressionMetric):
    """SSIM(x, y) = (2 mu_x mu_y + c1)(2 sigma_xy + c2) / ((mu_x^2 + mu_y^2 + c1)(sigma_x^2 + sigma_y^2 + c2)), averaged over channels and
    window positions: one value per batch item, differentiable in both images (`(1 - metric(recon, images).mean()).backward()`).

    Args:
        spatial_dims: 2 or 3.
        data_range: value range of the images (1.0 or 255 usually).
        kernel_type: "gaussian" or "uniform".
        kernel_size: window size, one int or one per axis (even sizes allowed; at most ops.ssim_max_window() per axis).
        kernel_sigma: Gaussian standard deviation, one float or one per axis.
        k1, k2: stability constants of the luminance and contrast terms.
        reduction, get_not_nans: how aggregate() reduces the buffered values.
    """

    def __init__(self, spatial_dims: int, data_range: float = 1.0, kernel_type: KernelType | str = KernelType.GAUSSIAN,
                 kernel_size: int | Sequence[int] = 11, kernel_sigma: float | Sequence[float] = 1.5, k1: float = 0.01, k2: float = 0.03,
                 reduction: MetricReduction | str = MetricReduction.MEAN, get_not_nans: bool = False) -> None:
        super().__init__(reduction=reduction, get_not_nans=get_not_nans)
        self.spatial_dims = spatial_dims
        self.data_range = data_range
        self.kernel_type = kernel_type
        self.kernel_size = _per_axis(kernel_size, spatial_dims)
        self.kernel_sigma = _per_axis(kernel_sigma, spatial_dims)
        self.k1 = k1
        self.k2 = k2

    def _compute_metric(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        _check_dims(y_pred, self.spatial_dims)
        if y.shape != y_pred.shape:
            raise ValueError(f"y_pred and y should have same shapes, got {y_pred.shape} and {y.shape}.")
        taps = window_taps(self.spatial_dims, self.kernel_type, self.kernel_size, self.kernel_sigma)
        c1, c2 = _constants(self.data_range, self.k1, self.k2)
        ssim_mean, _, _, _ = (autograd if _wants_grad(y_pred, y) else ops).ssim_cs(y_pred, y, taps, c1, c2)
        return ssim_mean.view(-1, 1)
