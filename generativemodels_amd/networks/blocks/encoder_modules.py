"""SpatialRescaler for MI355X: constructor arguments, checks, state_dict names and forward contract of the reference's
generative/networks/blocks/encoder_modules.py:24-83 (the conditioning pre-processor of latent diffusion, after CompVis/latent-diffusion
ldm/modules/encoders/modules.py): an optional 1x1 channel mapper, then `n_stages` interpolations by `multiplier` (or one to `size`).

    x -> channel_mapper (1x1 convolution, when out_channels is given) -> n_stages x F.interpolate(mode=method)

MI355X mapping: the input goes to the channels-last arena once; the 1x1 mapper is a row GEMM over the arena's voxels; every stage is ONE launch
of the separable tap kernel (gm_resize_taps, csrc/resize.hip) on tables the host planner makes once per geometry (resize_plan.py) -- stage k plans
from stage k - 1's output extents -- and the result goes back to channels first.  The order is the reference's (map, then resize) whatever the
direction of the resize: swapping them would change the rounding.  With gradients recorded every step is a differentiable native op
(generativemodels_amd.autograd): the resize gradient is the same kernel on transposed tables, the mapper's weight and bias gradients come back in
the parameters' dtype.

One departure from the reference: the constructor does not print the channel mapping."""
from __future__ import annotations

from collections.abc import Sequence

import torch
import torch.nn as nn

from ... import ops

__all__ = ["SpatialRescaler"]

_METHODS = ["nearest", "linear", "bilinear", "trilinear", "bicubic", "area"]
_CONV = {1: nn.Conv1d, 2: nn.Conv2d, 3: nn.Conv3d}


class _ChannelMapper(nn.Module):
    """Holder of the 1x1 convolution's parameters under the child name `conv` (the layout of MONAI's Convolution(conv_only=True)); nn.ConvNd is the
    parameter container with the reference's initialisation, its forward is never called."""

    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, bias: bool) -> None:
        super().__init__()
        self.conv = _CONV[spatial_dims](in_channels, out_channels, kernel_size=1, bias=bias)
        self._rows = None

    def weight_rows(self) -> torch.Tensor:
        """The weight as the (out, in) matrix of the row GEMM: one view object per parameter version, so the packed panel is cached on it."""
        w = self.conv.weight
        key = (w._version, w.data_ptr(), w.dtype, w.device)
        if self._rows is None or self._rows[0] != key:
            self._rows = (key, w.detach().view(w.shape[0], w.shape[1]))
        return self._rows[1]

    def forward(self, x):  # pragma: no cover - driven through SpatialRescaler
        raise RuntimeError("the channel mapper runs as a row GEMM inside SpatialRescaler, not as a torch module")


class SpatialRescaler(nn.Module):
    """Drop-in for generative.networks.blocks.encoder_modules.SpatialRescaler.

    Args:
        spatial_dims: number of spatial dimensions.
        n_stages: number of interpolation stages.
        size: output spatial size (int or one int per spatial axis); needs n_stages == 1.
        method: nearest, linear, bilinear, trilinear, bicubic or area.
        multiplier: scale factor of every stage (float or one float per spatial axis).
        in_channels: number of input channels.
        out_channels: number of output channels; None = no channel mapper.
        bias: whether the channel mapper has a bias term."""

    def __init__(self, spatial_dims: int = 2, n_stages: int = 1, size: Sequence[int] | int | None = None, method: str = "bilinear",
                 multiplier: Sequence[float] | float | None = None, in_channels: int = 3, out_channels: int | None = None,
                 bias: bool = False) -> None:
        super().__init__()
        self.n_stages = n_stages
        assert self.n_stages >= 0
        assert method in _METHODS
        if size is not None and n_stages != 1:
            raise ValueError("when size is not None, n_stages should be 1.")
        if size is not None and multiplier is not None:
            raise ValueError("only one of size or multiplier should be defined.")
        self.spatial_dims, self.method = spatial_dims, method
        self.size = tuple(size) if isinstance(size, (tuple, list)) else size
        self.multiplier = tuple(multiplier) if isinstance(multiplier, (tuple, list)) else multiplier
        self.remap_output = out_channels is not None
        if self.remap_output:
            self.channel_mapper = _ChannelMapper(spatial_dims, in_channels, out_channels, bias)

    def _entry(self, x: torch.Tensor, differentiable: bool) -> torch.Tensor:
        """x in the compute dtype: with a channel mapper the package's convention (its parameters' dtype, or the active autocast region's: the
        input is cast); without one the input's dtype is kept, as F.interpolate keeps it."""
        if not self.remap_output:
            ops.dt_code(x.dtype)
            return x
        pdt = self.channel_mapper.conv.weight.dtype
        if not differentiable:
            return ops.entry_cast(x, pdt)
        dt = ops.compute_dtype(pdt)
        if x.dtype != dt:
            if ops.autocast_dtype() is None:
                raise TypeError(f"input dtype {x.dtype} does not match the model dtype {pdt}")
            from ... import autograd as A

            x = A.cast(x, dt)
        return x

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """N C [D] H W in / out, like the reference module."""
        ops.require_device(x)
        if x.dim() != self.spatial_dims + 2:
            raise ValueError(f"SpatialRescaler(spatial_dims={self.spatial_dims}) expects a {self.spatial_dims + 2}-D input, got {tuple(x.shape)}")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return self._forward_train(x)
        with torch.no_grad():
            a = ops.to_channels_last(self._entry(x, False).contiguous())
            if self.remap_output:
                n, sp = a.shape[0], tuple(a.shape[1:-1])
                y = ops.linear(a.reshape(n, -1, a.shape[-1]), self.channel_mapper.weight_rows(), self.channel_mapper.conv.bias)
                a = y.reshape(n, *sp, y.shape[-1])
            for _ in range(self.n_stages):
                a = ops.resize(a, self.method, size=self.size, scale_factor=self.multiplier)
            return ops.to_channels_first(a)

    def _forward_train(self, x: torch.Tensor) -> torch.Tensor:
        from ... import autograd as A

        a = A.to_arena(self._entry(x, True).contiguous())
        if self.remap_output:
            conv = self.channel_mapper.conv
            n, sp = a.shape[0], tuple(a.shape[1:-1])
            y = A.linear(a.reshape(n, -1, a.shape[-1]), conv.weight.view(conv.weight.shape[0], conv.weight.shape[1]), conv.bias)
            a = y.reshape(n, *sp, y.shape[-1])
        for _ in range(self.n_stages):
            a = A.resize(a, self.method, size=self.size, scale_factor=self.multiplier)
        return A.from_arena(a)

    def encode(self, x: torch.Tensor) -> torch.Tensor:
        return self(x)
