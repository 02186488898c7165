"""JukeboxLoss (reference: generative/losses/spectral_loss.py) on the native Fourier kernels: nothing here calls torch.fft."""
from __future__ import annotations

from enum import Enum
from typing import Optional, Sequence

import torch
from torch.nn.modules.loss import _Loss

from .. import autograd as ag
from ..spectral_plan import NORMS


class LossReduction(str, Enum):
    NONE = "none"
    MEAN = "mean"
    SUM = "sum"


class JukeboxLoss(_Loss):
    """The spectral loss of Dhariwal et al., "Jukebox: A generative model for music" (https://arxiv.org/abs/2005.00341), section 3.3: the squared difference of
    the amplitudes of the Fourier transforms of `input` and `target`, both (B, C, *spatial).  As in the reference the transform runs over the channel
    axis as well as the spatial axes.

    Args:
        spatial_dims: number of spatial dimensions (1 to 3).
        fft_signal_size: signal size of the transformed axes (channel, then spatial): each is zero-filled or cropped to it, as torch.fft.fftn's `s`.
        fft_norm: "forward", "backward" or "ortho", as torch.fft.fftn's `norm`.
        reduction: "none" (the (B, *signal size) tensor), "mean" or "sum".

    The loss value is fp32 whatever the dtype of the operands (float32, bfloat16, float16: converted on load, all arithmetic in fp32); the gradients come back
    in each operand's dtype.  Either or both operands may require a gradient.  "sum" and "mean" are bit-reproducible (fixed-order folds, no atomics).

    Deviations from the reference.  (1) Where a bin's amplitude is exactly zero the reference's sqrt has an infinite derivative and autograd returns NaN for
    the WHOLE gradient (a constant image: every bin but one); here such a bin contributes zero.  (2) bf16 and fp16 operands are taken directly (torch.fft
    has no bf16 and only some fp16 sizes).  (3) fft_norm and the length of fft_signal_size are checked at construction rather than at the first call.  (4) The gradient is differentiable once: a second
    differentiation through the loss (a gradient penalty) raises."""

    def __init__(self, spatial_dims: int, fft_signal_size: Optional[Sequence[int]] = None, fft_norm: str = "ortho",
                 reduction: LossReduction | str = LossReduction.MEAN) -> None:
        super().__init__(reduction=LossReduction(reduction).value)
        if not 1 <= int(spatial_dims) <= 3:
            raise ValueError(f"JukeboxLoss: spatial_dims must be 1, 2 or 3, got {spatial_dims}")
        if fft_norm not in NORMS:
            raise ValueError(f"JukeboxLoss: fft_norm must be one of {NORMS}, got {fft_norm!r}")
        self.spatial_dims = int(spatial_dims)
        self.fft_dim = tuple(range(1, self.spatial_dims + 2))
        if fft_signal_size is not None:
            fft_signal_size = tuple(int(v) for v in fft_signal_size)
            if len(fft_signal_size) != len(self.fft_dim) or any(v < 1 for v in fft_signal_size):
                raise ValueError(f"JukeboxLoss: fft_signal_size needs {len(self.fft_dim)} positive entries (channel + spatial axes), got {fft_signal_size}")
        self.fft_signal_size = fft_signal_size
        self.fft_norm = fft_norm

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        for name, t in (("input", input), ("target", target)):
            if t.dim() != self.spatial_dims + 2:
                raise ValueError(f"JukeboxLoss: {name} must be (B, C, *spatial) with {self.spatial_dims} spatial axes, got shape {tuple(t.shape)}")
        return ag.spectral_loss(input, target, self.fft_signal_size, self.fft_norm, self.reduction)
