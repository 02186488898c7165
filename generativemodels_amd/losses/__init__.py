"""generative.losses on the MI355X: JukeboxLoss, the spectral loss, on the Fourier kernels of csrc/spectral.hip (forward and gradient)."""
from .spectral_loss import JukeboxLoss

__all__ = ["JukeboxLoss"]
