"""generative.metrics on the MI355X: SSIM, MS-SSIM and MMD run on the kernels of csrc/metrics.hip (one separable pass per SSIM scale, column sums for
MMD); FID is fp64 host arithmetic."""
from .fid import FIDMetric, get_fid_score
from .mmd import MMDMetric
from .ms_ssim import MultiScaleSSIMMetric
from .ssim import KernelType, SSIMMetric, compute_ssim_and_cs

__all__ = ["FIDMetric", "MMDMetric", "MultiScaleSSIMMetric", "SSIMMetric"]
