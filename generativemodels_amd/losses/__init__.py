"""generative.losses on the MI355X: JukeboxLoss, the spectral loss, on the Fourier kernels of csrc/spectral.hip (forward and gradient),
PatchAdversarialLoss on gm_patch_adv_loss (csrc/adversarial_loss.hip), and PerceptualLoss -- LPIPS over a frozen AlexNet / VGG16 stack -- on the
convolutions and the pooling, distance and slice-gather kernels of csrc/perceptual.hip."""
from .adversarial_loss import AdversarialCriterions, PatchAdversarialLoss
from .perceptual import PerceptualLoss
from .spectral_loss import JukeboxLoss

__all__ = ["AdversarialCriterions", "JukeboxLoss", "PatchAdversarialLoss", "PerceptualLoss"]
