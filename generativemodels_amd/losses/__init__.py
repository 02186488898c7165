"""generative.losses on the MI355X: JukeboxLoss, the spectral loss, on the Fourier kernels of csrc/spectral.hip (forward and gradient), and
PatchAdversarialLoss on gm_patch_adv_loss (csrc/adversarial_loss.hip)."""
from .adversarial_loss import AdversarialCriterions, PatchAdversarialLoss
from .spectral_loss import JukeboxLoss

__all__ = ["AdversarialCriterions", "JukeboxLoss", "PatchAdversarialLoss"]
