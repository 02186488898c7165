"""PatchAdversarialLoss for MI355X: arguments, errors, the generator-side warning and the return values of the reference's
generative/losses/adversarial_loss.py, over the outputs of a (multi-scale) patch discriminator.

Per discriminator output one launch of gm_patch_adv_loss does the criterion's activation (sigmoid for bce, tanh for hinge, LeakyReLU(0.05) or none
for least squares), the criterion (BCE with torch's -100 log clamp, squared error, -mean(min(+-a - 1, 0))), the mean or sum as a fixed-order fp64
fold, and -- in the backward -- the gradient with respect to the logits scaled by the upstream scalar.  The combination over the outputs (the mean or
sum of the stacked per-output values) is a handful of scalars and stays in torch.

Values are fp32 scalars whatever the logits' dtype (the reference returns the logits' dtype); reduction="none" returns what the reference returns:
element-wise tensors for bce / least squares, the per-output mean for hinge, one list entry per discriminator output."""
from __future__ import annotations

import warnings
from enum import Enum

import torch
from torch.nn.modules.loss import _Loss

from .. import ops

__all__ = ["AdversarialCriterions", "PatchAdversarialLoss"]


class AdversarialCriterions(str, Enum):
    BCE = "bce"
    HINGE = "hinge"
    LEAST_SQUARE = "least_squares"

    def __str__(self) -> str:
        return self.value

    def __repr__(self) -> str:
        return self.value


class PatchAdversarialLoss(_Loss):
    """Drop-in for generative.losses.PatchAdversarialLoss.

    Args:
        reduction: "none", "mean" (default) or "sum".
        criterion: "bce", "hinge" or "least_squares"; the matching activation is applied inside the loss, so the discriminator output must not have
            gone through one.
        no_activation_leastsq: least squares without its LeakyReLU(0.05)."""

    def __init__(self, reduction: str = "mean", criterion: str = AdversarialCriterions.LEAST_SQUARE.value, no_activation_leastsq: bool = False) -> None:
        reduction = str(getattr(reduction, "value", reduction))
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(f"'{reduction}' is not a valid LossReduction")
        super().__init__(reduction=reduction)
        if criterion.lower() not in [m.value for m in AdversarialCriterions]:
            raise ValueError(
                "Unrecognised criterion entered for Adversarial Loss. Must be one in: %s"
                % ", ".join([m.value for m in AdversarialCriterions])
            )
        self.real_label = 1.0
        self.fake_label = -1.0 if criterion == AdversarialCriterions.HINGE.value else 0.0
        self.criterion = str(getattr(criterion, "value", criterion))
        self.activation = not (self.criterion == AdversarialCriterions.LEAST_SQUARE.value and no_activation_leastsq)
        self.reduction = reduction

    def forward(self, input: torch.Tensor | list, target_is_real: bool, for_discriminator: bool) -> torch.Tensor | list[torch.Tensor]:
        """input: the output of a PatchDiscriminator (a tensor) or of a MultiScalePatchDiscriminator (a list), without a final activation.
        target_is_real: whether it stands for real (or wannabe-real) images; for_discriminator: the discriminator's loss or the generator's -- for
        the generator the target is always real.  -> the mean / sum over elements and outputs, or with reduction="none" a list with one entry per output."""
        if not for_discriminator and not target_is_real:
            target_is_real = True  # With generator, we always want this to be true!
            warnings.warn(
                "Variable target_is_real has been set to False, but for_discriminator is set"
                "to False. To optimise a generator, target_is_real must be set to True."
            )
        if type(input) is not list:
            input = [input]
        from .. import autograd as A

        hinge = self.criterion == AdversarialCriterions.HINGE.value
        loss = []
        for disc_out in input:
            ops.require_device(disc_out)
            target = self.real_label if target_is_real else self.fake_label
            reduction = "mean" if hinge else self.reduction  # (the hinge criterion is the mean of its output whatever the reduction)
            if torch.is_grad_enabled() and disc_out.requires_grad:
                loss.append(A.patch_adv_loss(disc_out, self.criterion, target, self.activation, reduction))
            else:
                loss.append(ops.patch_adv_loss(disc_out.detach(), self.criterion, target, self.activation, reduction))
        if self.reduction == "mean":
            return torch.mean(torch.stack(loss))
        if self.reduction == "sum":
            return torch.sum(torch.stack(loss))
        return loss
