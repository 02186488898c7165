"""Classifier guidance (Wolleb et al., "Diffusion Models for Medical Anomaly Detection"; the reference's
tutorials/generative/anomaly_detection/anomalydetection_tutorial_classifier_guidance.py): the gradient of log p(y | x_t) of a
DiffusionModelEncoder with respect to the noisy image, which the sampling loop adds to the predicted noise at every step."""
from __future__ import annotations

import torch

from .. import ops
from ..networks.nets.diffusion_model_unet import DiffusionModelEncoder, _detached_view

__all__ = ["classifier_guidance_gradient"]


def classifier_guidance_gradient(classifier: DiffusionModelEncoder, x: torch.Tensor, timesteps: torch.Tensor, y: torch.Tensor,
                                 context: torch.Tensor | None = None, class_labels: torch.Tensor | None = None) -> torch.Tensor:
    """The tutorial's

        x_in = x.detach().requires_grad_(True)
        log_probs = F.log_softmax(classifier(x_in, timesteps), dim=-1)
        a = torch.autograd.grad(log_probs[range(len(y)), y.view(-1)].sum(), x_in)[0]

    in one call, bit for bit the same result, in the shape and dtype of x.  The head runs outside autograd: gm_head_hidden, gm_head_tail (logits),
    the logit gradient onehot(y) - softmax(logits) from torch's own log-softmax forward and backward over the (N, K) logits (the kernels the lines above
    run, which is what makes the results identical), gm_head_tail (da) and gm_head_dinput.  Only the encoder half records a graph -- of native Functions, with the parameters as
    constants -- and its backward runs the data-gradient kernels alone: no weight, bias or affine gradient is computed."""
    if not isinstance(classifier, DiffusionModelEncoder):
        raise TypeError("classifier_guidance_gradient expects a DiffusionModelEncoder")
    classifier._check(x, timesteps, context, class_labels)  # (argument errors first: nothing is launched before they pass)
    ops.require_device(x, y)
    y = y.reshape(-1).to(torch.int64)
    if y.shape[0] != x.shape[0]:
        raise ValueError(f"classifier_guidance_gradient: {y.shape[0]} labels for a batch of {x.shape[0]}")
    net = _detached_view(classifier)  # the parameters as detached tensors: the recorded graph has the input as its only leaf
    l0, l3 = net.out[0], net.out[3]
    x_in = x.detach().requires_grad_(True)
    with torch.enable_grad():
        h = net._encode_arena_train(x_in, timesteps, context, class_labels)
    with torch.no_grad():
        feat = h.detach()
        mask = classifier._dropout_mask(feat.shape[0], feat.dtype, feat.device)
        head = ops.classifier_head(feat, l0.weight, l0.bias, l3.weight, l3.bias, mask)
        with torch.enable_grad():  # three torch nodes over the (N, K) logits: the very kernels the tutorial's lines run, through public API only
            logits = head.logits.detach().requires_grad_(True)
            log_probs = torch.log_softmax(logits, dim=-1)
            g = torch.autograd.grad(log_probs[range(len(logits)), y].sum(), logits)[0]
        dh, _ = ops.classifier_head_backward(feat, head.a, mask, l0.weight, l3.weight, g=g)
    return torch.autograd.grad(h, x_in, grad_outputs=dh)[0]
