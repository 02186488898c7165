"""Frechet inception distance between two sets of feature vectors (Heusel et al. 2017).  Host arithmetic in fp64 on (images, features)
matrices -- a few hundred numbers per side, no kernel.  tr(sqrtm(Sx Sy)) is the sum of the square roots of the eigenvalues of Sx Sy, which
are real and non-negative for covariance matrices up to rounding; no matrix square root is formed."""
from __future__ import annotations

import torch

from ._base import Metric


class FIDMetric(Metric):
    """`FIDMetric()(y_pred, y)` with y_pred, y of shape (number of images, number of features)."""

    def __call__(self, y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return get_fid_score(y_pred, y)


def _cov(samples: torch.Tensor) -> torch.Tensor:
    """Covariance of the columns of a (observations, variables) matrix, normalised by observations - 1."""
    rows = samples.t() if samples.size(0) != 1 else samples
    factor = 1.0 / (rows.size(1) - 1)
    rows = rows - torch.mean(rows, dim=1, keepdim=True)
    return factor * rows.matmul(rows.t()).squeeze()


def compute_frechet_distance(mu_x: torch.Tensor, sigma_x: torch.Tensor, mu_y: torch.Tensor, sigma_y: torch.Tensor) -> torch.Tensor:
    diff = mu_x - mu_y
    eig = torch.linalg.eigvals(sigma_x.mm(sigma_y))
    tr_covmean = torch.sqrt(torch.clamp(eig.real, min=0.0)).sum()
    return diff.dot(diff) + torch.trace(sigma_x) + torch.trace(sigma_y) - 2 * tr_covmean


def get_fid_score(y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    if y.dim() > 2 or y_pred.dim() > 2:
        raise ValueError("Inputs should have (number images, number of features) shape.")
    device = y_pred.device
    y = y.detach().double().cpu()
    y_pred = y_pred.detach().double().cpu()
    score = compute_frechet_distance(torch.mean(y_pred, dim=0), _cov(y_pred), torch.mean(y, dim=0), _cov(y))
    return score.to(device)
