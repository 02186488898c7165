"""Shared by the metric tests and tools/make_golden_metrics.py (test infrastructure): the input recipes of tests/golden/metrics.pt and
restatements of SSIM / MS-SSIM / MMD in a chosen precision -- fp64 is the yardstick of the GPU tests, fp32 the separable CPU evaluation whose
distance to fp64 the fixture records.  Everything here is plain torch on the CPU."""
import math

import torch
import torch.nn.functional as F


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def make_pair(recipe):
    """recipe: dict(shape, seed, smoothing, noise, data_range=1.0, identical=False) -> (y_pred, y) fp32.
    y is a random image constant on blocks of `smoothing` voxels per axis (structure at the scale of the SSIM windows), y_pred is y plus
    uniform noise of amplitude `noise`, both clamped to [0, 1] and scaled by data_range.  Only exactly rounded element-wise fp32 operations and
    the CPU generator are involved: the same bits on every machine (the fixture carries a checksum)."""
    shape, s = tuple(recipe["shape"]), int(recipe["smoothing"])
    g = torch.Generator().manual_seed(int(recipe["seed"]))
    coarse = tuple(shape[:2]) + tuple(-(-n // s) for n in shape[2:])
    y = torch.rand(coarse, generator=g, dtype=torch.float32)
    for ax in range(2, len(shape)):
        y = y.repeat_interleave(s, dim=ax).narrow(ax, 0, shape[ax])
    # a ramp along the last axis so that blocks are not flat (a flat window has zero variance: SSIM would rest on c2 alone)
    ramp = torch.arange(shape[-1], dtype=torch.float32) / float(2 * shape[-1])
    y = (y * 0.5 + ramp).contiguous()
    if recipe.get("identical", False):
        y_pred = y.clone()
    else:
        u = torch.rand(shape, generator=g, dtype=torch.float32)
        y_pred = (y + float(recipe["noise"]) * (u - 0.5)).clamp(0.0, 1.0)
    r = float(recipe.get("data_range", 1.0))
    return y_pred * r, y * r


def checksum(*tensors):
    """fp64 sum of position-weighted values: sensitive to any changed or moved element."""
    tot = 0.0
    for t in tensors:
        v = t.double().flatten()
        w = (torch.arange(v.numel(), dtype=torch.float64) % 8191.0) + 1.0
        tot += float((v * w).sum())
    return tot


def make_features(recipe):
    """recipe: dict(shape=(n, f), seed, rank=None) -> two (n, f) fp64 feature matrices with different means and covariances."""
    n, f = recipe["shape"]
    g = torch.Generator().manual_seed(int(recipe["seed"]))
    mix_a = torch.randn((f, f), generator=g, dtype=torch.float64) / math.sqrt(f)
    mix_b = torch.randn((f, f), generator=g, dtype=torch.float64) / math.sqrt(f)
    a = torch.randn((n, f), generator=g, dtype=torch.float64) @ mix_a
    b = torch.randn((n, f), generator=g, dtype=torch.float64) @ mix_b * 1.3 + 0.25
    return a, b


# ---- windows ---------------------------------------------------------------------------------------------------------------------------
def gaussian_table(size, sigma):
    """fp32 Gaussian taps at the `size` unit-spaced points centred on zero, normalised in fp32."""
    d = torch.arange(size, dtype=torch.float32) - (size - 1) / 2
    g = torch.exp(-((d / sigma) ** 2) / 2)
    return g / g.sum()


def tap_tables(kernel_type, sizes, sigmas):
    if kernel_type == "gaussian":
        return [gaussian_table(k, s) for k, s in zip(sizes, sigmas)]
    return [torch.full((k,), 1.0 / k, dtype=torch.float32) for k in sizes]


# ---- restatements ------------------------------------------------------------------------------------------------------------------------
def _separable(t, taps, dtype):
    """"valid" cross-correlation of (B, C, *spatial) with the outer product of the 1-D tables, one axis at a time."""
    b, c = t.shape[:2]
    nsp = t.dim() - 2
    conv = F.conv3d if nsp == 3 else F.conv2d
    t = t.reshape(b * c, 1, *t.shape[2:])
    for ax, tap in enumerate(taps):
        shape = [1, 1] + [1] * nsp
        shape[2 + ax] = len(tap)
        t = conv(t, tap.to(dtype).reshape(shape))
    return t.reshape(b, c, *t.shape[2:])


def ssim_cs_maps(y_pred, y, taps, c1, c2, dtype=torch.float64):
    x, y = y_pred.to(dtype), y.to(dtype)
    mu_x, mu_y = _separable(x, taps, dtype), _separable(y, taps, dtype)
    mu_xx, mu_yy, mu_xy = _separable(x * x, taps, dtype), _separable(y * y, taps, dtype), _separable(x * y, taps, dtype)
    sigma_x = mu_xx - mu_x * mu_x
    sigma_y = mu_yy - mu_y * mu_y
    sigma_xy = mu_xy - mu_x * mu_y
    cs = (2 * sigma_xy + c2) / (sigma_x + sigma_y + c2)
    ssim = ((2 * mu_x * mu_y + c1) / (mu_x ** 2 + mu_y ** 2 + c1)) * cs
    return ssim, cs


def constants(data_range, k1=0.01, k2=0.03):
    return (k1 * data_range) ** 2, (k2 * data_range) ** 2


def ssim_case(y_pred, y, p, dtype=torch.float64, want_maps=False):
    """p: dict(kernel_type, kernel_size, kernel_sigma, data_range) -> dict(ssim (B,), cs (B,) [, ssim_map, cs_map]) in `dtype`."""
    taps = tap_tables(p["kernel_type"], p["kernel_size"], p["kernel_sigma"])
    c1, c2 = constants(p["data_range"])
    ssim, cs = ssim_cs_maps(y_pred, y, taps, c1, c2, dtype)
    out = dict(ssim=ssim.flatten(1).mean(1), cs=cs.flatten(1).mean(1))
    if want_maps:
        out.update(ssim_map=ssim, cs_map=cs)
    return out


def ms_ssim_case(y_pred, y, p, dtype=torch.float64):
    """-> (B,) multi-scale SSIM in `dtype`: relu(cs mean) per scale, relu(ssim mean) at the last, product of powers; 2x average pooling between scales."""
    taps = tap_tables(p["kernel_type"], p["kernel_size"], p["kernel_sigma"])
    c1, c2 = constants(p["data_range"])
    pool = F.avg_pool3d if y.dim() == 5 else F.avg_pool2d
    x, y = y_pred.to(dtype), y.to(dtype)
    w = torch.tensor(p["weights"], dtype=torch.float32).to(dtype)
    factors = []
    for i in range(len(w)):
        ssim, cs = ssim_cs_maps(x, y, taps, c1, c2, dtype)
        last = i == len(w) - 1
        factors.append(torch.relu((ssim if last else cs).flatten(1).mean(1)))
        if not last:
            x, y = pool(x, kernel_size=2), pool(y, kernel_size=2)
    return torch.prod(torch.stack(factors) ** w.view(-1, 1), dim=0)


def mmd_case(y, y_pred, dtype=torch.float64):
    """The three Gram-matrix means, literally."""
    y = y.to(dtype).reshape(y.shape[0], -1)
    p = y_pred.to(dtype).reshape(y_pred.shape[0], -1)
    f = y.shape[1]
    return 1.0 * (torch.mean(y @ y.t() / f) + torch.mean(p @ p.t() / f)) - 2.0 * torch.mean(p @ y.t() / f)


MMD_TRANSFORMS = {
    None: None,
    "square_minus_half": lambda t: t * t - 0.5,
    "halve": lambda t: t * 0.5,
}
