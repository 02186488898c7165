"""Shared by tools/make_golden_patchgan.py (which writes tests/golden/patchgan.pt from the unmodified reference) and the PatchGAN tests: the cases, the
recipes of their weights and inputs, the sampling of large tensors, and a plain fp64 restatement of the three adversarial criteria.  No reference code.

Recipes instead of stored tensors.  Weights are restatement.synthetic_state_dict over the case's shapes (0-dim entries skipped), then
running_var = 0.5 + 10 |that| (a variance must be positive) and num_batches_tracked = 3, everything rounded to bf16-representable values; inputs are
bf16-representable normal draws from a seeded CPU generator.  The fixture stores the seed and the fp64 sum of every input, which `make_input` callers
check, so a generator that drew other numbers fails loudly instead of as a parity error.

Conditioning of the loss.  The least-squares criterion puts LeakyReLU(0.05) on the logits: its derivative jumps by a factor of 20 at zero, so one logit
whose sign a bf16 forward flips moves the aggregate gradient error by several per cent (measured: 6 % on 702 logits), in the reference as in any other
implementation.  The fixture script therefore draws the input of a least-squares case from the first candidate seed for which every fp64 logit is at
least KINK_MARGIN times the reference's own mean bf16 error of that logit tensor away from zero.

Sampling.  All returned tensors of all cases, train and eval, plus every gradient are about 3 MB in fp32; a committed file holds at most 1 MiB.  A tensor
of more than SAMPLE_MAX elements is therefore stored as `sample(t)`: every s-th element of the flattened tensor, s odd (so that every residue of the
power-of-two extents is visited), together with the absolute maximum and the sum of the whole tensor.  Both sides of a comparison are sampled the same way."""
import torch

import restatement as R

SAMPLE_MAX = 1024

_P = dict(kind="patch")
_M = dict(kind="multi")
CASES = {
    "a2d": dict(_P, seed=921, cfg=dict(spatial_dims=2, num_channels=8, in_channels=1, out_channels=1, num_layers_d=3), input=(2, 1, 64, 64),
                loss=("mean", "least_squares")),
    "b3d": dict(_P, seed=922, cfg=dict(spatial_dims=3, num_channels=8, in_channels=1, out_channels=1, num_layers_d=2), input=(2, 1, 32, 32, 32),
                loss=("mean", "least_squares")),
    "c2d": dict(_P, seed=923, cfg=dict(spatial_dims=2, num_channels=8, in_channels=3, out_channels=2, num_layers_d=2, last_conv_kernel_size=1, bias=True),
                input=(3, 3, 40, 56), loss=("mean", "least_squares")),
    "d3d": dict(_P, seed=924, cfg=dict(spatial_dims=3, num_channels=4, in_channels=2, out_channels=1, num_layers_d=1, kernel_size=3), input=(2, 2, 16, 12, 20),
                loss=("mean", "least_squares")),
    "e_ms": dict(_M, seed=925, cfg=dict(num_d=2, num_layers_d=1, spatial_dims=2, num_channels=4, in_channels=1, pooling_method="avg", minimum_size_im=32),
                 input=(2, 1, 32, 32), loss=("mean", "least_squares")),
    "f_ms": dict(_M, seed=926, cfg=dict(num_d=2, num_layers_d=1, spatial_dims=2, num_channels=8, in_channels=3, out_channels=3, minimum_size_im=32,
                                        norm="INSTANCE", kernel_size=3), input=(2, 3, 32, 48), loss=("sum", "hinge")),
}
DSTEP_CASE = "a2d"  # the discriminator step runs on this case's network: D(fake) and D(real) before one backward
DSTEP_CRITERIA = ("bce", "hinge", "least_squares")
KINK_MARGIN = 4.0  # |logit| >= KINK_MARGIN * (the reference's mean bf16 forward error of the logits) for every logit of a least-squares case
FEATURE_WEIGHT = 0.1  # loss = adv(out, True, False) + FEATURE_WEIGHT * sum over features of mean(feature^2)


def bf16_values(t):
    return t.bfloat16().float()


def make_state_dict(shapes, seed):
    """The case's weights from its state_dict shapes (key -> shape, 0-dim entries included)."""
    sd = R.synthetic_state_dict({k: s for k, s in shapes.items() if len(s) > 0}, seed=seed)
    out = {}
    for k, s in shapes.items():
        if len(s) == 0:
            out[k] = torch.tensor(3, dtype=torch.long)  # num_batches_tracked
        elif k.endswith("running_var"):
            out[k] = bf16_values(0.5 + 10.0 * sd[k].abs())
        else:
            out[k] = bf16_values(sd[k])
    return out


def make_input(shape, seed):
    return bf16_values(torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)))


def candidate_input_seeds(name):
    """The input seeds tools/make_golden_patchgan.py tries in order; the fixture records the first one whose logits stay clear of the kink of the
    least-squares activation (`input_seed`), which is the one the tests draw."""
    return (10 * CASES[name]["seed"] + 1 + 1000 * k for k in range(200000))


def case_input(name, seed):
    return make_input(CASES[name]["input"], seed)


def dstep_fake():
    return make_input(CASES[DSTEP_CASE]["input"], 10 * CASES[DSTEP_CASE]["seed"] + 2)


def sample(t):
    """The stored form of a tensor: itself (flattened) up to SAMPLE_MAX elements, else every s-th element, s odd."""
    flat = t.detach().reshape(-1)
    if flat.numel() <= SAMPLE_MAX:
        return flat
    return flat[::(flat.numel() // SAMPLE_MAX) | 1]


def record(t, dtype=torch.float32):
    """What the fixture keeps of a reference tensor."""
    t = t.detach()
    return dict(shape=tuple(t.shape), sample=sample(t).to(dtype).clone(), absmax=float(t.abs().max()) if t.numel() else 0.0, sum=float(t.double().sum()))


def flatten_outputs(kind, returned):
    """The returned structure as one flat list of tensors and the index lists of its (outputs, features)."""
    if kind == "patch":
        tensors = list(returned)
        return tensors, [len(tensors) - 1], list(range(len(tensors) - 1))
    outs, feats = returned
    tensors, oi, fi = [], [], []
    for o, fs in zip(outs, feats):
        for f in fs:
            fi.append(len(tensors))
            tensors.append(f)
        oi.append(len(tensors))
        tensors.append(o)
    return tensors, oi, fi


def training_loss(kind, returned, adv):
    """adv(out, True, False) + FEATURE_WEIGHT * sum of mean(feature^2); `adv` is a PatchAdversarialLoss."""
    tensors, oi, fi = flatten_outputs(kind, returned)
    out = tensors[oi[0]] if kind == "patch" else [tensors[i] for i in oi]
    loss = adv(out, True, False)
    for i in fi:
        loss = loss + FEATURE_WEIGHT * tensors[i].pow(2).mean()
    return loss


# ---- the three criteria, restated in fp64 on plain tensors ----------------------------------------------------------------------------------------
def criterion_terms(x, criterion, target_is_real, no_activation_leastsq=False):
    """Per-logit terms of PatchAdversarialLoss in fp64 (x: any tensor of logits)."""
    x = x.double()
    if criterion == "bce":
        a = torch.sigmoid(x)
        t = 1.0 if target_is_real else 0.0
        return -(t * torch.log(a).clamp_min(-100.0) + (1.0 - t) * torch.log(1.0 - a).clamp_min(-100.0))
    if criterion == "hinge":
        a = torch.tanh(x)
        return -torch.minimum((a if target_is_real else -a) - 1.0, torch.zeros_like(a))
    a = x if no_activation_leastsq else torch.where(x > 0, x, 0.05 * x)
    return (a - (1.0 if target_is_real else 0.0)) ** 2


def criterion_value(outputs, criterion, target_is_real, for_discriminator, reduction="mean", no_activation_leastsq=False):
    """PatchAdversarialLoss.forward for reduction "mean" / "sum" over a tensor or a list of tensors, in fp64."""
    if not for_discriminator:
        target_is_real = True
    outputs = outputs if isinstance(outputs, list) else [outputs]
    per = []
    for o in outputs:
        terms = criterion_terms(o, criterion, target_is_real, no_activation_leastsq)
        per.append(terms.mean() if criterion == "hinge" or reduction == "mean" else terms.sum())
    stack = torch.stack(per)
    return stack.mean() if reduction == "mean" else stack.sum()


def rel_l2(got, want):
    """Aggregate relative L2 distance of two equally keyed / ordered collections of (sampled) tensors."""
    d = torch.cat([(g.double().reshape(-1).cpu() - w.double().reshape(-1).cpu()) for g, w in zip(got, want)])
    r = torch.cat([w.double().reshape(-1).cpu() for w in want])
    return (d.norm() / r.norm().clamp_min(1e-300)).item()
