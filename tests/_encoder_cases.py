"""Shared by tools/make_golden_encoder.py (which writes tests/golden/encoder.pt from the unmodified reference) and the DiffusionModelEncoder tests: the
cases, the recipes of their weights and inputs, and the classifier-guided DDIM chain.  No reference code.

Recipes instead of stored tensors.  Weights are restatement.synthetic_state_dict over the case's state_dict shapes -- for EVERY parameter: a fresh
encoder has all-zero `conv2` / `proj_out` weights and GroupNorm biases, with which most of the network would drop out of a parity test -- rounded to
bf16-representable values, so that the fp64, fp32 and bf16 runs hold the same numbers.  Inputs, contexts, labels and timesteps come from seeded CPU
generators; the fixture stores the fp64 sum of every input, which the tests check, so a generator that drew other numbers fails loudly.

Every case leaves 4096 features, from an input that is neither square nor cubic (an axis-order mistake in the flatten then shows), and has 16 classes at
batch 4 (2 in 3-D, 1 for the tutorial's own classifier), so that the error statistics rest on 64 logits."""
import torch

import restatement as R

CASES = {
    "a2d": dict(seed=941, cfg=dict(spatial_dims=2, in_channels=1, out_channels=16, num_res_blocks=(1, 1), num_channels=(8, 16),
                                   attention_levels=(False, False), norm_num_groups=8), input=(4, 1, 32, 128)),
    "b2d_attn": dict(seed=942, cfg=dict(spatial_dims=2, in_channels=3, out_channels=16, num_res_blocks=(1, 1), num_channels=(32, 64),
                                        attention_levels=(False, True), num_head_channels=32), input=(4, 3, 16, 64)),
    "c3d": dict(seed=943, cfg=dict(spatial_dims=3, in_channels=1, out_channels=16, num_res_blocks=(1, 1), num_channels=(32, 64),
                                   attention_levels=(False, False)), input=(2, 1, 16, 32, 8)),
    "d2d_cond": dict(seed=944, cfg=dict(spatial_dims=2, in_channels=1, out_channels=16, num_res_blocks=(1, 1), num_channels=(32, 64),
                                        attention_levels=(False, True), num_head_channels=32, with_conditioning=True, cross_attention_dim=16,
                                        num_class_embeds=5, resblock_updown=True), input=(4, 1, 16, 64), context=(4, 1, 16), class_embeds=5),
    # the classifier of the reference's anomaly-detection tutorial, called as there: one image, a float timestep of shape (1,)
    "tut": dict(seed=945, cfg=dict(spatial_dims=2, in_channels=1, out_channels=2, num_channels=(32, 64, 64), attention_levels=(False, True, True),
                                   num_res_blocks=(1, 1, 1), num_head_channels=64, with_conditioning=False), input=(1, 1, 64, 64), float_timestep=True),
}

# ---- the guided chain: the tutorial's loop on a two-level UNet and the a2d-sized classifier ---------------------------------------------------------
CHAIN = dict(classifier="a2d", classifier_seed=951, unet_seed=952, input=(2, 1, 32, 128), input_seed=9531, labels=(3, 11), scale=6.0,
             L=4, stride=50, num_train_timesteps=1000,
             unet=dict(spatial_dims=2, in_channels=1, out_channels=1, num_res_blocks=(1, 1), num_channels=(8, 16), attention_levels=(False, False),
                       norm_num_groups=8, num_head_channels=8))
FP32_BAR = 1e-4   # test_gpu_models._fp32_close: 1e-4 * max(1, |ref|max)
GRAD_BAR = 6e-4   # fp32 gradients: 6e-4 * max(1, |g|max), as in test_gpu_patchgan.py
CHAIN_FACTOR = 2.0  # the existing DDIM chain test's bar: _fp32_close(..., factor=2.0)


def bf16_values(t):
    return t.bfloat16().float()


KINK_MARGIN = 4.0  # every fp64 hidden pre-activation is at least KINK_MARGIN x (the reference's mean bf16 error of the pre-activations) away from zero
HEAD_WEIGHT_SCALE, HEAD_BIAS_OFFSET = 0.25, 1.5


def make_state_dict(shapes, seed):
    """The recipe, with the head's first layer conditioned for a ReLU: out.0.weight is scaled by HEAD_WEIGHT_SCALE (pre-activation spread about 0.3 to
    0.4) and out.0.bias is +-HEAD_BIAS_OFFSET plus the recipe's draw, the sign that of the draw -- half of the 512 units on, half off, none near zero.

    Why.  d relu / dz jumps at zero, and a hidden unit whose sign a bf16 forward flips moves the input gradient by about 1 / sqrt(active units), 6 %.
    With the plain recipe the pre-activations are N(0, 1.2 .. 1.5) and their bf16 error is about 0.006: 10 to 34 of a case's units lie within
    KINK_MARGIN errors of zero, and the reference's OWN bf16 run flips 1 to 4 units per case (measured on the reference, tools/make_golden_encoder.py
    prints both counts).  Its bf16 gradient error -- the yardstick of the bf16 tests -- would then be a lottery over which units flip, in the reference
    as in any other implementation.  The op-level tests exercise the kink itself, on operands that both sides share exactly."""
    sd = {k: bf16_values(v) for k, v in R.synthetic_state_dict(shapes, seed=seed).items()}
    draw = sd["out.0.bias"]
    sd["out.0.weight"] = bf16_values(HEAD_WEIGHT_SCALE * sd["out.0.weight"])
    sd["out.0.bias"] = bf16_values(torch.where(draw >= 0, HEAD_BIAS_OFFSET, -HEAD_BIAS_OFFSET) + draw)
    return sd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def case_input(name):
    c = CASES[name]
    return bf16_values(torch.randn(c["input"], generator=_gen(10 * c["seed"] + 1)))


def case_timesteps(name):
    """Integer timesteps, one per sample; the tutorial's case passes torch.Tensor((t,)): float32 of shape (1,)."""
    c = CASES[name]
    if c.get("float_timestep"):
        return torch.Tensor((37,))
    return torch.randint(0, 1000, (c["input"][0],), generator=_gen(10 * c["seed"] + 2))


def case_labels(name):
    c = CASES[name]
    return torch.randint(0, c["cfg"]["out_channels"], (c["input"][0],), generator=_gen(10 * c["seed"] + 3))


def case_context(name):
    c = CASES[name]
    return bf16_values(torch.randn(c["context"], generator=_gen(10 * c["seed"] + 4))) if "context" in c else None


def case_class_labels(name):
    c = CASES[name]
    return torch.randint(0, c["class_embeds"], (c["input"][0],), generator=_gen(10 * c["seed"] + 5)) if "class_embeds" in c else None


def case_kwargs(name, device=None, dtype=None):
    """context / class_labels keyword arguments of the case's forward."""
    kw = {}
    ctx, cl = case_context(name), case_class_labels(name)
    if ctx is not None:
        kw["context"] = ctx.to(device=device, dtype=dtype or ctx.dtype)
    if cl is not None:
        kw["class_labels"] = cl.to(device=device)
    return kw


def chain_input():
    """An image-like start in [0, 1] (the schedulers clip the predicted x_0 to [-1, 1])."""
    return bf16_values(torch.rand(CHAIN["input"], generator=_gen(CHAIN["input_seed"])))


def guided_chain(unet, classifier, scheduler, x, labels, gradient=None):
    """The tutorial's loop: L reversed DDIM steps (encoding), then L DDIM steps whose predicted noise is moved along the classifier's gradient,
    model_output - sqrt(1 - abar_t) * scale * a.  gradient(x, t_tensor) -> a; None: the tutorial's own autograd lines; False: no guidance.
    `scheduler` has had set_timesteps(num_train_timesteps // stride)."""
    import torch.nn.functional as F

    L, stride, scale = CHAIN["L"], CHAIN["stride"], CHAIN["scale"]
    cur = x
    for k in range(L):
        t = k * stride
        with torch.no_grad():
            out = unet(cur, timesteps=torch.Tensor((t,)).to(cur.device))
        cur, _ = scheduler.reversed_step(out, t, cur)
    for k in range(L):
        t = (L - k) * stride
        tt = torch.Tensor((t,)).to(cur.device)
        with torch.no_grad():
            out = unet(cur, timesteps=tt).detach()
        if gradient is False:
            updated = out
        else:
            if gradient is None:
                with torch.enable_grad():
                    x_in = cur.detach().requires_grad_(True)
                    logits = classifier(x_in, timesteps=tt)
                    log_probs = F.log_softmax(logits, dim=-1)
                    selected = log_probs[range(len(logits)), labels.view(-1)]
                    a = torch.autograd.grad(selected.sum(), x_in)[0]
            else:
                a = gradient(cur, tt)
            alpha_prod_t = scheduler.alphas_cumprod[t]
            updated = out - (1 - alpha_prod_t).sqrt().to(out) * scale * a
        cur, _ = scheduler.step(updated, t, cur)
    return cur


def rel_l2(got, want):
    """Aggregate relative L2 distance of two equally ordered collections of tensors."""
    d = torch.cat([(g.double().reshape(-1).cpu() - w.double().reshape(-1).cpu()) for g, w in zip(got, want)])
    r = torch.cat([w.double().reshape(-1).cpu() for w in want])
    return (d.norm() / r.norm().clamp_min(1e-300)).item()


def err_stats(got, want):
    e = (got.double().cpu() - want.double().cpu()).abs()
    return dict(max_err=e.max().item(), mean_err=e.mean().item())


# ---- large tensors are stored sampled: a committed file holds at most 1 MiB, `out.0.weight`'s gradient alone is 8 MB ------------------------------------
SAMPLE_MAX = 1024


def sample(t):
    """The stored form of a tensor: itself (flattened) up to SAMPLE_MAX elements, else every s-th element, s odd (every residue of the power-of-two
    extents is visited).  Both sides of a comparison are sampled the same way."""
    flat = t.detach().reshape(-1)
    if flat.numel() <= SAMPLE_MAX:
        return flat
    return flat[::(flat.numel() // SAMPLE_MAX) | 1]


def record(t, dtype=torch.float32):
    """What the fixture keeps of a reference tensor: the sample, and the absolute maximum and sum of the whole tensor."""
    t = t.detach()
    return dict(shape=tuple(t.shape), sample=sample(t).to(dtype).clone(), absmax=float(t.abs().max()), sum=float(t.double().sum()))
