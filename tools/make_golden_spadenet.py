"""TEST INFRASTRUCTURE ONLY (CPU, needs the reference tree).  Writes tests/golden/spadenet.pt: the UNMODIFIED reference's SPADENet on four small
configurations -- encoder outputs, decode(seg, z), the KLD term, its own bf16 error, and every parameter gradient from an fp64 run.

    python tools/make_golden_spadenet.py

Weights are restatement.synthetic_state_dict(shapes, seed) ROUNDED TO bf16-REPRESENTABLE VALUES on both sides (the fixture stores the shapes and
the seed, never the weights); the inputs are bf16-representable too.  The rounding keeps pre-activations away from the LeakyReLU kinks, where one
flipped sign makes a reference's own fp32 autograd differ from fp64 by far more than rounding noise; with it the fp32 reference gradients of all
four cases are within 7.5e-5 * max(1, |g|max) of the fp64 ones.  The script refuses to write a fixture in which any tensor exceeds 2e-4 of that
scale.  oracle/ stays as it is; this script only borrows its loader
and restatement."""
import copy
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from ref_loader import load_reference  # noqa: E402
from restatement import synthetic_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spadenet.pt")
BATCH = 2
CASES = {
    "a2d": (811, dict(spatial_dims=2, in_channels=1, out_channels=1, label_nc=3, input_shape=[16, 16], num_channels=[8, 16], z_dim=8,
                      spade_intermediate_channels=16)),
    "b3d": (812, dict(spatial_dims=3, in_channels=1, out_channels=1, label_nc=3, input_shape=[8, 8, 8], num_channels=[8, 16], z_dim=8,
                      spade_intermediate_channels=16)),
    "c2d": (813, dict(spatial_dims=2, in_channels=2, out_channels=3, label_nc=4, input_shape=[16, 24], num_channels=[8, 8, 12], z_dim=5,
                      spade_intermediate_channels=8)),
    "d3d": (814, dict(spatial_dims=3, in_channels=1, out_channels=2, label_nc=2, input_shape=[16, 8, 24], num_channels=[16, 16], z_dim=4,
                      spade_intermediate_channels=8)),
}
GUARD = 2e-4


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf16_values(t):
    return t.bfloat16().float()


def rounded_state_dict(shapes, seed):
    return {k: _bf16_values(v) for k, v in synthetic_state_dict(shapes, seed=seed).items()}


def _model(nets, cfg, sd, dtype):
    m = nets.SPADENet(**copy.deepcopy(cfg))  # (the reference reverses and extends cfg["num_channels"] in place)
    m.load_state_dict(sd)
    return m.to(dtype)


def _loss_and_grads(m, x, seg, eps, w):
    m.train()
    for p in m.parameters():
        p.grad = None
    mu, logvar = m.encoder(x)
    z = mu + eps * torch.exp(0.5 * logvar)
    y = m.decode(seg, z)
    loss = (y * w).sum() + m.kld_loss(mu, logvar)
    loss.backward()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def main():
    gen = load_reference()
    if gen is None:
        raise SystemExit("the reference tree is not present")
    nets = gen.networks.nets
    torch.manual_seed(0)
    cases = {}
    for name, (seed, cfg) in CASES.items():
        sp = cfg["input_shape"]
        shapes = {k: tuple(v.shape) for k, v in nets.SPADENet(**copy.deepcopy(cfg)).state_dict().items()}
        sd = rounded_state_dict(shapes, seed)
        x = _bf16_values(torch.randn((BATCH, cfg["in_channels"], *sp), generator=_gen(10 * seed + 1)))
        labels = torch.randint(0, cfg["label_nc"], (BATCH, *sp), generator=_gen(10 * seed + 2))
        seg = torch.nn.functional.one_hot(labels, cfg["label_nc"]).movedim(-1, 1).float().contiguous()
        eps = _bf16_values(torch.randn((BATCH, cfg["z_dim"]), generator=_gen(10 * seed + 3)))
        w = _bf16_values(torch.randn((BATCH, cfg["out_channels"], *sp), generator=_gen(10 * seed + 4)))

        m32 = _model(nets, cfg, sd, torch.float32).eval()
        with torch.no_grad():
            mu, logvar = m32.encoder(x)
            z = mu + eps * torch.exp(0.5 * logvar)
            y = m32.decode(seg, z)
            kld = m32.kld_loss(mu, logvar)
            m16 = _model(nets, cfg, sd, torch.bfloat16).eval()
            y16 = m16.decode(seg.bfloat16(), z.bfloat16()).float()
        err = (y16 - y).abs()
        bf16 = dict(mean_err=err.mean().item(), max_err=err.max().item(), sigma=y.std().item())

        g64 = _loss_and_grads(_model(nets, cfg, sd, torch.float64), x.double(), seg.double(), eps.double(), w.double())
        g32 = _loss_and_grads(m32, x, seg, eps, w)
        worst = 0.0
        for k, g in g64.items():
            rel = (g32[k].double() - g).abs().max().item() / max(1.0, g.abs().max().item())
            worst = max(worst, rel)
            if rel > GUARD:
                raise SystemExit(f"{name}: the fp32 reference gradient of {k} is {rel:.3e} (relative to max(1, |g|max)) from fp64: above {GUARD:g}, "
                                 "not a sound fixture")
        case = dict(cfg=cfg, shapes=shapes, synthetic_seed=seed, weights_rounded_to="bfloat16",
                    inputs=dict(x=x, labels=labels.to(torch.uint8), eps=eps, w=w),  # seg = one_hot(labels) over dim 1, as floats
                    outputs=dict(mu=mu, logvar=logvar, z=z, y=y, kld=kld),
                    bf16=bf16, grads={k: g.float() for k, g in g64.items()}, fp32_grad_err=worst)
        if name == "a2d":
            gb = _loss_and_grads(_model(nets, cfg, sd, torch.bfloat16), x.bfloat16(), seg.bfloat16(), eps.bfloat16(), w.bfloat16())
            keys = sorted(g64)
            d = torch.cat([(gb[k].double() - g64[k]).flatten() for k in keys])
            r = torch.cat([g64[k].flatten() for k in keys])
            case["bf16_grad_rel_l2"] = (d.norm() / r.norm()).item()
            per_tensor = [(gb[k].double() - g64[k]).abs().max().item() / max(1.0, g64[k].abs().max().item()) for k in keys]
            case["bf16_grad_per_tensor_max"] = max(per_tensor)
        cases[name] = case
        print(name, sum(torch.Size(s).numel() for s in shapes.values()), "parameters; |y|max", float(y.abs().max()), "kld", float(kld), "bf16", bf16,
              "fp32 grad err", f"{worst:.2e}", "bf16 grad rel L2", case.get("bf16_grad_rel_l2"))
    torch.save(dict(kind="spadenet", cases=cases), OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
