"""TEST INFRASTRUCTURE ONLY (CPU, needs the reference tree).  Writes tests/golden/wide_nets.pt: the UNMODIFIED reference's fp32 outputs for the
networks whose attention heads are wider than 256 channels -- the brain / CXR latent-diffusion bundles' UNets, the 3-D DDPM tutorial's UNet, an
AutoencoderKL with a 512-channel non-local attention level.

    python tools/make_golden_wide.py

Weights are restatement.synthetic_state_dict(shapes, seed) on both sides (the fixture stores the shapes and the seed, never the weights), so
the file holds configs, inputs and outputs only.  oracle/ stays as it is; this script only borrows its loader and restatement."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from ref_loader import load_reference  # noqa: E402
from restatement import synthetic_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "wide_nets.pt")

# the brain-image LDM bundle's diffusion_def (model-zoo brain_image_synthesis_latent_diffusion_model, configs/inference.json)
BRAIN = dict(spatial_dims=3, in_channels=7, out_channels=3, num_channels=[256, 512, 768], num_res_blocks=2, attention_levels=[False, True, True],
             norm_num_groups=32, norm_eps=1e-6, resblock_updown=True, num_head_channels=[0, 512, 768], with_conditioning=True,
             transformer_num_layers=1, cross_attention_dim=4, upcast_attention=True, use_flash_attention=False)
# the CXR LDM bundle's UNet (cxr_image_synthesis_latent_diffusion_model, configs/inference.json)
CXR = dict(spatial_dims=2, in_channels=3, out_channels=3, num_channels=[256, 512, 768], num_res_blocks=2, attention_levels=[False, True, True],
           norm_num_groups=32, norm_eps=1e-6, resblock_updown=False, num_head_channels=[0, 512, 768], with_conditioning=True,
           transformer_num_layers=1, cross_attention_dim=1024)
# tutorials/generative/3d_ddpm/3d_ddpm_tutorial.py
TUTORIAL = dict(spatial_dims=3, in_channels=1, out_channels=1, num_channels=[256, 256, 512], attention_levels=[False, False, True],
                num_head_channels=[0, 0, 512], num_res_blocks=2)
AEKL = dict(spatial_dims=2, in_channels=1, out_channels=1, num_channels=(64, 128, 512), attention_levels=(False, False, True), latent_channels=4,
            num_res_blocks=1)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def main():
    gen = load_reference()
    if gen is None:
        raise SystemExit("the reference tree is not present")
    nets = gen.networks.nets
    cases = {}
    unets = {
        "brain": (BRAIN, 701, (1, 7, 8, 12, 8), (1, 1, 4), [999, 17]),
        "tutorial": (TUTORIAL, 702, (1, 1, 16, 20, 16), None, [500]),
        "cxr": (CXR, 703, (1, 3, 24, 24), (1, 77, 1024), [321]),
    }
    with torch.no_grad():
        for i, (name, (cfg, seed, xshape, cshape, ts)) in enumerate(unets.items()):
            m = nets.DiffusionModelUNet(**cfg).eval()
            shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
            m.load_state_dict(synthetic_state_dict(shapes, seed=seed))
            x = _randn(xshape, 10 * seed + 1)
            ctx = _randn(cshape, 10 * seed + 2) if cshape else None
            ys = [m(x, torch.tensor([t], dtype=torch.long), context=ctx) for t in ts]
            cases[name] = dict(kind="unet", cfg=cfg, shapes=shapes, synthetic_seed=seed,
                               inputs=dict(x=x, timesteps=ts, context=ctx), outputs=dict(y=ys))
            print(name, sum(torch.Size(s).numel() for s in shapes.values()), "parameters", [float(y.abs().max()) for y in ys])
            del m
        m = nets.AutoencoderKL(**AEKL).eval()
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict(synthetic_state_dict(shapes, seed=704))
        x = _randn((1, 1, 64, 48), 7041)
        mu, sigma = m.encode(x)
        rec = m.decode(mu)
        cases["aekl"] = dict(kind="aekl", cfg=AEKL, shapes=shapes, synthetic_seed=704, inputs=dict(x=x),
                             outputs=dict(z_mu=mu, z_sigma=sigma, reconstruction=rec))
        print("aekl", tuple(mu.shape), float(rec.abs().max()))
    torch.save(dict(kind="wide_nets", cases=cases), OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
