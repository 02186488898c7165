"""MI355X: timings of the wide-head attention kernel (csrc/attention_wide.hip) and of the reference's wide networks, random-init weights
(nothing from oracle/ or the fixtures).  Reported numbers, no bar.

    python tools/bench_wide_nets.py [--skip-nets]

Prints: wide-head attention us per call beside the head-dim-256 kernel at the same token counts (and the per-FLOP ratio); the brain-bundle UNet
forward (graph-replayed) and the DDIM-50 sample + AutoencoderKL decode seconds per volume; the 3-D DDPM tutorial network's step rate at
1x1x32x40x32 beside BASELINE.md's 16.2 / 4.44 it/s (an anecdote on unknown hardware)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from generativemodels_amd import ops  # noqa: E402
from generativemodels_amd.networks import nets  # noqa: E402

DEV = "cuda"


def _time(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters * 1e3  # us


def attention_table():
    print("# wide-head attention, us per call (B=1); dh=256 reference row at the same tokens and channel count split into 256-wide heads")
    print(f"{'shape':34s} {'dtype':5s} {'wide us':>9s} {'dh256 us':>9s} {'per-FLOP ratio':>15s}")
    for lq, lk, dh in ((1400, 1400, 512), (175, 175, 768), (1400, 1, 512), (1024, 1024, 512), (256, 256, 768), (1024, 77, 512), (256, 77, 768),
                       (640, 640, 512)):
        for dt in (torch.bfloat16, torch.float32):
            g = torch.Generator(device=DEV).manual_seed(0)
            q = torch.randn((1, lq, dh), device=DEV, generator=g).to(dt)
            k = torch.randn((1, lk, dh), device=DEV, generator=g).to(dt)
            v = torch.randn((1, lk, dh), device=DEV, generator=g).to(dt)
            wide = _time(lambda: ops.attention(q, k, v, 1, dh ** -0.5))
            # the same tensors as dh/256 heads of 256: the same FLOPs on the single-pass kernel
            narrow = _time(lambda: ops.attention(q, k, v, dh // 256, 256 ** -0.5)) if dh % 256 == 0 else float("nan")
            print(f"{f'Lq {lq} Lk {lk} dh {dh}':34s} {str(dt)[6:]:5s} {wide:9.1f} {narrow:9.1f} {wide / narrow:15.2f}")


def unet_rows():
    from generativemodels_amd.inferers import DiffusionInferer
    from generativemodels_amd.networks.schedulers import DDIMScheduler, DDPMScheduler
    brain = dict(spatial_dims=3, in_channels=7, out_channels=3, num_channels=[256, 512, 768], num_res_blocks=2, attention_levels=[False, True, True],
                 norm_num_groups=32, norm_eps=1e-6, resblock_updown=True, num_head_channels=[0, 512, 768], with_conditioning=True,
                 transformer_num_layers=1, cross_attention_dim=4, upcast_attention=True)
    ae_cfg = dict(spatial_dims=3, in_channels=1, out_channels=1, latent_channels=3, num_channels=[64, 128, 128, 128], num_res_blocks=2,
                  norm_num_groups=32, norm_eps=1e-6, attention_levels=[False, False, False, False], with_encoder_nonlocal_attn=False,
                  with_decoder_nonlocal_attn=False)
    tut = dict(spatial_dims=3, in_channels=1, out_channels=1, num_channels=[256, 256, 512], attention_levels=[False, False, True],
               num_head_channels=[0, 0, 512], num_res_blocks=2)
    for dt in (torch.bfloat16, torch.float32):
        torch.manual_seed(0)
        m = nets.DiffusionModelUNet(**brain).eval().to(DEV, dt)
        ae = nets.AutoencoderKL(**ae_cfg).eval().to(DEV, dt)
        x = torch.randn((1, 7, 20, 28, 20), device=DEV).to(dt)
        cond = torch.randn((1, 1, 4), device=DEV).to(dt)
        ts = torch.tensor([500], device=DEV)
        with torch.no_grad():
            g = torch.cuda.CUDAGraph()
            m(x, ts, context=cond)
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                m(x, ts, context=cond)
            fwd = _time(g.replay, iters=20) / 1e3
            sched = DDIMScheduler(1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0205, clip_sample=False)
            sched.set_timesteps(50)

            # the bundle's loop: the UNet sees cat(latent, conditions broadcast over the volume), context = conditions
            class _Cat(torch.nn.Module):
                def forward(self, x_, timesteps, context=None):
                    cv = cond.reshape(1, 4, 1, 1, 1).expand(1, 4, *x_.shape[2:]).contiguous()
                    return m(torch.cat([x_, cv], 1), timesteps, context=cond)

            def sample():
                noise = torch.randn((1, 3, 20, 28, 20), device=DEV).to(dt)
                img = noise
                for t in sched.timesteps:
                    out = _Cat()(img, torch.tensor([int(t)], device=DEV))
                    img, _ = sched.step(out, int(t), img)
                return ae.decode(img)
            sample()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sample()
            torch.cuda.synchronize()
            vol = time.perf_counter() - t0
        print(f"brain-bundle UNet {str(dt)[6:]}: forward (graph replay) {fwd:.3f} ms; DDIM-50 sample + AEKL decode {vol:.3f} s per volume")
        del m, ae, g
        torch.cuda.empty_cache()
        m = nets.DiffusionModelUNet(**tut).eval().to(DEV, dt)
        sched = DDPMScheduler(1000)
        noise = torch.randn((1, 1, 32, 40, 32), device=DEV).to(dt)
        inf = DiffusionInferer(sched, use_hip_graph=True)
        with torch.no_grad():
            sched.set_timesteps(20)
            inf.sample(noise, m, sched, verbose=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inf.sample(noise, m, sched, verbose=False)
            torch.cuda.synchronize()
            its = 20 / (time.perf_counter() - t0)
        ref = 16.2 if dt == torch.bfloat16 else 4.44
        print(f"3-D DDPM tutorial UNet {str(dt)[6:]}: {its:.1f} it/s at 1x1x32x40x32 (BASELINE.md anecdote {ref} it/s, hardware unknown)")
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-nets", action="store_true")
    a = ap.parse_args()
    attention_table()
    if not a.skip_nets:
        unet_rows()
