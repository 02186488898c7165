"""Measures the PatchGAN discriminators and the BatchNorm passes on the MI355X (needs the GPU: fails without one).

    python tools/bench_patchgan.py [--seconds 0.5] [--rounds 5] [--out FILE]

Two discriminators, fp32 and bf16: the 3-D latent-diffusion tutorial's (spatial_dims 3, num_layers_d 3, num_channels 32) at 2 x 1 x 64^3 and the 2-D one
(num_channels 64) at 16 x 1 x 64 x 64.  Reports
  * forward + backward of one discriminator term (least-squares loss of D(x)[-1], gradients of every parameter) per step: host clock around steps that
    end in a device synchronise, windows of at least --seconds after a warm-up, --rounds windows ALTERNATING with a plain torch.nn restatement of the same
    layers (nn.Conv / nn.BatchNorm / nn.LeakyReLU, written here) on the same GPU; median and [min, max] over the rounds: the spread a difference must exceed;
  * the share of every kernel label in one step (ops.start_profile: device events around each launch);
  * the BatchNorm passes against EXISTING code on the same tensors in the same run: gm_bn_apply against gm_gn_apply, and gm_bn_bwd_stats + gm_bn_bwd_apply
    against gm_gn_bwd_stats + gm_gn_bwd_apply (the [N][C]-table kernels the new ones were modelled on), alternating, with achieved bytes / s from
    shape-computed traffic (apply: read x, write y; backward statistics: read x, gy; backward apply: read x, gy, write dx) as a share of the 8.0 TB/s peak."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
NETS = {"3d": (dict(spatial_dims=3, num_layers_d=3, num_channels=32, in_channels=1, out_channels=1), (2, 1, 64, 64, 64)),
        "2d": (dict(spatial_dims=2, num_layers_d=3, num_channels=64, in_channels=1, out_channels=1), (16, 1, 64, 64))}


def _window(fn, seconds):
    fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        for _ in range(3):
            fn()
        calls += 3
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / calls


def _alternate(fns, seconds, rounds):
    """-> per function (median, min, max) seconds per call over `rounds` windows, the functions taking turns."""
    got = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            got[i].append(_window(fn, seconds))
    return [(statistics.median(g), min(g), max(g)) for g in got]


def _fmt(t):
    return f"{t[0] * 1e3:8.3f} ms [{t[1] * 1e3:.3f}, {t[2] * 1e3:.3f}]"


def torch_restatement(cfg):
    d, nc, k = cfg["spatial_dims"], cfg["num_channels"], 4
    conv, bn = {2: nn.Conv2d, 3: nn.Conv3d}[d], {2: nn.BatchNorm2d, 3: nn.BatchNorm3d}[d]
    layers = [conv(cfg["in_channels"], nc, k, 2, 1), nn.LeakyReLU(0.2)]
    cin, cout = nc, 2 * nc
    for l_ in range(cfg["num_layers_d"]):
        layers += [conv(cin, cout, k, 1 if l_ == cfg["num_layers_d"] - 1 else 2, 1, bias=False), bn(cout), nn.LeakyReLU(0.2)]
        cin, cout = cout, 2 * cout
    layers.append(conv(cin, cfg["out_channels"], k, 1, 1))
    return nn.Sequential(*layers)


def steps(out, seconds, rounds):
    from generativemodels_amd import ops
    from generativemodels_amd.losses import PatchAdversarialLoss
    from generativemodels_amd.networks.nets import PatchDiscriminator
    adv = PatchAdversarialLoss()
    for tag, (cfg, shape) in NETS.items():
        for dtype in (torch.float32, torch.bfloat16):
            torch.manual_seed(0)
            ours = PatchDiscriminator(**cfg).to("cuda", dtype).train()
            plain = torch_restatement(cfg).to("cuda", dtype).train()
            x = torch.randn(shape, device="cuda", dtype=dtype)

            def step_ours():
                ours.zero_grad(set_to_none=True)
                adv(ours(x)[-1], True, True).backward()

            def step_plain():
                plain.zero_grad(set_to_none=True)
                y = plain(x).float()
                ((torch.where(y > 0, y, 0.05 * y) - 1.0) ** 2).mean().backward()

            for _ in range(3):
                step_ours()
                step_plain()
            a, b = _alternate([step_ours, step_plain], seconds, rounds)
            name = str(dtype).split(".")[-1]
            out(f"step {tag} {tuple(shape)} {name}: native {_fmt(a)}   torch.nn {_fmt(b)}   ratio of medians {a[0] / b[0]:.2f}")
            ops.start_profile()
            step_ours()
            rec = ops.stop_profile()
            total, by = sum(r[2] for r in rec), {}
            for label, _, ms in rec:
                by[label] = by.get(label, 0.0) + ms
            out(f"  kernels of one step (labelled launches: {total:.3f} ms): " + ", ".join(f"{k} {v:.3f} ms ({100 * v / total:.0f}%)"
                                                                                           for k, v in sorted(by.items(), key=lambda kv: -kv[1])[:8]))


def norm_passes(out, seconds, rounds):
    from generativemodels_amd import ops
    from generativemodels_amd._native import check, lib
    L, s = lib(), ops._stream
    # the normalised tensors of the two discriminators: (N, spatial, C)
    tensors = [(2, (16, 16, 16), 64), (2, (8, 8, 8), 128), (2, (7, 7, 7), 256), (16, (16, 16), 128), (16, (8, 8), 256), (16, (7, 7), 512), (2, (64, 64, 64), 64)]
    for n, sp, c in tensors:
        for dtype in (torch.float32, torch.bfloat16):
            code = ops.dt_code(dtype)
            x = torch.randn((n, *sp, c), device="cuda").to(dtype)
            gy = torch.randn((n, *sp, c), device="cuda").to(dtype)
            y, dx = torch.empty_like(x), torch.empty_like(x)
            rows, v = ops.rows_of(x), ops.rows_of(x) // n
            tab = torch.randn((6, c), device="cuda")
            tabn = torch.randn((6, n, c), device="cuda")
            part = torch.empty((max(int(L.gm_bn_bwd_stats_slots(rows)), 1), c, 2), dtype=torch.float64, device="cuda")
            partn = torch.empty((max(int(L.gm_gn_bwd_stats_slots(n, v)), 1), n, c, 2), dtype=torch.float64, device="cuda")
            p = lambda t: t.data_ptr()  # noqa: E731

            def bn_apply():
                check(L.gm_bn_apply(p(x), c, p(y), c, p(tab[0]), p(tab[1]), rows, c, 1, 0.2, code, s()), "gm_bn_apply")

            def gn_apply():
                check(L.gm_gn_apply(p(x), c, p(y), c, p(tabn[0]), p(tabn[1]), c, n, v, c, 2, code, s()), "gm_gn_apply")

            def bn_bwd():
                check(L.gm_bn_bwd_stats(p(x), c, p(gy), c, p(tab[0]), p(tab[1]), p(tab[2]), p(tab[3]), rows, c, 1, 0.2, p(part), code, s()), "gm_bn_bwd_stats")
                check(L.gm_bn_bwd_apply(p(x), c, p(gy), c, p(dx), c, p(tab[0]), p(tab[1]), p(tab[2]), p(tab[4]), p(tab[5]), rows, c, 1, 0.2, code, s()), "gm_bn_bwd_apply")

            def gn_bwd():
                check(L.gm_gn_bwd_stats(p(x), c, p(gy), c, p(tabn[0]), p(tabn[1]), c, n, v, c, 2, p(partn), code, s()), "gm_gn_bwd_stats")
                check(L.gm_gn_bwd_apply(p(x), c, p(gy), c, p(dx), c, p(tabn[0]), p(tabn[1]), c, p(tabn[2]), p(tabn[3]), p(tabn[4]), n, v, c, 2, code, s()),
                      "gm_gn_bwd_apply")

            fa, ga, fb, gb = _alternate([bn_apply, gn_apply, bn_bwd, gn_bwd], seconds / 4, rounds)
            nbytes = x.numel() * x.element_size()
            name = str(dtype).split(".")[-1]
            out(f"norm {n}x{'x'.join(map(str, sp))}x{c} {name} ({nbytes / 1e6:.1f} MB): apply bn {fa[0] * 1e6:8.1f} us [{fa[1] * 1e6:.1f}, {fa[2] * 1e6:.1f}] "
                f"({2 * nbytes / fa[0] / HBM_PEAK * 100:.0f}% of peak) vs gn {ga[0] * 1e6:8.1f} us [{ga[1] * 1e6:.1f}, {ga[2] * 1e6:.1f}]   "
                f"backward bn {fb[0] * 1e6:8.1f} us [{fb[1] * 1e6:.1f}, {fb[2] * 1e6:.1f}] ({5 * nbytes / fb[0] / HBM_PEAK * 100:.0f}% of peak) "
                f"vs gn {gb[0] * 1e6:8.1f} us [{gb[1] * 1e6:.1f}, {gb[2] * 1e6:.1f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_patchgan needs an MI355X: no GPU found")
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)
    out(f"device {torch.cuda.get_device_name(0)}; windows of {args.seconds} s, {args.rounds} alternating rounds; median [min, max]")
    norm_passes(out, args.seconds, args.rounds)
    if not args.skip_steps:
        steps(out, args.seconds, args.rounds)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
