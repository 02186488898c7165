"""Measures PerceptualLoss on the MI355X (needs the GPU: fails without one).

    python tools/bench_perceptual.py [--seconds 0.5] [--rounds 5] [--out FILE]

fp32 and bf16, default-initialised weights (the arithmetic does not depend on their values):
  * forward + backward (the gradient with respect to the reconstruction) of "alex" and "vgg" at 16 x 1 x 64 x 64;
  * the 2.5-D loss of "alex" at 1 x 1 x 64^3 with fake_3d_ratio 0.25 (16 slices per axis, three axes).
Host clock around steps that end in a device synchronise, windows of at least --seconds after a warm-up, --rounds windows; median and [min, max] over the
rounds.  Then the share of every kernel label in one step (ops.start_profile: device events around each launch).  The numbers are records: the reference
needs the lpips package and torchvision, so there is no same-machine comparison."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("alex 2-D", dict(spatial_dims=2, network_type="alex"), (16, 1, 64, 64)),
         ("vgg 2-D", dict(spatial_dims=2, network_type="vgg"), (16, 1, 64, 64)),
         ("alex 2.5-D ratio 0.25", dict(spatial_dims=3, network_type="alex", is_fake_3d=True, fake_3d_ratio=0.25), (1, 1, 64, 64, 64))]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_perceptual needs an MI355X: no GPU found")
    from generativemodels_amd import ops
    from generativemodels_amd.losses import PerceptualLoss

    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)
    out(f"device {torch.cuda.get_device_name(0)}; windows of {args.seconds} s, {args.rounds} rounds; median [min, max]")
    for tag, cfg, shape in CASES:
        for dtype in (torch.float32, torch.bfloat16):
            torch.manual_seed(0)
            loss = PerceptualLoss(pretrained=False, **cfg).to("cuda", dtype)
            images = (torch.rand(shape, device="cuda") * 2 - 1).to(dtype)
            recon = (images + 0.1 * torch.randn(shape, device="cuda").to(dtype)).requires_grad_(True)

            def step():
                recon.grad = None
                loss(recon, images).backward()

            for _ in range(3):
                step()
            got = [_window(step, args.seconds) for _ in range(args.rounds)]
            name = str(dtype).split(".")[-1]
            out(f"step {tag} {tuple(shape)} {name}: forward + backward {statistics.median(got) * 1e3:8.3f} ms [{min(got) * 1e3:.3f}, {max(got) * 1e3:.3f}]")
            ops.start_profile()
            step()
            rec = ops.stop_profile()
            total, by = sum(r[2] for r in rec), {}
            for label, _, ms in rec:
                by[label] = by.get(label, 0.0) + ms
            out(f"  kernels of one step ({len(rec)} labelled launches: {total:.3f} ms): "
                + ", ".join(f"{k} {v:.3f} ms ({100 * v / total:.0f}%)" for k, v in sorted(by.items(), key=lambda kv: -kv[1])[:8]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
