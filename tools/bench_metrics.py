"""Times the metric kernels against the op sequence the reference runs for the same numbers, on the same GPU.

    python tools/bench_metrics.py                 # every configuration and implementation, one child process each
    python tools/bench_metrics.py --config ssim3d_128 --impl native
    python tools/bench_metrics.py --backward      # forward + backward: the native kernels against torch autograd through the dense sequence

Each (configuration, implementation) step is its own process under `timeout -k 10`; the steps are chained -- the first one that fails ends the
run.  A step warms its shapes up, then times `reps` repetitions with device events and prints ONE JSON line: median / min / max milliseconds
per call, the bytes one pass over the inputs moves, and that figure over the median as a share of the HBM peak.

The "torch" implementation is the reference's op sequence restated here (dense grouped convolution with the full outer-product window, eight
image-size temporaries, avg_pool between scales); it exists for this comparison only and is not part of the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s (spec)
CONFIGS = {
    "ssim3d_128": dict(kind="ssim", shape=(1, 1, 128, 128, 128), kernel_size=11),
    "ms_ssim3d_128": dict(kind="ms_ssim", shape=(1, 1, 128, 128, 128), kernel_size=4),
    "ssim2d_256": dict(kind="ssim", shape=(16, 1, 256, 256), kernel_size=11),
}
STEP_TIMEOUT = {"native": 120, "torch": 150}
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def torch_ssim_cs(x, y, window, c1, c2):
    import torch.nn.functional as F

    conv = F.conv3d if x.dim() == 5 else F.conv2d
    ch = x.shape[1]
    mu_x, mu_y = conv(x, window, groups=ch), conv(y, window, groups=ch)
    mu_xx, mu_yy, mu_xy = conv(x * x, window, groups=ch), conv(y * y, window, groups=ch), conv(x * y, window, groups=ch)
    sigma_x, sigma_y, sigma_xy = mu_xx - mu_x * mu_x, mu_yy - mu_y * mu_y, mu_xy - mu_x * mu_y
    cs = (2 * sigma_xy + c2) / (sigma_x + sigma_y + c2)
    return ((2 * mu_x * mu_y + c1) / (mu_x ** 2 + mu_y ** 2 + c1)) * cs, cs


def torch_call(cfg, x, y):
    """-> a closure running the dense op sequence once."""
    import torch
    import torch.nn.functional as F

    from generativemodels_amd.metrics.ssim import gaussian_taps

    nsp = x.dim() - 2
    g = gaussian_taps(cfg["kernel_size"], 1.5).to(x.device)
    window = g
    for _ in range(nsp - 1):
        window = window.unsqueeze(-1) * g
    window = window.expand(x.shape[1], 1, *window.shape).contiguous()
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    if cfg["kind"] == "ssim":
        return lambda: torch_ssim_cs(x, y, window, c1, c2)[0].flatten(1).mean(1, keepdim=True)
    pool = F.avg_pool3d if nsp == 3 else F.avg_pool2d
    w = torch.tensor(WEIGHTS, device=x.device)

    def ms():
        a, b, parts = x, y, []
        for i in range(len(WEIGHTS)):
            ssim, cs = torch_ssim_cs(a, b, window, c1, c2)
            parts.append(torch.relu((ssim if i == len(WEIGHTS) - 1 else cs).flatten(1).mean(1)))
            a, b = pool(a, kernel_size=2), pool(b, kernel_size=2)
        return torch.prod(torch.stack(parts) ** w.view(-1, 1), dim=0).view(-1, 1)
    return ms


def native_call(cfg, x, y):
    from generativemodels_amd.metrics import MultiScaleSSIMMetric, SSIMMetric

    nsp = x.dim() - 2
    metric = SSIMMetric(nsp, kernel_size=cfg["kernel_size"]) if cfg["kind"] == "ssim" else MultiScaleSSIMMetric(nsp, kernel_size=cfg["kernel_size"], weights=WEIGHTS)
    return lambda: metric._compute_metric(x, y)


def run_step(name, impl, reps, warmup, backward=False):
    import torch

    assert torch.cuda.is_available(), "bench_metrics needs an MI355X"
    cfg = CONFIGS[name]
    g = torch.Generator().manual_seed(3)
    y = torch.rand(cfg["shape"], generator=g).to("cuda:0")
    x = (y + 0.1 * torch.rand(cfg["shape"], generator=g).to("cuda:0")).clamp(0, 1)
    call = (native_call if impl == "native" else torch_call)(cfg, x, y)
    if backward:  # one training-style step: the value, then d(sum of the values) / d(both images)
        x.requires_grad_(True), y.requires_grad_(True)
        forward = call

        def call():
            x.grad = y.grad = None
            value = forward()
            value.sum().backward()
            return value.detach()
    for _ in range(warmup):
        value = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        value = call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    med = statistics.median(times)
    one_pass = 2 * x.numel() * x.element_size()  # both images once; MS-SSIM's pooled scales add 1/7 (3-D) of that again, not counted
    rec = dict(config=name, impl=impl, backward=backward, shape=list(cfg["shape"]), kernel_size=cfg["kernel_size"], reps=reps, ms_median=med, ms_min=min(times), ms_max=max(times),
               value=[float(v) for v in value.flatten().tolist()], one_pass_bytes=one_pass, one_pass_gb_per_s=one_pass / (med * 1e-3) / 1e9,
               share_of_hbm_peak=one_pass / (med * 1e-3) / HBM_PEAK, peak_mem_mb=torch.cuda.max_memory_allocated() / 2 ** 20)
    if backward:
        rec.update(grad_abs_max=[float(x.grad.abs().max()), float(y.grad.abs().max())])
    if impl == "native":  # per-launch split of one more call (device events around each launch)
        from generativemodels_amd import ops

        ops.start_profile()
        call()
        rec["launches"] = [dict(name=n, shape=m["shape"], ms=t, gb_per_s=m["bytes"] / (t * 1e-3) / 1e9, gflop_per_s=m["flops"] / (t * 1e-3) / 1e9)
                           for n, m, t in ops.stop_profile()]
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=list(CONFIGS))
    ap.add_argument("--impl", choices=["native", "torch"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--backward", action="store_true", help="time forward + backward with both images requiring a gradient")
    a = ap.parse_args()
    if a.config and a.impl:
        run_step(a.config, a.impl, a.reps, a.warmup, a.backward)
        return 0
    # the native steps first, then the dense sequence from the cheapest configuration to the dearest: a dense step that fails ends the run late
    names = [a.config] if a.config else list(CONFIGS)
    steps = [(n, i) for i in ([a.impl] if a.impl else ["native", "torch"]) for n in (names if i == "native" else names[::-1])]
    for name, impl in steps:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[impl]), sys.executable, os.path.abspath(__file__), "--config", name, "--impl", impl,
               "--reps", str(a.reps if impl == "native" else max(5, a.reps // 3)), "--warmup", str(a.warmup if impl == "native" else 2)] + (["--backward"] if a.backward else [])
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:  # chained: nothing more is started on the device after a step that failed
            print(json.dumps(dict(config=name, impl=impl, failed=True, returncode=rc)), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
