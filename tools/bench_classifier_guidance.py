"""GPU: one classifier-guided DDIM step at the sizes of the reference's anomaly-detection tutorial (1 x 1 x 64 x 64; UNet (64, 64, 64), attention on the
last level; classifier DiffusionModelEncoder (32, 64, 64), attention (F, T, T), 2 classes), split three ways -- the UNet forward, the classifier gradient
through the tutorial's autograd lines, and the same gradient through inferers.classifier_guidance_gradient -- with launches per step and per-kernel
shares from ops.start_profile, and the head alone (gm_head_hidden + gm_head_tail) against a composition of operations the library had before it:
ops.to_channels_first -> ops.linear(post_act="relu") -> ops.linear, both in this process, at N = 1 and N = 16.  Every time is the minimum of REPS timed
repetitions after a warm-up.  Prints one JSON line per measurement.  Not bench.py: nothing here is a pass bar.
usage: python tools/bench_classifier_guidance.py [dtype=float32|bfloat16] [reps=30]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch
import torch.nn.functional as F

from generativemodels_amd import ops
from generativemodels_amd.inferers import classifier_guidance_gradient
from generativemodels_amd.networks.nets import DiffusionModelEncoder, DiffusionModelUNet

dt = getattr(torch, sys.argv[1]) if len(sys.argv) > 1 else torch.float32
REPS = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 30
dev = "cuda"
torch.manual_seed(0)
unet = DiffusionModelUNet(spatial_dims=2, in_channels=1, out_channels=1, num_channels=(64, 64, 64), attention_levels=(False, False, True), num_res_blocks=1,
                          num_head_channels=64, with_conditioning=False).to(dev, dt).eval()
clf = DiffusionModelEncoder(spatial_dims=2, in_channels=1, out_channels=2, num_channels=(32, 64, 64), attention_levels=(False, True, True),
                            num_res_blocks=(1, 1, 1), num_head_channels=64, with_conditioning=False).to(dev, dt).eval()
for p in clf.parameters():  # a fresh encoder has zero conv2 / proj_out weights; the times do not depend on the values, the gradients' finiteness check does
    if float(p.detach().abs().max()) == 0.0:
        p.data.normal_(0.0, 0.02)
x = torch.rand(1, 1, 64, 64, device=dev).to(dt)
t = torch.Tensor((100,)).to(dev)
y = torch.tensor([0], device=dev)


def min_ms(fn, reps=REPS):
    for _ in range(3):  # warm-up: packs weights, first-use initialisation
        fn()
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def profile(fn):
    ops.start_profile()
    fn()
    rec = ops.stop_profile()
    by = {}
    for name, _, ms in rec:
        by[name] = by.get(name, 0.0) + ms
    return len(rec), {k: round(v, 4) for k, v in sorted(by.items(), key=lambda kv: -kv[1])}


def unet_forward():
    with torch.no_grad():
        return unet(x, timesteps=t)


def gradient_autograd():
    x_in = x.detach().requires_grad_(True)
    logits = clf(x_in, timesteps=t)
    log_probs = F.log_softmax(logits, dim=-1)
    return torch.autograd.grad(log_probs[range(len(logits)), y.view(-1)].sum(), x_in)[0]


def gradient_helper():
    return classifier_guidance_gradient(clf, x, t, y)


assert torch.equal(gradient_autograd(), gradient_helper()) and bool(torch.isfinite(gradient_helper()).all())
for label, fn in (("unet_forward", unet_forward), ("classifier_gradient_autograd", gradient_autograd), ("classifier_gradient_helper", gradient_helper)):
    ms = min_ms(fn)
    launches, kernels = profile(fn)
    print(json.dumps(dict(part=label, dtype=str(dt).split(".")[-1], min_ms=round(ms, 4), timed_launches=launches, timed_kernels_ms=kernels,
                          note="timed_launches counts the launches that carry an ops._timed record")), flush=True)

# ---- the head alone against what the library had before it --------------------------------------------------------------------------------------------
l0, l3 = clf.out[0], clf.out[3]
for n in (1, 16):
    h = torch.randn(n, 8, 8, 64, device=dev).to(dt)  # the arena of the last level

    def head():
        return ops.classifier_head(h, l0.weight, l0.bias, l3.weight, l3.bias).logits

    def composed():
        flat = ops.to_channels_first(h).reshape(n, 4096)
        return ops.linear(ops.linear(flat, l0.weight, l0.bias, post_act="relu"), l3.weight, l3.bias)

    with torch.no_grad():
        err = (head().double() - composed().double()).abs().max().item()
        a, b = min_ms(head), min_ms(composed)
        again = (min_ms(head), min_ms(composed))  # a second round: the run-to-run spread of the minima
        launches_head, k_head = profile(head)
        launches_comp, k_comp = profile(composed)
    weight_bytes = l0.weight.numel() * l0.weight.element_size()
    print(json.dumps(dict(part="head_alone", dtype=str(dt).split(".")[-1], N=n, head_min_ms=round(a, 4), composed_min_ms=round(b, 4),
                          second_round_min_ms=[round(v, 4) for v in again], max_abs_difference=err, head_kernels_ms=k_head, composed_kernels_ms=k_comp,
                          composed_timed_launches=launches_comp, head_timed_launches=launches_head, w1_bytes=weight_bytes,
                          w1_passes_head=-(-n // ops.classifier_head_chunk(dt)))), flush=True)
