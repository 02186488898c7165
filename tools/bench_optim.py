"""GPU: the optimizer step alone -- generativemodels_amd.optim.Adam (one native launch per dtype + the counter launch) against torch.optim.Adam as
tools/bench_train.py constructs it (torch's default implementation), torch's foreach=True and torch's fused=True, on
  * the parameter set of the C4 latent UNet of tools/bench_train.py (41.7 M parameters), fp32 and bf16, and
  * the parameter set of the BASELINE configs[0] 2-D UNet (tools/bench_c1b.py) in fp32, as a small, launch-bound case,
with random gradients on every parameter that receives one in training (proj_attn never does).  Two more rows time the native step with gradients that are
element-aligned views of one flat bucket (the one-element path of the kernel) and the native step replayed from a HIP graph.
Every optimizer owns a copy of the parameters and gradients; they are timed in ALTERNATING windows of the same process (a host clock around `steps` steps that
end in a device synchronise; `steps` sized per optimizer from a pilot so that a window is at least --window seconds), and the median and the range of the
windows' per-step times are reported -- with the launches per step (counted by torch's profiler in a run of its own, after the timing) and the achieved
bytes/s at the bytes the update has to move: fp32 28 B per element (reads p, g, m, v; writes p, m, v); bf16 here 22 B (bf16 p and g, fp32 moments), torch's
bf16 14 B (bf16 moments).  The MI355X sustains about 6.3 TB/s from HBM (the microarchitecture guide's achievable rate).
usage: python tools/bench_optim.py [--windows 5] [--window 0.25] [--out profiles/optim_bench.txt]"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

import generativemodels_amd as gm
from generativemodels_amd.networks.nets import DiffusionModelUNet

HBM = 6.3e12


def c4_unet():
    return DiffusionModelUNet(spatial_dims=3, in_channels=4, out_channels=4, num_channels=(64, 128, 256), attention_levels=(False, True, True),
                              num_res_blocks=2, num_head_channels=(0, 128, 256))


def c1b_unet():
    return DiffusionModelUNet(2, 1, 1, num_channels=(32, 64), attention_levels=(False, True), num_res_blocks=1, num_head_channels=64)


def shapes_of(model):
    """[(shape, receives a gradient)] in parameters() order."""
    return [(tuple(p.shape), "proj_attn" not in k) for k, p in model.named_parameters()]


def make_set(shapes, dtype, seed, bucket=False):
    """bucket: the gradients are views of ONE flat buffer at element offsets off the 16-byte grid, as a GradientReducer bucket leaves them."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=g, device="cuda", dtype=torch.float32).mul_(0.05).to(dtype)) for s, _ in shapes]
    flat, cur = torch.empty(sum(math.prod(s) + 1 for s, t in shapes if t) + 1 if bucket else 0, device="cuda", dtype=dtype), 1
    per16 = 16 // max(1, flat.element_size())
    for p, (s, trained) in zip(params, shapes):
        p.grad = torch.randn(s, generator=g, device="cuda", dtype=torch.float32).mul_(0.01).to(dtype) if trained else None
        if bucket and trained:
            view = flat[cur:cur + p.numel()].view(s).copy_(p.grad)
            cur += p.numel() + (1 if (cur + p.numel()) % per16 == 0 else 0)
            assert view.data_ptr() % 16 != 0
            p.grad = view
    return params


def candidates(shapes, dtype):
    out = []
    for name, make, bytes_bf16 in (("gm.optim.Adam", lambda p: gm.optim.Adam(p, lr=1e-5), 22),
                                   ("torch.optim.Adam (default)", lambda p: torch.optim.Adam(p, lr=1e-5), 14),
                                   ("torch.optim.Adam(foreach=True)", lambda p: torch.optim.Adam(p, lr=1e-5, foreach=True), 14),
                                   ("torch.optim.Adam(fused=True)", lambda p: torch.optim.Adam(p, lr=1e-5, fused=True), 14)):
        params = make_set(shapes, dtype, seed=5)  # (the same values for every optimizer)
        try:
            opt = make(params)
            opt.step()
            torch.cuda.synchronize()
        except Exception as e:  # (fused=True where it does not construct or run: written down, not hidden)
            out.append(dict(name=name, error=f"{type(e).__name__}: {str(e).splitlines()[0][:140]}"))
            continue
        out.append(dict(name=name, opt=opt, params=params, step=opt.step, bytes=28 if dtype == torch.float32 else bytes_bf16, times=[]))
    # gradients that are element-aligned views of a flat bucket: every chunk on the one-element path
    params = make_set(shapes, dtype, seed=5, bucket=True)
    opt = gm.optim.Adam(params, lr=1e-5)
    opt.step()
    out.append(dict(name="gm.optim.Adam (bucket-view grads)", opt=opt, params=params, step=opt.step, bytes=28 if dtype == torch.float32 else 22, times=[]))
    # the native step replayed from a HIP graph: what is left when the host loop over the parameters is gone too
    params = make_set(shapes, dtype, seed=5)
    opt = gm.optim.Adam(params, lr=1e-5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    out.append(dict(name="gm.optim.Adam (graph replay)", opt=opt, params=params, step=graph.replay, bytes=28 if dtype == torch.float32 else 22, times=[]))
    return out


def window(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def launches(step):
    try:
        from torch.profiler import ProfilerActivity, profile

        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return str(n) if n else "not measured"
    except Exception as e:
        return f"not measured ({type(e).__name__})"


def agreement(shapes, dtype):
    """Three steps of the native optimizer and of torch's default from the same values: the largest parameter difference, over the largest parameter."""
    a, b = make_set(shapes, dtype, seed=9), make_set(shapes, dtype, seed=9)
    oa, ob = gm.optim.Adam(a, lr=1e-3), torch.optim.Adam(b, lr=1e-3)
    for _ in range(3):
        oa.step()
        ob.step()
    return max((x.detach().float() - y.detach().float()).abs().max().item() for x, y in zip(a, b)), max(y.detach().float().abs().max().item() for y in b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="least seconds per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on an MI355X: no GPU here, nothing measured")
    lines = [f"optimizer step alone, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {args.windows} alternating windows of >= {args.window} s each; "
             "per-step times in ms: median [min .. max]"]
    verdict = []
    sets = (("C4 latent UNet", shapes_of(c4_unet()), torch.float32), ("C4 latent UNet", shapes_of(c4_unet()), torch.bfloat16),
            ("configs[0] 2-D UNet", shapes_of(c1b_unet()), torch.float32))
    for label, shapes, dtype in sets:
        elems = sum(math.prod(s) for s, t in shapes if t)
        diff, scale = agreement(shapes, dtype)
        cands = candidates(shapes, dtype)
        live = [c for c in cands if "error" not in c]
        for c in live:  # pilot: warm, then size the window
            window(c["step"], 5)
            c["steps"] = max(20, math.ceil(args.window / window(c["step"], 10)))
        for _ in range(args.windows):
            for c in live:
                c["times"].append(window(c["step"], c["steps"]))
        lines.append("")
        lines.append(f"== {label}, {str(dtype).replace('torch.', '')}: {sum(1 for _, t in shapes if t)} tensors with a gradient of {len(shapes)}, {elems / 1e6:.2f} M elements; "
                     f"3 steps native vs torch default: max |dp| {diff:.2e} at max |p| {scale:.2f}")
        for c in cands:
            if "error" in c:
                lines.append(f"  {c['name']:<34} does not run here: {c['error']}")
                continue
            med, lo, hi = statistics.median(c["times"]), min(c["times"]), max(c["times"])
            n = (f"{len(c['opt']._launches) + 1} (by construction)" if c["name"] == "gm.optim.Adam" else launches(c["step"]))
            lines.append(f"  {c['name']:<34} {med * 1e3:8.4f} [{lo * 1e3:8.4f} .. {hi * 1e3:8.4f}]  {c['steps']:5d} steps/window  launches/step {n:<22} "
                         f"{c['bytes']} B/elem -> {c['bytes'] * elems / med / 1e12:6.3f} TB/s = {100 * c['bytes'] * elems / med / HBM:5.1f} % of 6.3 TB/s")
        if dtype == torch.float32:
            nat, ref = cands[0], cands[1]
            ok = max(nat["times"]) < min(ref["times"])
            verdict.append(f"{label} fp32: native window range [{min(nat['times']) * 1e3:.4f} .. {max(nat['times']) * 1e3:.4f}] ms "
                           f"{'lies BELOW' if ok else 'does NOT lie below'} torch default's [{min(ref['times']) * 1e3:.4f} .. {max(ref['times']) * 1e3:.4f}] ms")
        del cands, live
        torch.cuda.empty_cache()
    lines += ["", "condition (both fp32 sets: the native step's window range below the range of torch's default):"] + ["  " + v for v in verdict]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
