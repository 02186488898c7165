"""Times JukeboxLoss forward + backward (reduction "mean", both operands wanting a gradient) on the native Fourier kernels, fp32 and bf16, against torch's own
composite on the same GPU (torch.fft.fftn + the formula + autograd, fp32), and writes one JSON line per shape and dtype to profiles/spectral_bench.jsonl.

Method: every shape is warmed up on both sides; then ROUNDS rounds alternate the two sides, each round timing `iters` forward + backward steps between two
device events (iters sized so that a window lasts about 0.5 s); the median over rounds and the min / max spread are reported.  `bytes` are the HBM bytes
the native passes must move (spectral_plan.bytes_moved for the four transforms, plus the amplitude pass), `floor_ms` that count over the 6.29 TB/s a copy
sustains on this part and over its 8.0 TB/s specification.

    python tools/bench_spectral.py [--out profiles/spectral_bench.jsonl] [--rounds 7]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from generativemodels_amd.losses import JukeboxLoss  # noqa: E402
from generativemodels_amd.spectral_plan import plan_for  # noqa: E402

SHAPES = [(16, 1, 256, 256), (8, 3, 224, 224), (2, 1, 128, 128, 128), (1, 1, 160, 160, 96)]
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
WINDOW_MS = 500.0  # one timed window: long enough that the clock and the scheduler do not show


def composite(x, y):
    def amp(t):
        f = torch.fft.fftn(t, dim=tuple(range(1, t.dim())), norm="ortho")
        return torch.sqrt(torch.real(f) ** 2 + torch.imag(f) ** 2)
    return ((amp(x) - amp(y)) ** 2).mean()


def step(fn, x, y):
    x.grad = y.grad = None
    fn(x, y).backward()


def window(fn, x, y, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step(fn, x, y)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def native_bytes(shape, element_size):
    plan = plan_for(shape)
    bins = math.prod(plan.spectrum_shape)
    transforms = 2 * plan.bytes_moved(element_size) + 2 * plan.bytes_moved(element_size, adjoint=True)
    return transforms + 8 * bins * 4  # the amplitude pass reads both spectra and writes both gradient spectra over them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spectral.py needs an MI355X"
    dev = "cuda"
    rows = []
    for shape in SHAPES:
        g = torch.Generator().manual_seed(1)
        x32, y32 = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
        loss = JukeboxLoss(len(shape) - 2)
        ref = None
        for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            xn, yn = x32.to(dtype, copy=True).requires_grad_(True), y32.to(dtype, copy=True).requires_grad_(True)
            xt, yt = x32.clone().requires_grad_(True), y32.clone().requires_grad_(True)
            for _ in range(3):
                step(loss, xn, yn)
                step(composite, xt, yt)
            torch.cuda.synchronize()
            if dtype == torch.float32:  # the two sides compute the same thing
                vn, vt = float(loss(xn, yn).detach()), float(composite(xt, yt).detach())
                gerr = float((xn.grad - xt.grad).abs().max() / xt.grad.abs().max())
                ref = dict(loss_native=vn, loss_torch=vt, grad_rel_diff=gerr)
            it_n = max(1, int(WINDOW_MS / max(window(loss, xn, yn, 2), 1e-3)))
            it_t = max(1, int(WINDOW_MS / max(window(composite, xt, yt, 2), 1e-3)))
            tn, tt = [], []
            for _ in range(args.rounds):
                tn.append(window(loss, xn, yn, it_n))
                tt.append(window(composite, xt, yt, it_t))
            nbytes = native_bytes(shape, xn.element_size())
            row = dict(shape=list(shape), dtype=name, native_ms=statistics.median(tn), native_ms_min=min(tn), native_ms_max=max(tn),
                       torch_fp32_ms=statistics.median(tt), torch_fp32_ms_min=min(tt), torch_fp32_ms_max=max(tt),
                       speedup=statistics.median(tt) / statistics.median(tn), iters=[it_n, it_t], rounds=args.rounds, bytes=nbytes,
                       floor_ms_measured_bw=1e3 * nbytes / HBM_MEASURED, floor_ms_spec_bw=1e3 * nbytes / HBM_SPEC, check=ref,
                       device=torch.cuda.get_device_name(0), torch=torch.__version__)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
