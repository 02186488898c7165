"""Writes tests/golden/spectral_loss.pt: what the UNMODIFIED reference JukeboxLoss (loaded through oracle/ref_loader.py and its stub) returns on CPU fp32
tensors for the cases of tests/_spectral_cases.py, its gradient through autograd, the fp64 evaluation of the same formula, and per case and reduction
the distance of the reference in fp32 from fp64 (`e_ref`) and of the plan's fp32 NumPy emulator from fp64 (`e_emul`), for the loss and for the gradient (max
norm over both operands).  The GPU tests compare the kernels with fp64 and take max(e_ref, 8 * e_emul) as their bar.  A case is only written when the
reference's gradient is finite and e_ref(gradient) <= 2^-20 * max|gradient| (else the next seed is tried): the bar then rests on a well-conditioned
input, not on an amplitude near zero.  Data only; runs where the reference tree is present (CPU, seconds):

    python tools/make_golden_spectral.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _spectral_cases as S  # noqa: E402
import ref_loader  # noqa: E402


def reference_class():
    """JukeboxLoss from the reference's own file (its package __init__ also imports the perceptual loss, whose networks are not on this machine)."""
    assert ref_loader.load_reference() is not None, "no reference tree"
    path = os.path.join(ref_loader.reference_root(), "generative", "losses", "spectral_loss.py")
    spec = importlib.util.spec_from_file_location("_reference_spectral_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.JukeboxLoss


def _maxabs(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def evaluate(case, seed, Ref):
    plan = S.plan_of(case)
    x, y = S.make_inputs(case["shape"], seed)
    up = S.make_upstream(plan.full_shape, seed)
    out = dict(name=case["name"], shape=case["shape"], fft_signal_size=case["fft_signal_size"], fft_norm=case["fft_norm"], recipe=dict(shape=case["shape"], seed=seed),
               loss_ref={}, loss_fp64={}, e_ref_loss={}, e_emul_loss={}, e_ref_grad={}, e_emul_grad={}, grad_max={})
    amp = torch.minimum(S.amplitude(x.double(), case).min(), S.amplitude(y.double(), case).min())
    out["min_amplitude"] = float(amp)
    ok = True
    for red in S.REDUCTIONS:
        loss = Ref(spatial_dims=len(case["shape"]) - 2, fft_signal_size=case["fft_signal_size"], fft_norm=case["fft_norm"], reduction=red)
        xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        v = loss(xr, yr)
        gx, gy = torch.autograd.grad(v, [xr, yr], up if red == "none" else None)
        v64, gx64, gy64 = S.exact(x, y, case, red, up if red == "none" else None)
        ev, egx, egy = plan.emulate_loss(x.numpy(), y.numpy(), red, np.float32, upstream=up.numpy() if red == "none" else None)
        if red == "none":
            out["e_emul_loss"][red] = _maxabs(ev, v64.narrow(-1, 0, plan.half))
        else:
            out["loss_ref"][red], out["loss_fp64"][red] = float(v.detach()), float(v64)
            out["e_emul_loss"][red] = abs(float(ev) - float(v64))
        out["e_ref_loss"][red] = _maxabs(v.detach(), v64)
        out["e_ref_grad"][red] = max(_maxabs(gx, gx64), _maxabs(gy, gy64))
        out["e_emul_grad"][red] = max(_maxabs(egx, gx64), _maxabs(egy, gy64))
        out["grad_max"][red] = float(torch.maximum(gx64.abs().max(), gy64.abs().max()))
        finite = bool(torch.isfinite(gx).all() and torch.isfinite(gy).all())
        ok = ok and finite and out["e_ref_grad"][red] <= 2.0 ** -20 * out["grad_max"][red]
        if red == "mean":
            out["grad_ref"], out["grad_fp64"] = gx.detach().clone(), gx64.clone()
    return out, ok


def main():
    Ref = reference_class()
    cases = []
    for i, case in enumerate(S.CASES):
        for attempt in range(20):
            seed = 1000 + 37 * i + 1009 * attempt
            got, ok = evaluate(case, seed, Ref)
            if ok:
                break
        else:
            raise SystemExit(f"{case['name']}: no seed in 20 met the fixture's condition")
        ratio = max(got["e_ref_grad"][red] / got["grad_max"][red] for red in S.REDUCTIONS)
        print(f"{got['name']:28s} seed {seed}  min amplitude {got['min_amplitude']:.3e}  e_ref(grad) / max|grad| {ratio:.2e}  "
              f"loss e_ref {got['e_ref_loss']['mean']:.2e} e_emul {got['e_emul_loss']['mean']:.2e}  grad e_ref {got['e_ref_grad']['mean']:.2e} "
              f"e_emul {got['e_emul_grad']['mean']:.2e}")
        cases.append(got)
    path = os.path.join(ROOT, "tests", "golden", "spectral_loss.pt")
    torch.save(dict(cases=cases, torch_version=str(torch.__version__)), path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
