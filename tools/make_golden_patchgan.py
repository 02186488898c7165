"""TEST INFRASTRUCTURE ONLY (CPU, needs the reference tree).  Writes tests/golden/patchgan.pt: the UNMODIFIED reference's PatchDiscriminator,
MultiScalePatchDiscriminator and PatchAdversarialLoss on the cases of tests/_patchgan_cases.py.

    python tools/make_golden_patchgan.py

Per case: the state_dict shapes and the recipe of weights and inputs (tests/_patchgan_cases.py: never the tensors), every returned tensor in train() and
in eval() mode from an fp32 run, the running buffers after the train() call, every parameter gradient and the input gradient from an fp64 run of
loss = adv(out, True, False) + 0.1 * sum(mean(feature^2)), the input's seed (chosen so that no logit of a least-squares case sits at the kink of the
loss's LeakyReLU(0.05): tests/_patchgan_cases.py), and the reference's own bf16 errors against fp64 (per returned tensor the max and mean error
over the stored sample; for the gradients the aggregate relative L2).  `dstep`: on a2d's network, 0.5 * (adv(D(fake)[-1], False, True) +
adv(D(real)[-1], True, True)) for the three criteria -- losses, the two logit maps, gradients and the buffers after both calls.

Large tensors are stored sampled (tests/_patchgan_cases.py says why and how).  The script refuses to write a fixture in which any fp32 tensor is further
than 2e-4 * max(1, |ref|max) from its fp64 twin: that is a condition on the inputs (pre-activations away from the LeakyReLU kink, enough values per
channel), met here with a margin of two orders.  oracle/ stays as it is; this script borrows its loader and stub."""
import copy
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _patchgan_cases as P  # noqa: E402
import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "patchgan.pt")
GUARD = 2e-4


def reference_loss_module():
    """adversarial_loss.py from the reference's own file (its package __init__ also imports the perceptual loss, whose networks are not here)."""
    path = os.path.join(ref_loader.reference_root(), "generative", "losses", "adversarial_loss.py")
    spec = importlib.util.spec_from_file_location("_reference_adversarial_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _model(nets, case, sd, dtype, train):
    cls = nets.PatchDiscriminator if case["kind"] == "patch" else nets.MultiScalePatchDiscriminator
    m = cls(**copy.deepcopy(case["cfg"]))
    m.load_state_dict(sd)
    m = m.to(dtype)
    return m.train() if train else m.eval()


def choose_input(nets, case, name, sd):
    """-> (seed, input): the first candidate whose logits keep KINK_MARGIN mean bf16 errors away from the kink of the least-squares activation (any seed for
    a smooth criterion).  An fp32 forward sieves the candidates with the previous estimate of the error; the accepted one is checked with its own."""
    m32, m64, mb = (_model(nets, case, sd, dt, True) for dt in (torch.float32, torch.float64, torch.bfloat16))
    estimate = None
    with torch.no_grad():
        for seed in P.candidate_input_seeds(name):
            x = P.case_input(name, seed)
            if case["loss"][1] != "least_squares":
                return seed, x
            if estimate is not None:
                t32, oi, _ = P.flatten_outputs(case["kind"], m32(x))
                if min(float(t32[i].abs().min()) / estimate[j] for j, i in enumerate(oi)) < 0.9 * P.KINK_MARGIN:
                    continue
            t64, oi, _ = P.flatten_outputs(case["kind"], m64(x.double()))
            tb, _, _ = P.flatten_outputs(case["kind"], mb(x.bfloat16()))
            estimate = [float((tb[i].double() - t64[i]).abs().mean()) for i in oi]
            if all(float(t64[i].abs().min()) >= P.KINK_MARGIN * e for i, e in zip(oi, estimate)):
                return seed, x
    raise SystemExit(f"{name}: no candidate input keeps the logits away from the kink")


def _buffers(m):
    return {k: v.detach().clone() for k, v in m.named_buffers()}


def _guard(what, a32, a64, worst):
    rel = (a32.double() - a64.double()).abs().max().item() / max(1.0, a64.abs().max().item())
    if rel > GUARD:
        raise SystemExit(f"{what}: the fp32 reference is {rel:.3e} (relative to max(1, |ref|max)) from fp64: above {GUARD:g}, not a sound fixture")
    return max(worst, rel)


def _grad_run(nets, Loss, case, sd, x, dtype):
    m = _model(nets, case, sd, dtype, True)
    xr = x.to(dtype).clone().requires_grad_(True)
    reduction, criterion = case["loss"]
    loss = P.training_loss(case["kind"], m(xr), Loss(reduction=reduction, criterion=criterion))
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    grads["input"] = xr.grad.detach().clone()
    return loss.detach(), grads


def _dstep_run(nets, Loss, case, sd, fake, real, criterion, dtype):
    m = _model(nets, case, sd, dtype, True)
    adv = Loss(criterion=criterion)
    lf, lr = m(fake.to(dtype))[-1], m(real.to(dtype))[-1]
    loss = 0.5 * (adv(lf, False, True) + adv(lr, True, True))
    loss.backward()
    return loss.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}, _buffers(m), lf.detach(), lr.detach()


def main():
    gen = ref_loader.load_reference()
    if gen is None:
        raise SystemExit("the reference tree is not present")
    nets = gen.networks.nets
    Loss = reference_loss_module().PatchAdversarialLoss
    torch.manual_seed(0)
    cases, sds = {}, {}
    for name, case in P.CASES.items():
        cls = nets.PatchDiscriminator if case["kind"] == "patch" else nets.MultiScalePatchDiscriminator
        shapes = {k: tuple(v.shape) for k, v in cls(**copy.deepcopy(case["cfg"])).state_dict().items()}
        sd = sds[name] = P.make_state_dict(shapes, case["seed"])
        input_seed, x = choose_input(nets, case, name, sd)
        worst_out = worst_grad = worst_buf = 0.0
        rec = dict(cfg=case["cfg"], kind=case["kind"], shapes=shapes, synthetic_seed=case["seed"], weights_rounded_to="bfloat16",
                   input_shape=tuple(x.shape), input_seed=input_seed, input_sum=float(x.double().sum()), loss=case["loss"])
        with torch.no_grad():
            for mode in ("train", "eval"):
                m32, m64 = (_model(nets, case, sd, dt, mode == "train") for dt in (torch.float32, torch.float64))
                t32, oi, fi = P.flatten_outputs(case["kind"], m32(x))
                t64, _, _ = P.flatten_outputs(case["kind"], m64(x.double()))
                for i, (a, b) in enumerate(zip(t32, t64)):
                    worst_out = _guard(f"{name} {mode} output {i}", a, b, worst_out)
                rec[mode] = [P.record(t) for t in t32]
                if mode == "train":
                    rec["output_index"], rec["feature_index"] = oi, fi
                    b32, b64 = _buffers(m32), _buffers(m64)
                    for k in b32:
                        worst_buf = _guard(f"{name} buffer {k}", b32[k], b64[k], worst_buf)
                    rec["buffers_after"] = b32
                    mb = _model(nets, case, sd, torch.bfloat16, True)
                    tb, _, _ = P.flatten_outputs(case["kind"], mb(x.bfloat16()))
                    errs = [(P.sample(a).double() - P.sample(b)).abs() for a, b in zip(tb, t64)]
                    rec["bf16_forward"] = [dict(max_err=e.max().item(), mean_err=e.mean().item()) for e in errs]
        loss64, g64 = _grad_run(nets, Loss, case, sd, x, torch.float64)
        loss32, g32 = _grad_run(nets, Loss, case, sd, x, torch.float32)
        _, gb = _grad_run(nets, Loss, case, sd, x, torch.bfloat16)
        for k in g64:
            worst_grad = _guard(f"{name} gradient {k}", g32[k], g64[k], worst_grad)
        keys = sorted(g64)
        rec["loss"] = case["loss"]
        rec["loss_value"] = float(loss64)
        rec["grads"] = {k: P.record(g64[k]) for k in keys}
        rec["bf16_grad_rel_l2"] = P.rel_l2([P.sample(gb[k]) for k in keys], [P.sample(g64[k]) for k in keys])
        rec["fp32_err"] = dict(outputs=worst_out, grads=worst_grad, buffers=worst_buf)
        cases[name] = rec
        print(name, "input seed", input_seed, sum(torch.Size(s).numel() for s in shapes.values()), "state entries;", [r["shape"] for r in rec["train"]], "fp32 err", rec["fp32_err"],
              "bf16 forward", [f"{e['max_err']:.2e}/{e['mean_err']:.2e}" for e in rec["bf16_forward"]], "bf16 grad rel L2", f"{rec['bf16_grad_rel_l2']:.2e}")

    case, sd = P.CASES[P.DSTEP_CASE], sds[P.DSTEP_CASE]
    fake, real = P.dstep_fake(), P.case_input(P.DSTEP_CASE, cases[P.DSTEP_CASE]["input_seed"])
    dstep = dict(case=P.DSTEP_CASE, fake_sum=float(fake.double().sum()), criteria={})
    for criterion in P.DSTEP_CRITERIA:
        l64, g64, b64, lf, lr = _dstep_run(nets, Loss, case, sd, fake.double(), real.double(), criterion, torch.float64)
        l32, g32, b32, _, _ = _dstep_run(nets, Loss, case, sd, fake, real, criterion, torch.float32)
        _, gb, _, _, _ = _dstep_run(nets, Loss, case, sd, fake, real, criterion, torch.bfloat16)
        worst = _guard(f"dstep {criterion} loss", l32, l64, 0.0)
        for k in g64:
            worst = _guard(f"dstep {criterion} gradient {k}", g32[k], g64[k], worst)
        for k in b64:
            worst = _guard(f"dstep {criterion} buffer {k}", b32[k], b64[k], worst)
        keys = sorted(g64)
        dstep["criteria"][criterion] = dict(loss=float(l64), grads={k: P.record(g64[k]) for k in keys}, buffers_after={k: v.float() if v.is_floating_point() else v for k, v in b64.items()},
                                            logits_fake=lf, logits_real=lr, fp32_err=worst,
                                            bf16_grad_rel_l2=P.rel_l2([P.sample(gb[k]) for k in keys], [P.sample(g64[k]) for k in keys]))
        print("dstep", criterion, "loss", float(l64), "fp32 err", f"{worst:.2e}", "bf16 grad rel L2", f"{dstep['criteria'][criterion]['bf16_grad_rel_l2']:.2e}",
              "num_batches_tracked", {int(v) for k, v in b64.items() if k.endswith("num_batches_tracked")})
    torch.save(dict(kind="patchgan", sample_max=P.SAMPLE_MAX, cases=cases, dstep=dstep), OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
