"""TEST INFRASTRUCTURE ONLY (CPU, needs the reference tree).  Writes tests/golden/encoder.pt: the UNMODIFIED reference's DiffusionModelEncoder on the
cases of tests/_encoder_cases.py, and the classifier-guided DDIM chain of the reference's anomaly-detection tutorial.

    python tools/make_golden_encoder.py

Per case: the state_dict shapes (the weights are a recipe: tests/_encoder_cases.py), the fp64 sum of the input, and
  * from an fp64 run in eval(): the final feature map, the logits, and the guidance gradient d sum_n log_softmax(logits)[n, y_n] / dx for stored labels;
  * from an fp64 run in train() with out[2].p = 0: every parameter gradient and the input gradient of F.cross_entropy(logits, y);
  * the reference's own fp32 and bf16 errors against fp64: per tensor the max and mean error (over the stored sample), for the gradients the aggregate
    relative L2.
The chain: L reversed DDIM steps, then L DDIM steps guided at scale 6, on a two-level UNet and the a2d-sized classifier, in fp64 with and without guidance.

Large tensors are stored sampled (tests/_encoder_cases.py).  The script refuses to write unless (a) every fp32 result of the reference is within one
tenth of the tests' bar of its fp64 twin, (b) the guided and unguided chains differ by at least 100 chain bars and (c) every fp64 hidden pre-activation
of every case is at least KINK_MARGIN times the reference's own mean bf16 error of the pre-activations away from zero, so that no bf16 run flips a ReLU
(tests/_encoder_cases.py::make_state_dict says why) -- conditions on the inputs, not measurements of the code under test.  oracle/ stays as it is; this script borrows its loader and stub."""
import copy
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _encoder_cases as E  # noqa: E402
import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "encoder.pt")


def _model(cls, cfg, sd, dtype, train):
    m = cls(**copy.deepcopy(cfg))
    m.load_state_dict(sd)
    m = m.to(dtype)
    return m.train() if train else m.eval()


def _encode(m, x, t, context=None, class_labels=None):
    """The reference's forward up to the flatten (diffusion_model_unet.py:2088-2111), by its own sub-modules."""
    from generative.networks.nets.diffusion_model_unet import get_timestep_embedding

    emb = m.time_embed(get_timestep_embedding(t, m.block_out_channels[0]).to(x.dtype))
    if m.num_class_embeds is not None:
        emb = emb + m.class_embedding(class_labels).to(x.dtype)
    h = m.conv_in(x)
    for blk in m.down_blocks:
        h, _ = blk(hidden_states=h, temb=emb, context=context)
    return h


def _eval_run(cls, name, sd, dtype):
    case = E.CASES[name]
    m = _model(cls, case["cfg"], sd, dtype, False)
    kw = E.case_kwargs(name, dtype=dtype)
    x, t, y = E.case_input(name).to(dtype), E.case_timesteps(name), E.case_labels(name)
    with torch.no_grad():
        feat = _encode(m, x, t, **kw)
        hidden = m.out[0](feat.reshape(feat.shape[0], -1))
    x_in = x.clone().requires_grad_(True)
    logits = m(x_in, t, **kw)
    selected = F.log_softmax(logits, dim=-1)[range(len(logits)), y.view(-1)]
    a = torch.autograd.grad(selected.sum(), x_in)[0]
    return dict(features=feat.detach(), logits=logits.detach(), guidance=a.detach(), hidden=hidden.detach())


def _train_run(cls, name, sd, dtype):
    case = E.CASES[name]
    m = _model(cls, case["cfg"], sd, dtype, True)
    m.out[2].p = 0.0
    kw = E.case_kwargs(name, dtype=dtype)
    x = E.case_input(name).to(dtype).requires_grad_(True)
    loss = F.cross_entropy(m(x, E.case_timesteps(name), **kw), E.case_labels(name))
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}  # (AttentionBlock.proj_attn is never applied)
    grads["input"] = x.grad.detach().clone()
    return loss.detach(), grads


def _guard(what, a, b, bar, worst):
    """fp32 within one tenth of the tests' bar of fp64."""
    rel = (a.double() - b.double()).abs().max().item() / max(1.0, b.abs().max().item())
    if rel > 0.1 * bar:
        raise SystemExit(f"{what}: the fp32 reference is {rel:.3e} (relative to max(1, |ref|max)) from fp64: above a tenth of the bar {bar:g}")
    return max(worst, rel)


def _chain(nets, DDIM, dtype, guided):
    C = E.CHAIN
    ccfg = E.CASES[C["classifier"]]["cfg"]
    shapes_c = {k: tuple(v.shape) for k, v in nets.diffusion_model_unet.DiffusionModelEncoder(**copy.deepcopy(ccfg)).state_dict().items()}
    shapes_u = {k: tuple(v.shape) for k, v in nets.DiffusionModelUNet(**copy.deepcopy(C["unet"])).state_dict().items()}
    clf = _model(nets.diffusion_model_unet.DiffusionModelEncoder, ccfg, E.make_state_dict(shapes_c, C["classifier_seed"]), dtype, False)
    unet = _model(nets.DiffusionModelUNet, C["unet"], E.make_state_dict(shapes_u, C["unet_seed"]), dtype, False)
    sch = DDIM(num_train_timesteps=C["num_train_timesteps"])
    sch.set_timesteps(C["num_train_timesteps"] // C["stride"])
    out = E.guided_chain(unet, clf, sch, E.chain_input().to(dtype), torch.tensor(C["labels"]), gradient=None if guided else False)
    return out.detach(), shapes_u


def main():
    gen = ref_loader.load_reference()
    if gen is None:
        raise SystemExit("the reference tree is not present")
    nets = gen.networks.nets
    cls = nets.diffusion_model_unet.DiffusionModelEncoder
    torch.manual_seed(0)
    cases = {}
    for name, case in E.CASES.items():
        shapes = {k: tuple(v.shape) for k, v in cls(**copy.deepcopy(case["cfg"])).state_dict().items()}
        sd = E.make_state_dict(shapes, case["seed"])
        e64, e32, eb = (_eval_run(cls, name, sd, dt) for dt in (torch.float64, torch.float32, torch.bfloat16))
        (l64, g64), (l32, g32), (_, gb) = (_train_run(cls, name, sd, dt) for dt in (torch.float64, torch.float32, torch.bfloat16))
        worst_v = worst_g = 0.0
        for k in ("features", "logits"):
            worst_v = _guard(f"{name} {k}", e32[k], e64[k], E.FP32_BAR, worst_v)
        worst_g = _guard(f"{name} guidance", e32["guidance"], e64["guidance"], E.GRAD_BAR, worst_g)
        for k in g64:
            worst_g = _guard(f"{name} gradient {k}", g32[k], g64[k], E.GRAD_BAR, worst_g)
        z, zb = e64["hidden"], eb["hidden"].double()
        z_err = (zb - z).abs().mean().item()
        at_risk, flips = int((z.abs() < E.KINK_MARGIN * z_err).sum()), int(((zb > 0) != (z > 0)).sum())
        print(name, f"hidden pre-activations: std {z.std().item():.3f}, mean bf16 error {z_err:.2e}, min |z| {z.abs().min().item():.3f}, units on "
              f"{int((z > 0).sum())} of {z.numel()}, within {E.KINK_MARGIN:g} errors of zero {at_risk}, flipped by the reference's bf16 run {flips}")
        if at_risk or flips:
            raise SystemExit(f"{name}: {at_risk} hidden units within {E.KINK_MARGIN:g} bf16 errors of the ReLU's kink, {flips} flipped: not a sound fixture")
        keys = sorted(g64)
        x = E.case_input(name)
        rec = dict(cfg=case["cfg"], shapes=shapes, synthetic_seed=case["seed"], weights_rounded_to="bfloat16", input_shape=tuple(x.shape),
                   input_sum=float(x.double().sum()), labels=E.case_labels(name), timesteps=E.case_timesteps(name),
                   features=E.record(e64["features"]), logits=e64["logits"].float(), logits64=e64["logits"], guidance=E.record(e64["guidance"]),
                   loss_value=float(l64), grads={k: E.record(g64[k]) for k in keys},
                   fp32_err=dict(values=worst_v, grads=worst_g), hidden=dict(min_abs=z.abs().min().item(), mean_bf16_err=z_err, units_on=int((z > 0).sum())),
                   bf16_err=dict(features=E.err_stats(E.sample(eb["features"]), E.sample(e64["features"])),
                                 logits_rel_l2=E.rel_l2([eb["logits"]], [e64["logits"]]),
                                 guidance_rel_l2=E.rel_l2([E.sample(eb["guidance"])], [E.sample(e64["guidance"])]),
                                 grads_rel_l2=E.rel_l2([E.sample(gb[k]) for k in keys], [E.sample(g64[k]) for k in keys])))
        cases[name] = rec
        print(name, "features", rec["features"]["shape"], "loss", rec["loss_value"], "fp32 err", rec["fp32_err"], "bf16", rec["bf16_err"])

    DDIM = gen.networks.schedulers.DDIMScheduler
    g64, shapes_u = _chain(nets, DDIM, torch.float64, True)
    u64, _ = _chain(nets, DDIM, torch.float64, False)
    g32, _ = _chain(nets, DDIM, torch.float32, True)
    bar = E.FP32_BAR * E.CHAIN_FACTOR * max(1.0, g64.abs().max().item())
    dev32 = (g32.double() - g64).abs().max().item()
    effect = (g64 - u64).abs().max().item()
    print(f"chain: fp32 vs fp64 {dev32:.3e}, guided vs unguided {effect:.3e}, bar {bar:.3e}")
    if dev32 > 0.1 * bar:
        raise SystemExit(f"chain: the fp32 reference is {dev32:.3e} from fp64: above a tenth of the bar {bar:.3e}")
    if effect < 100 * bar:
        raise SystemExit(f"chain: guidance moves the result by {effect:.3e}: less than 100 bars of {bar:.3e}; the chain test would not depend on the gradient")
    x = E.chain_input()
    chain = dict(cfg=E.CHAIN, unet_shapes=shapes_u, input_sum=float(x.double().sum()), guided=g64.float(), unguided=u64.float(), fp32_err=dev32, effect=effect)
    torch.save(dict(kind="encoder", sample_max=E.SAMPLE_MAX, cases=cases, chain=chain), OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
