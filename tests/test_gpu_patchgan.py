"""PatchDiscriminator, MultiScalePatchDiscriminator and PatchAdversarialLoss on the GPU against tests/golden/patchgan.pt (the unmodified reference on
the CPU: tools/make_golden_patchgan.py), the loss kernel alone against fp64, and a discriminator step replayed from a HIP graph against the eager step.

Bars.  fp32 forward, train and eval: test_gpu_models._fp32_close.  Running buffers: 1e-5 * max(1, |ref|max).  fp32 gradients, the input gradient included:
6e-4 * max(1, |g|max) per tensor.  bf16 modules and fp32 masters under autocast: per returned tensor the mean error at most 1.5 x and the max error at most
2.0 x the reference's own bf16 errors, gradients at most 1.5 x the reference's own aggregate relative L2 error, all as stored in the fixture.
Large tensors are compared on the sample the fixture stores (tests/_patchgan_cases.py), plus the sum of the whole tensor."""
import warnings

import pytest
import torch

import _patchgan_cases as P
import generativemodels_amd as gm
from _util import load_fixture
from generativemodels_amd.losses import PatchAdversarialLoss
from generativemodels_amd.networks.nets import MultiScalePatchDiscriminator, PatchDiscriminator
from test_gpu_models import _fp32_close

pytestmark = pytest.mark.gpu

NAMES = sorted(P.CASES)
GRAD_BAR, BUFFER_BAR = 6e-4, 1e-5


@pytest.fixture(scope="module")
def fx():
    return load_fixture("patchgan")


def _model(fx, name, dtype=torch.float32, train=True):
    case = P.CASES[name]
    m = (PatchDiscriminator if case["kind"] == "patch" else MultiScalePatchDiscriminator)(**case["cfg"])
    m.load_state_dict(P.make_state_dict(fx["cases"][name]["shapes"], case["seed"]))
    m = m.to(dtype).cuda()
    return m.train() if train else m.eval()


def _input(fx, name):
    x = P.case_input(name, fx["cases"][name]["input_seed"])
    assert float(x.double().sum()) == fx["cases"][name]["input_sum"], "the seeded generator drew other numbers than the fixture's: regenerate it"
    return x


def _scaled_close(got, rec, bar, what):
    """max|err| over the stored sample <= bar * max(1, |ref|max of the whole tensor); the whole tensor's sum within numel * that."""
    assert tuple(got.shape) == rec["shape"], (what, tuple(got.shape), rec["shape"])
    tol = bar * max(1.0, rec["absmax"])
    err = (P.sample(got).double().cpu() - rec["sample"].double()).abs().max().item()
    print(f"{what}: max|err| {err:.3e} (bar {tol:.3e})")
    assert err <= tol, f"{what}: max|err| {err:.3e} > {tol:.3e}"
    assert abs(got.double().sum().item() - rec["sum"]) <= tol * got.numel(), f"{what}: sum {got.double().sum().item()} vs {rec['sum']}"


def _buffers_close(m, want, what):
    got = dict(m.named_buffers())
    assert set(got) == set(want)
    for k, w in want.items():
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(w), (what, k, int(got[k]), int(w))
        else:
            err = (got[k].double().cpu() - w.double()).abs().max().item()
            tol = BUFFER_BAR * max(1.0, w.abs().max().item())
            assert err <= tol, f"{what} {k}: max|err| {err:.3e} > {tol:.3e}"


def _grads(m, x, case, dtype=None, autocast=False):
    m.zero_grad(set_to_none=True)
    xr = (x if dtype is None else x.to(dtype)).cuda().requires_grad_(True)
    reduction, criterion = case["loss"]
    adv = PatchAdversarialLoss(reduction=reduction, criterion=criterion)
    with gm.autocast(torch.bfloat16, enabled=autocast):
        loss = P.training_loss(case["kind"], m(xr), adv)
    loss.backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads["input"] = xr.grad
    return loss.detach(), grads


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name", NAMES)
def test_fp32_forward_and_running_buffers(fx, name, mode):
    rec = fx["cases"][name]
    m = _model(fx, name, train=mode == "train")
    with torch.no_grad():  # (train() under no_grad still updates the running buffers)
        tensors, oi, fi = P.flatten_outputs(rec["kind"], m(_input(fx, name).cuda()))
    assert (oi, fi) == (rec["output_index"], rec["feature_index"]) and len(tensors) == len(rec[mode])
    for i, (t, r) in enumerate(zip(tensors, rec[mode])):
        assert tuple(t.shape) == r["shape"] and t.dtype == torch.float32
        _fp32_close(P.sample(t), r["sample"], f"{name} {mode} tensor {i}")
        _scaled_close(t, r, 1e-4, f"{name} {mode} tensor {i}")
    if mode == "train":
        _buffers_close(m, rec["buffers_after"], name)
    else:  # eval leaves every buffer as it was loaded
        loaded = P.make_state_dict(rec["shapes"], P.CASES[name]["seed"])
        _buffers_close(m, {k: loaded[k] for k, _ in m.named_buffers()}, name)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_gradients(fx, name):
    rec = fx["cases"][name]
    loss, grads = _grads(_model(fx, name), _input(fx, name), rec)
    assert abs(loss.item() - rec["loss_value"]) <= 1e-4 * max(1.0, abs(rec["loss_value"]))
    assert sorted(grads) == sorted(rec["grads"])
    for k, r in rec["grads"].items():
        assert grads[k] is not None, k
        _scaled_close(grads[k], r, GRAD_BAR, f"{name} gradient {k}")


@pytest.mark.parametrize("mode", ["bf16", "autocast"])
@pytest.mark.parametrize("name", NAMES)
def test_bf16_and_autocast_forward(fx, name, mode):
    rec = fx["cases"][name]
    m = _model(fx, name, torch.bfloat16 if mode == "bf16" else torch.float32)
    x = _input(fx, name)
    with torch.no_grad(), gm.autocast(torch.bfloat16, enabled=mode == "autocast"):
        tensors, _, _ = P.flatten_outputs(rec["kind"], m((x.bfloat16() if mode == "bf16" else x).cuda()))
    for i, (t, r, e) in enumerate(zip(tensors, rec["train"], rec["bf16_forward"])):
        assert t.dtype == torch.bfloat16 and tuple(t.shape) == r["shape"]
        err = (P.sample(t).double().cpu() - r["sample"].double()).abs()
        print(f"{name} {mode} tensor {i}: mean {err.mean().item():.3e} (reference {e['mean_err']:.3e}), max {err.max().item():.3e} (reference {e['max_err']:.3e})")
        assert err.mean().item() <= 1.5 * e["mean_err"] and err.max().item() <= 2.0 * e["max_err"], (name, mode, i)


@pytest.mark.parametrize("mode", ["bf16", "autocast"])
@pytest.mark.parametrize("name", NAMES)
def test_bf16_and_autocast_gradients(fx, name, mode):
    rec = fx["cases"][name]
    if mode == "bf16":
        _, grads = _grads(_model(fx, name, torch.bfloat16), _input(fx, name), rec, dtype=torch.bfloat16)
    else:
        _, grads = _grads(_model(fx, name), _input(fx, name), rec, autocast=True)
        assert all(g.dtype == torch.float32 for g in grads.values())  # fp32 masters get fp32 gradients, and so does the fp32 input
    keys = sorted(rec["grads"])
    got = P.rel_l2([P.sample(grads[k]) for k in keys], [rec["grads"][k]["sample"] for k in keys])
    print(f"{name} {mode}: gradient relative L2 {got:.3e} (reference {rec['bf16_grad_rel_l2']:.3e})")
    assert got <= 1.5 * rec["bf16_grad_rel_l2"]


@pytest.mark.parametrize("criterion", P.DSTEP_CRITERIA)
def test_discriminator_step(fx, criterion):
    """0.5 * (adv(D(fake)[-1], False, True) + adv(D(real)[-1], True, True)): two forwards before one backward."""
    rec = fx["dstep"]["criteria"][criterion]
    m = _model(fx, P.DSTEP_CASE)
    fake, real = P.dstep_fake(), _input(fx, P.DSTEP_CASE)
    assert float(fake.double().sum()) == fx["dstep"]["fake_sum"]
    adv = PatchAdversarialLoss(criterion=criterion)
    lf, lr = m(fake.cuda())[-1], m(real.cuda())[-1]
    _fp32_close(lf, rec["logits_fake"], "logits of the fake batch")
    _fp32_close(lr, rec["logits_real"], "logits of the real batch")
    loss = 0.5 * (adv(lf, False, True) + adv(lr, True, True))
    loss.backward()
    assert abs(loss.item() - rec["loss"]) <= 1e-4 * max(1.0, abs(rec["loss"])), (loss.item(), rec["loss"])
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert sorted(grads) == sorted(rec["grads"])
    for k, r in rec["grads"].items():
        _scaled_close(grads[k], r, GRAD_BAR, f"dstep {criterion} gradient {k}")
    _buffers_close(m, rec["buffers_after"], f"dstep {criterion}")  # (num_batches_tracked: 3 -> 5)


# ---- the loss kernel alone --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("for_discriminator", [True, False], ids=["discriminator", "generator"])
@pytest.mark.parametrize("target_is_real", [True, False], ids=["real", "fake"])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("criterion,no_act", [("bce", False), ("hinge", False), ("least_squares", False), ("least_squares", True)])
def test_loss_kernel_against_fp64(criterion, no_act, reduction, target_is_real, for_discriminator, dtype):
    g = torch.Generator().manual_seed(31)
    outs = [(2.0 * torch.randn(shape, generator=g)).to(dtype) for shape in ((2, 1, 6, 6), (2, 1, 3, 5, 7))]  # a multi-scale list: 72 and 210 logits
    real = target_is_real or not for_discriminator
    adv = PatchAdversarialLoss(reduction=reduction, criterion=criterion, no_activation_leastsq=no_act)
    xd = [o.cuda().requires_grad_(True) for o in outs]
    x64 = [o.double().requires_grad_(True) for o in outs]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = adv(xd, target_is_real, for_discriminator)
    bar = 1e-4 if dtype == torch.float32 else 2e-2  # the kernel computes in fp64; "none" rounds its terms to the logits' dtype
    if reduction == "none":
        assert isinstance(got, list) and len(got) == 2
        want = [P.criterion_terms(o, criterion, real, no_act) for o in x64]
        if criterion == "hinge":
            want = [w.mean() for w in want]
        up = [torch.randn(w.shape, generator=g, dtype=torch.float64) for w in want]
        for a, w in zip(got, want):
            assert a.shape == w.shape
            assert (a.double().cpu() - w.detach()).abs().max().item() <= bar * max(1.0, w.abs().max().item())
        sum((a * u.to(a.dtype).cuda()).sum() for a, u in zip(got, up)).backward()
        sum((w * u.to(dtype).double()).sum() for w, u in zip(want, up)).backward()
    else:
        want = P.criterion_value(x64, criterion, target_is_real, for_discriminator, reduction, no_act)
        assert got.dtype == torch.float32 and got.dim() == 0
        assert abs(got.item() - want.item()) <= 1e-6 * max(1.0, abs(want.item()))  # fp64 fold, one fp32 rounding
        got.backward()
        want.backward()
    for a, w in zip(xd, x64):
        assert a.grad.dtype == dtype and a.grad.shape == w.shape
        assert (a.grad.double().cpu() - w.grad).abs().max().item() <= bar * max(1e-3, w.grad.abs().max().item())


def test_loss_without_grad_and_repeatability():
    x = (2.0 * torch.randn((2, 1, 30, 30), generator=torch.Generator().manual_seed(5))).cuda()
    adv = PatchAdversarialLoss(criterion="bce")
    with torch.no_grad():
        a, b = adv(x, True, True), adv(x, True, True)
    assert torch.equal(a, b) and not a.requires_grad
    big = torch.tensor([[200.0, -200.0, 40.0, -40.0]]).cuda()  # torch's -100 clamp of the logarithm
    assert abs(adv(big, True, True).item() - (0.0 + 100.0 + 0.0 + 40.0) / 4) <= 1e-5
    assert abs(adv(big, False, True).item() - (100.0 + 0.0 + 100.0 + 0.0) / 4) <= 1e-5  # (1 - sigmoid(40) is 0 in fp64: the clamp, as in torch's own fp64)


# ---- refusals on the device -----------------------------------------------------------------------------------------------------------------------------
def test_training_forward_with_one_value_per_channel_raises_like_torch():
    m = PatchDiscriminator(2, 4, 1, num_layers_d=1, kernel_size=3, last_conv_kernel_size=1).cuda()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.randn(1, 1, 2, 2, device="cuda"))
    m.eval()
    assert tuple(m(torch.randn(1, 1, 2, 2, device="cuda"))[-1].shape) == (1, 1, 1, 1)


def test_input_checks_on_the_device():
    m = PatchDiscriminator(2, 4, 1).cuda()
    with pytest.raises(ValueError, match="expected a"):
        m(torch.zeros(2, 3, 32, 32, device="cuda"))
    with pytest.raises(TypeError, match="does not match the model dtype"):
        m(torch.zeros(2, 1, 32, 32, device="cuda", dtype=torch.bfloat16))


# ---- one discriminator step from a HIP graph ------------------------------------------------------------------------------------------------------------
def test_graphed_discriminator_step_equals_the_eager_step_bitwise(fx):
    fake, real = P.dstep_fake().cuda(), _input(fx, P.DSTEP_CASE).cuda()
    adv = PatchAdversarialLoss(criterion="least_squares")

    def step_of(m):
        return lambda f, r: 0.5 * (adv(m(f)[-1], False, True) + adv(m(r)[-1], True, True))

    graphed = _model(fx, P.DSTEP_CASE)
    step = gm.GraphedForwardBackward(step_of(graphed), (fake, real), graphed.parameters(), warmup=2)  # (before any eager step of this model)
    loss_g = step(fake, real).clone()
    eager = _model(fx, P.DSTEP_CASE)
    fn = step_of(eager)
    for _ in range(3):  # as many steps as the graphed model has run: two warm-up steps and one replay
        eager.zero_grad(set_to_none=True)
        loss_e = fn(fake, real)
        loss_e.backward()
    assert torch.equal(loss_g, loss_e.detach())
    for (k, pg), (_, pe) in zip(graphed.named_parameters(), eager.named_parameters()):
        assert torch.equal(pg.grad, pe.grad), k
    for (k, bg), (_, be) in zip(graphed.named_buffers(), eager.named_buffers()):
        assert torch.equal(bg, be), k  # running statistics and num_batches_tracked (3 + 2 * 3) advance inside the graph
    assert int(graphed[1].adn.N.num_batches_tracked) == 9
