"""GPU (-m gpu): the Fourier kernels (gm_dft_lines, gm_spectral_loss through ops / autograd) and generative.losses.JukeboxLoss over the case list of
_spectral_cases.py, against fp64 on the CPU.

Bars.  Transform, fp32: K * 2^-24 * S * s_norm * sum|x| per element against the plan's fp64 emulator (K = 16, S = the sum over all stages of all passes
of radix + 2: the first-order bound of a direct evaluation, which any factorisation stays under).  Loss and gradient, fp32: max(e_ref, 8 * e_emul) from
tests/golden/spectral_loss.pt -- the distance of the reference in fp32, and of the plan's fp32 emulator, from fp64 -- the value not below
2^-24 * (log2 M + 8) * |loss| for the fold over M bins; gradients element-wise in max norm.  bf16 / fp16 operands: the same bars against fp64 on the rounded
values, the gradient plus 2^-8 |ref| (bf16) or 2^-11 |ref| (fp16) for the one rounding on store -- for fp16 not below 2^-25, half a step of its
subnormal range (_store_rounding)."""
import math
import os

import numpy as np
import pytest
import torch

import _spectral_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectral_loss.pt")
FX = {c["name"]: c for c in torch.load(GOLDEN, weights_only=True)["cases"]}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _loss(case, reduction):
    from generativemodels_amd.losses import JukeboxLoss
    return JukeboxLoss(len(case["shape"]) - 2, fft_signal_size=case["fft_signal_size"], fft_norm=case["fft_norm"], reduction=reduction)


def _inputs(name, dtype=torch.float32):
    """The case's operands rounded to `dtype`, as fp32 CPU tensors (the input of the fp64 yardstick too)."""
    x, y = S.make_inputs(S.BY_NAME[name]["shape"], FX[name]["recipe"]["seed"])
    return x.to(dtype).float(), y.to(dtype).float()


def _within(got, ref, tol, what):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).double()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"{what}: max|err| {float(err.max()):.3e}, largest err / bar {worst:.3f}")
    assert not bool((err > tol).any()), f"{what}: max|err| {float(err.max()):.3e}, largest err / bar {worst:.2f}"


def _bars(name, reduction, loss64):
    c = FX[name]
    value = max(c["e_ref_loss"][reduction], 8 * c["e_emul_loss"][reduction])
    if reduction != "none":
        value = max(value, S.fold_floor(S.BY_NAME[name], loss64))
    return value, max(c["e_ref_grad"][reduction], 8 * c["e_emul_grad"][reduction])


# ---- the transform ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_forward_transform_against_the_fp64_emulator(name):
    from generativemodels_amd import ops
    case = S.BY_NAME[name]
    plan = S.plan_of(case)
    seed = FX[name]["recipe"]["seed"]
    x, _ = S.make_inputs(case["shape"], seed)
    ref, bar = S.forward_reference(case, seed)
    spec = ops.dft_forward(x.to(DEV), plan)
    torch.cuda.synchronize()
    assert tuple(spec.shape) == (*plan.spectrum_shape, 2) and spec.dtype == torch.float32
    got = torch.view_as_complex(spec.cpu()).numpy().astype(np.complex128)
    err = np.abs(got - ref)
    assert np.isfinite(got).all()
    ratio = float((err / bar).max())
    print(f"{name}: S = {plan.stage_cost()}, max|err| {err.max():.3e}, largest err / bar {ratio:.3f}")
    assert ratio < 1.0
    # the adjoint of the spectrum the kernel made, against the fp64 emulator's adjoint of the same numbers: the bar of the transposed sum,
    # K * 2^-24 * S * s_norm * sum over the bins of weight * |h|
    back = ops.dft_adjoint(spec, plan, torch.float32)
    want = plan.emulate_adjoint(got)
    from generativemodels_amd.spectral_plan import half_weights
    mag = (np.abs(got) * half_weights(plan.m[-1])).reshape(plan.batch, -1).sum(1)
    abar = (S.K * S.EPS * plan.stage_cost() * plan.norm_scale * mag).reshape((-1,) + (1,) * len(plan.n))
    aerr = np.abs(back.double().cpu().numpy() - want)
    print(f"{name}: adjoint max|err| {aerr.max():.3e}, largest err / bar {float((aerr / abar).max()):.3f}")
    assert tuple(back.shape) == case["shape"] and float((aerr / abar).max()) < 1.0


def test_more_tiles_than_work_groups():
    """(64, 1, 4100, 2): the last-axis pass has 262 400 lines of 2 points = 4 100 tiles of 64 lines, more than the 4 096 work-groups of the grid, so some
    work-groups take a SECOND tile -- the line table and both LDS buffers are reused behind the barrier at the top of the tile loop.  The other pass
    transforms 4 100 = 4 * 5 * 5 * 41 points, one line per work-group.  Same bars as test_forward_transform_against_the_fp64_emulator."""
    from generativemodels_amd import ops
    from generativemodels_amd.spectral_plan import half_weights, plan_for
    shape = (64, 1, 4100, 2)
    plan = plan_for(shape)
    assert math.prod(plan.forward[0].extent) > 64 * 4096 and plan.forward[1].n == 4100
    x, _ = S.make_inputs(shape, 4100)
    ref = plan.emulate_forward(x.numpy(), np.float64)
    unit = S.K * S.EPS * plan.stage_cost() * plan.norm_scale
    bar = (unit * x.double().abs().flatten(1).sum(1).numpy()).reshape(-1, 1, 1, 1)
    spec = ops.dft_forward(x.to(DEV), plan)
    got = torch.view_as_complex(spec.cpu()).numpy().astype(np.complex128)
    ratio = float((np.abs(got - ref) / bar).max())
    back = ops.dft_adjoint(spec, plan, torch.float32)
    want = plan.emulate_adjoint(got)
    abar = (unit * (np.abs(got) * half_weights(2)).reshape(64, -1).sum(1)).reshape(-1, 1, 1, 1)
    aratio = float((np.abs(back.double().cpu().numpy() - want) / abar).max())
    print(f"4100 tiles: forward largest err / bar {ratio:.3f}, adjoint {aratio:.3f}")
    assert np.isfinite(got).all() and ratio < 1.0 and aratio < 1.0


# ---- the loss and its gradient ---------------------------------------------------------------------------------------------------------------------
PRECISIONS = [(r, d) for d in DTYPES for r in ("sum", "mean")]


def _store_rounding(ref, dtype):
    """Half a unit in the last place of `dtype` at |ref|, for the one rounding on store: 2^-8 |ref| (bf16), 2^-11 |ref| (fp16).  Below 2^-14 fp16 is
    subnormal: its spacing is 2^-24 whatever the value, so half a step there is 2^-25 -- "mean" scales a gradient by 1 / M into that range, where the
    exact fp64 gradient rounded once to fp16 is up to 387 x 2^-11 |ref| away (2x3x12x10-forward).  Where fp16 is normal the bar is 2^-11 |ref| itself."""
    rel = HALF_ULP[dtype] * ref.abs()
    return torch.clamp_min(rel, 2.0 ** -25) if dtype == torch.float16 else rel


@pytest.mark.parametrize("reduction,dt", PRECISIONS, ids=[f"{r}-{d}" for r, d in PRECISIONS])
@pytest.mark.parametrize("name", S.NAMES)
def test_loss_and_gradients_against_fp64(name, reduction, dt):
    dtype = DTYPES[dt]
    case = S.BY_NAME[name]
    x, y = _inputs(name, dtype)
    v64, gx64, gy64 = S.exact(x, y, case, reduction)
    if dtype == torch.float32:  # the recorded fp64 value is this evaluation
        assert abs(float(v64) - FX[name]["loss_fp64"][reduction]) <= 1e-12 * abs(float(v64))
    vbar, gbar = _bars(name, reduction, v64)
    xd, yd = x.to(dtype).to(DEV).requires_grad_(True), y.to(dtype).to(DEV).requires_grad_(True)
    v = _loss(case, reduction)(xd, yd)
    assert v.dtype == torch.float32 and v.dim() == 0 and v.requires_grad
    _within(v, v64, vbar, f"{name} {reduction} {dt} loss")
    v.backward()
    for what, g, g64, t in (("input", xd.grad, gx64, xd), ("target", yd.grad, gy64, yd)):
        assert g is not None and g.dtype == dtype and g.shape == t.shape
        _within(g, g64, gbar + _store_rounding(g64, dtype), f"{name} {reduction} {dt} d/d{what}")


@pytest.mark.parametrize("name", ["2x3x12x10", "1x2x30x17", "2x3x12x10-s2x8x7"])
def test_one_operand_alone_may_require_the_gradient(name):
    case = S.BY_NAME[name]
    x, y = _inputs(name)
    v64, gx64, gy64 = S.exact(x, y, case, "mean")
    _, gbar = _bars(name, "mean", v64)
    for which in (0, 1):
        ops_ = [x.to(DEV), y.to(DEV)]
        ops_[which].requires_grad_(True)
        v = _loss(case, "mean")(*ops_)
        v.backward()
        assert ops_[1 - which].grad is None
        _within(ops_[which].grad, (gx64, gy64)[which], gbar, f"{name} only operand {which}")
    with torch.no_grad():
        assert not _loss(case, "mean")(x.to(DEV), y.to(DEV)).requires_grad


@pytest.mark.parametrize("name", S.NAMES)
def test_reduction_none_map_mirror_and_gradient_for_a_non_symmetric_upstream(name):
    case = S.BY_NAME[name]
    plan = S.plan_of(case)
    x, y = _inputs(name)
    up = S.make_upstream(plan.full_shape, FX[name]["recipe"]["seed"])
    v64, gx64, gy64 = S.exact(x, y, case, "none", up)
    vbar, gbar = _bars(name, "none", None)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    v = _loss(case, "none")(xd, yd)
    assert tuple(v.shape) == tuple(v64.shape) == plan.full_shape and v.dtype == torch.float32
    _within(v, v64, vbar, f"{name} none map")
    dims = tuple(range(1, v.dim()))
    vc = v.detach().cpu()
    assert torch.equal(vc, torch.roll(torch.flip(vc, dims), (1,) * len(dims), dims)), "a bin and its mirror differ"
    v.backward(up.to(DEV))
    _within(xd.grad, gx64, gbar, f"{name} none d/dinput")
    _within(yd.grad, gy64, gbar, f"{name} none d/dtarget")


def test_a_bin_of_amplitude_zero_contributes_nothing():
    """x = a * 1, y = b * 1: every bin but the DC bin is exactly zero in both spectra (lengths with radices 2, 3, 4 only: the butterflies cancel equal inputs
    exactly), where the reference's gradient is NaN.  Here the gradient is that of the DC bin alone: with A = s N |a| and s the normalisation factor,
    dL/dx = u * 2 (|a| - |b|) s^2 N sign(a) at every element, u = 1 / (B N) for "mean".  Bar: each amplitude carries at most S + 8 roundings of 2^-24 (S of the
    plan's stages, 8 for the scale, the square root and the quotient); their difference is conditioned by c = (|a| + |b|) / ||a| - |b||, so the gradient is
    within (c + 1) (S + 8) 2^-24 of the closed form, plus its rounding on store, and the loss, a square of the difference, within 2 c (S + 8) 2^-24."""
    from generativemodels_amd.losses import JukeboxLoss
    from generativemodels_amd.spectral_plan import plan_for
    shape, a, b = (2, 3, 12, 8), 1.5, -0.75
    n = 3 * 12 * 8
    cond = (abs(a) + abs(b)) / abs(abs(a) - abs(b))
    unit = (plan_for(shape).stage_cost() + 8) * S.EPS
    for norm, s in (("ortho", 1 / math.sqrt(n)), ("backward", 1.0)):
        for reduction, u in (("sum", 1.0), ("mean", 1.0 / (shape[0] * n))):
            for dtype in (torch.float32, torch.bfloat16):
                x = torch.full(shape, a, dtype=dtype, device=DEV, requires_grad=True)
                y = torch.full(shape, b, dtype=dtype, device=DEV, requires_grad=True)
                v = JukeboxLoss(2, fft_norm=norm, reduction=reduction)(x, y)
                v.backward()
                want_v = u * shape[0] * (s * n * (abs(a) - abs(b))) ** 2
                gx = u * 2 * (abs(a) - abs(b)) * s * s * n * math.copysign(1.0, a)
                gy = u * 2 * (abs(b) - abs(a)) * s * s * n * math.copysign(1.0, b)
                tol = (cond + 1) * unit + HALF_ULP[dtype]
                _within(v, torch.tensor(want_v, dtype=torch.float64), 2 * cond * unit * want_v, f"constant images {norm} {reduction} {dtype} loss")
                _within(x.grad, torch.full(shape, gx, dtype=torch.float64), tol * abs(gx), f"constant images {norm} {reduction} {dtype} d/dinput")
                _within(y.grad, torch.full(shape, gy, dtype=torch.float64), tol * abs(gy), f"constant images {norm} {reduction} {dtype} d/dtarget")


def test_two_runs_are_bitwise_equal():
    for name in ("2x3x12x10", "1x1x16x16x16", "1x1x2x194"):
        case = S.BY_NAME[name]
        x, y = _inputs(name)
        runs = []
        for _ in range(2):
            xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
            v = _loss(case, "mean")(xd, yd)
            v.backward()
            runs.append((v.detach().clone(), xd.grad.clone(), yd.grad.clone()))
        for p, q in zip(*runs):
            assert torch.equal(p, q), name


def test_a_permuted_operand_gives_the_bits_of_its_dense_copy():
    case = S.BY_NAME["2x3x12x10"]
    x, y = _inputs("2x3x12x10")
    base = x.permute(0, 3, 2, 1).contiguous().to(DEV)  # (B, W, H, C) in memory
    view = base.permute(0, 3, 2, 1)
    assert not view.is_contiguous() and torch.equal(view.cpu(), x)
    out = []
    for t in (view, view.contiguous()):
        t = t.detach().requires_grad_(True)
        yd = y.to(DEV).requires_grad_(True)
        v = _loss(case, "mean")(t, yd)
        v.backward()
        out.append((v.detach(), t.grad, yd.grad))
    for p, q in zip(*out):
        assert torch.equal(p, q)
    assert out[0][1].shape == view.shape


def test_operands_must_be_device_tensors_of_one_shape_and_a_served_dtype():
    case = S.BY_NAME["2x1x8x8"]
    x, y = _inputs("2x1x8x8")
    loss = _loss(case, "mean")
    with pytest.raises(RuntimeError):
        loss(x, y.to(DEV))
    with pytest.raises(ValueError):
        loss(x.to(DEV), y[:1].to(DEV))
    with pytest.raises(TypeError):
        loss(x.double().to(DEV), y.double().to(DEV))
    # the gradient is differentiable once: a second differentiation raises, whichever way torch words it -- the gradient carries no graph when the
    # upstream does not require one, and an error node ("once_differentiable") when it does
    xd = x.to(DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(loss(xd, y.to(DEV)), xd, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    w = torch.ones((), device=DEV, requires_grad=True)
    (g,) = torch.autograd.grad(loss(xd, y.to(DEV)) * w, xd, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_autoencoder_reconstruction_trains_through_the_loss():
    """A small 2-D AutoencoderKL in train() mode: JukeboxLoss(reconstruction, image).backward() gives the parameter gradients that feeding the CPU fp64
    dL/dreconstruction into reconstruction.backward() gives.  Bar: test_gpu_backward.py's fp32 bar for parameter gradients, 3 * 2e-4 * max(1, |ref|)."""
    from generativemodels_amd.losses import JukeboxLoss
    from generativemodels_amd.networks.nets import AutoencoderKL
    torch.manual_seed(7)
    model = AutoencoderKL(spatial_dims=2, in_channels=1, out_channels=1, num_res_blocks=1, num_channels=(32, 64), attention_levels=(False, True),
                          latent_channels=4, norm_num_groups=32).to(DEV).train()
    g = torch.Generator().manual_seed(8)
    image = torch.randn((2, 1, 16, 16), generator=g)
    case = dict(fft_signal_size=None, fft_norm="ortho")

    def reconstruct():
        model.zero_grad(set_to_none=True)
        mu, _ = model.encode(image.to(DEV))
        return model.decode(mu)

    rec = reconstruct()
    loss = JukeboxLoss(2)(rec, image.to(DEV))
    loss.backward()
    native = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    rec = reconstruct()
    _, g64, _ = S.exact(rec.detach().float().cpu(), image, case, "mean")
    rec.backward(g64.float().to(DEV))
    checked = 0
    worst = 0.0
    for k, p in model.named_parameters():
        if p.grad is None:
            assert k not in native
            continue
        ref = p.grad.double().cpu()
        scale = max(1.0, float(ref.abs().max()))
        err = float((native[k].double().cpu() - ref).abs().max())
        worst = max(worst, err / (6e-4 * scale))
        assert err <= 6e-4 * scale, f"d {k}: max|err| {err:.3e} > {6e-4 * scale:.3e}"
        checked += 1
    print(f"autoencoder: {checked} parameter gradients, largest err / bar {worst:.4f}")
    assert checked > 30
