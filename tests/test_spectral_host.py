"""CPU (-m "not gpu"): the planner of the Fourier kernels (generativemodels_amd/spectral_plan.py) and its NumPy emulator against numpy.fft, the
adjoint identity, the limits, JukeboxLoss's constructor contract (reference: generative/losses/spectral_loss.py), the conditions of the fixture
tests/golden/spectral_loss.pt, and the `generative.losses` alias.  Nothing is launched."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

import _spectral_cases as S
from generativemodels_amd import spectral_plan as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spectral_loss.pt")
FX = {c["name"]: c for c in torch.load(GOLDEN, weights_only=True)["cases"]}


def _case(name):
    return S.BY_NAME[name]


# ---- the emulator is a Fourier transform ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_fp64_emulator_against_numpy_fft_in_both_directions(name):
    case, plan = _case(name), S.plan_of(_case(name))
    x, _ = S.make_inputs(case["shape"], FX[name]["recipe"]["seed"])
    xd = x.double().numpy()
    axes = tuple(range(1, xd.ndim))
    ref = np.fft.fftn(xd, s=plan.m, axes=axes, norm=case["fft_norm"])
    got = plan.emulate_forward(xd)
    assert got.shape == plan.spectrum_shape
    err = np.abs(got - ref[..., :plan.half]).max() / np.abs(ref).max()
    # the adjoint on a random half spectrum: norm_scale * Re(unnormalised inverse of its Hermitian expansion), then the crop / zero-fill to the input extents
    g = np.random.default_rng(3)
    h = g.standard_normal(plan.spectrum_shape) + 1j * g.standard_normal(plan.spectrum_shape)
    full = np.zeros((plan.batch, *plan.m), dtype=np.complex128)
    full[..., :plan.half] = h
    mirror = np.conj(np.roll(np.flip(full, axes), 1, axes))  # conj(h[-k])
    full[..., plan.half:] = mirror[..., plan.half:]
    inv = np.fft.ifftn(full, axes=axes, norm="forward").real * plan.norm_scale  # norm="forward" on the inverse: no factor
    want = np.zeros((plan.batch, *plan.n))
    sl = (slice(None),) + tuple(slice(0, v) for v in plan.valid)
    want[sl] = inv[sl]
    back = plan.emulate_adjoint(h)
    assert back.shape == (plan.batch, *plan.n)
    err_adj = np.abs(back - want).max() / np.abs(want).max()
    print(f"{name}: forward {err:.2e}, adjoint {err_adj:.2e} relative to the largest magnitude")
    assert err < 1e-12 and err_adj < 1e-12


@pytest.mark.parametrize("name", S.NAMES)
def test_adjoint_identity_in_fp64(name):
    """<F x, y> == <x, F^H y> with the half spectrum's inner product Re sum w conj(a) b (w = 2 on the bins that stand for two)."""
    plan = S.plan_of(_case(name))
    g = np.random.default_rng(11)
    x = g.standard_normal((plan.batch, *plan.n))
    fx = plan.emulate_forward(x)
    # a half spectrum that is the half of a Hermitian one: the transform of another real tensor
    y = plan.emulate_forward(g.standard_normal((plan.batch, *plan.n)))
    w = P.half_weights(plan.m[-1])
    lhs = float((w * (np.conj(fx) * y).real).sum())
    rhs = float((x * plan.emulate_adjoint(y)).sum())
    print(f"{name}: <Fx, y> {lhs:.12e}, <x, F^H y> {rhs:.12e}")
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs), float(np.abs(x).sum()))


@pytest.mark.parametrize("name", S.NAMES)
def test_torch_fftn_and_the_fp32_emulator_sit_inside_the_kernel_bar(name):
    """The bar of the GPU kernel test, K * 2^-24 * S * s_norm * sum|x|, holds torch's own fp32 fftn and the plan's stages in fp32."""
    case, plan = _case(name), S.plan_of(_case(name))
    seed = FX[name]["recipe"]["seed"]
    x, _ = S.make_inputs(case["shape"], seed)
    ref, bar = S.forward_reference(case, seed)
    for what, got in (("torch.fft.fftn fp32", S.torch_half_spectrum(x, case)), ("fp32 emulator", plan.emulate_forward(x.numpy(), np.float32))):
        ratio = float((np.abs(got.astype(np.complex128) - ref) / bar).max())
        print(f"{name} {what}: largest err / bar {ratio:.3f}")
        assert ratio < 1.0, (what, ratio)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------
def test_every_length_is_served_and_the_factors_multiply_to_it():
    for n in list(range(1, 258)) + [1024, 9973, P.max_length()]:
        f = P.factorise(n)
        assert math.prod(f) == n and len(f) <= P.MAX_STAGES
        for r in f:
            assert r in P.DEDICATED or all(r % q for q in range(2, int(math.isqrt(r)) + 1)), (n, f)
    assert P.factorise(1) == () and P.factorise(8) == (4, 2) and P.factorise(194) == (2, 97) and P.factorise(12) == (4, 3)


def test_half_spectrum_weights_sum_to_the_full_count():
    for n in range(1, 40):
        w = P.half_weights(n)
        assert len(w) == n // 2 + 1 and w.sum() == n
    for name in S.NAMES:
        plan = S.plan_of(_case(name))
        assert math.prod(plan.spectrum_shape[:-1]) * P.half_weights(plan.m[-1]).sum() == plan.batch * plan.count


def test_twiddles_are_the_fp64_values_rounded_once():
    for n in (1, 2, 7, 12, 194, 1024):
        t = P.twiddles(n)
        assert t.dtype == np.float32 and t.shape == (n, 2)
        ang = -2.0 * np.pi * np.arange(n) / n
        assert (t[:, 0] == np.cos(ang).astype(np.float32)).all() and (t[:, 1] == np.sin(ang).astype(np.float32)).all()


def test_pass_order_lines_and_skipped_axes():
    plan = P.plan_for((2, 1, 12, 10))
    assert [p.axis for p in plan.forward] == [2, 1] and [p.axis for p in plan.adjoint] == [1, 2]  # C == 1 is skipped
    first, last = plan.forward[0], plan.adjoint[-1]
    assert (first.n, first.n_store, first.src, first.dst, first.inverse) == (10, 6, "x", "spec", False)
    assert (last.src_kind, last.dst, last.inverse, last.n_store) == (4, "x", True, 10)
    assert plan.adjoint[0].src == "h" and plan.adjoint[0].dst == "work" and last.src == "work"  # the saved spectrum is never written
    padded = P.plan_for((2, 3, 12, 10), (3, 16, 12))
    assert [(p.n, p.n_valid) for p in padded.forward] == [(12, 10), (16, 12), (3, 3)] and not padded.crops
    # the last-axis pass runs over the lines that hold data, not over the padded extent
    assert math.prod(padded.forward[0].extent) == 2 * 3 * 12 and math.prod(padded.forward[1].extent) == 2 * 3 * 7
    cropped = P.plan_for((2, 3, 12, 10), (2, 8, 7))
    assert cropped.crops and cropped.valid == (2, 8, 7) and cropped.adjoint[-1].n_store == 7
    assert P.plan_for((3, 2, 7, 1)).forward[0].n == 1  # the real -> complex pass always runs
    for name in S.NAMES:  # every line of every pass stays inside its operand
        plan = S.plan_of(_case(name))
        sizes = {"x": plan.batch * math.prod(plan.n), "spec": math.prod(plan.spectrum_shape), "h": math.prod(plan.spectrum_shape),
                 "work": math.prod(plan.spectrum_shape)}
        for p in plan.forward + plan.adjoint:
            n_read = p.n // 2 + 1 if p.src_kind == 4 else p.n_valid
            top_src = sum((e - 1) * s for e, s in zip(p.extent, p.src_stride)) + (n_read - 1) * p.src_axis_stride
            top_dst = sum((e - 1) * s for e, s in zip(p.extent, p.dst_stride)) + (p.n_store - 1) * p.dst_axis_stride
            assert top_src < sizes[p.src] and top_dst < sizes[p.dst], (name, p)
            assert math.prod(p.radices) == p.n


def test_the_limit_raises_before_any_launch():
    limit = P.max_length()
    assert limit == (160 * 1024 - 1024) // 16 - 1
    from generativemodels_amd import _native
    assert _native.lib().gm_dft_max_length() == limit
    P.SpectralPlan((1, 1, 2, limit))
    with pytest.raises(ValueError, match=str(limit)):
        P.SpectralPlan((1, 1, 2, limit + 1))
    with pytest.raises(ValueError, match=str(limit)):
        P.SpectralPlan((1, 1, 4, 4), fft_signal_size=(1, limit + 1, 4))
    for bad in ((4, 4), (1, 1, 2, 2, 2, 2), (1, 0, 4)):
        with pytest.raises(ValueError):
            P.SpectralPlan(bad)
    with pytest.raises(ValueError):
        P.SpectralPlan((1, 1, 4, 4), fft_signal_size=(4, 4))
    with pytest.raises(ValueError):
        P.SpectralPlan((1, 1, 4, 4), fft_norm="unitary")


# ---- the module ------------------------------------------------------------------------------------------------------------------------------------
def test_constructor_contract():
    from torch.nn.modules.loss import _Loss
    from generativemodels_amd.losses import JukeboxLoss
    m = JukeboxLoss(spatial_dims=2)
    assert isinstance(m, _Loss) and (m.spatial_dims, m.fft_signal_size, m.fft_norm, m.reduction, m.fft_dim) == (2, None, "ortho", "mean", (1, 2, 3))
    m = JukeboxLoss(3, fft_signal_size=(2, 8, 8, 8), fft_norm="forward", reduction="none")
    assert (m.fft_signal_size, m.fft_norm, m.reduction, m.fft_dim) == ((2, 8, 8, 8), "forward", "none", (1, 2, 3, 4))
    assert JukeboxLoss(1, reduction="sum").reduction == "sum"
    for kw in (dict(reduction="batch"), dict(fft_norm="unitary"), dict(fft_signal_size=(8, 8)), dict(fft_signal_size=(1, 0, 8))):
        with pytest.raises(ValueError):
            JukeboxLoss(2, **kw)
    with pytest.raises(ValueError):
        JukeboxLoss(4)
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU"):  # no eager fallback
        JukeboxLoss(2)(x, x)
    with pytest.raises(ValueError):
        JukeboxLoss(3)(x, x)


def test_generative_losses_resolves_after_install_as_generative():
    import generativemodels_amd as gm
    saved = {k: v for k, v in sys.modules.items() if k == "generative" or k.startswith("generative.")}
    try:
        gm.install_as_generative(force=True)
        from generative.losses import JukeboxLoss
        assert JukeboxLoss is importlib.import_module("generativemodels_amd.losses").JukeboxLoss
    finally:
        for k in [k for k in sys.modules if k == "generative" or k.startswith("generative.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------------------
def test_fixture_conditions_and_size():
    assert os.path.getsize(GOLDEN) < 1_000_000
    assert list(FX) == S.NAMES
    for name, c in FX.items():
        case = _case(name)
        assert (tuple(c["shape"]), c["fft_signal_size"], c["fft_norm"]) == (case["shape"], case["fft_signal_size"], case["fft_norm"])
        assert c["min_amplitude"] > 0
        x, y = S.make_inputs(c["recipe"]["shape"], c["recipe"]["seed"])
        assert torch.isfinite(c["grad_ref"]).all() and c["grad_ref"].shape == x.shape and c["grad_ref"].dtype == torch.float32
        for red in S.REDUCTIONS:
            assert c["e_ref_grad"][red] <= 2.0 ** -20 * c["grad_max"][red], (name, red)
        # the recorded fp64 values are those of the restatement on the recipe's inputs (the generator gives the same bits everywhere)
        v, gx, _ = S.exact(x, y, case, "mean")
        assert abs(float(v) - c["loss_fp64"]["mean"]) <= 1e-12 * abs(float(v))
        assert float((gx - c["grad_fp64"]).abs().max()) <= 1e-12 * c["grad_max"]["mean"]
        assert abs(c["loss_ref"]["mean"] - c["loss_fp64"]["mean"]) == pytest.approx(c["e_ref_loss"]["mean"], abs=1e-18)
