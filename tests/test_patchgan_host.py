"""CPU (-m "not gpu"): the host side of the PatchGAN discriminators and the adversarial loss, against tests/golden/patchgan.pt (written by
tools/make_golden_patchgan.py from the unmodified reference) and torch's own pooling.  Needs no reference tree and no GPU."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _patchgan_cases as P
import generativemodels_amd as gm
from _util import load_fixture
from generativemodels_amd import autograd as A
from generativemodels_amd.losses import AdversarialCriterions, PatchAdversarialLoss
from generativemodels_amd.networks.nets import MultiScalePatchDiscriminator, PatchDiscriminator
from generativemodels_amd.resize_plan import ResizePlan, avg_pool_plan, avg_pool_taps


@pytest.fixture(scope="module")
def fx():
    return load_fixture("patchgan")


def _build(case):
    return (PatchDiscriminator if case["kind"] == "patch" else MultiScalePatchDiscriminator)(**case["cfg"])


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_state_dict_keys_and_shapes_are_the_references(fx, name):
    want = fx["cases"][name]["shapes"]
    m = _build(P.CASES[name])
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want) and got == want
    m.load_state_dict(P.make_state_dict(want, P.CASES[name]["seed"]))  # strict
    x = P.case_input(name, fx["cases"][name]["input_seed"])
    assert tuple(x.shape) == fx["cases"][name]["input_shape"] and float(x.double().sum()) == fx["cases"][name]["input_sum"]


def test_state_dict_names_of_the_layers():
    sd = PatchDiscriminator(2, 8, 1, num_layers_d=2, bias=True).state_dict()
    for k in ("initial_conv.conv.weight", "initial_conv.conv.bias", "0.conv.weight", "0.conv.bias", "0.adn.N.weight", "0.adn.N.bias", "0.adn.N.running_mean",
              "0.adn.N.running_var", "0.adn.N.num_batches_tracked", "1.adn.N.weight", "final_conv.conv.weight", "final_conv.conv.bias"):
        assert k in sd, k
    assert "0.conv.bias" not in PatchDiscriminator(2, 8, 1, num_layers_d=2).state_dict()
    ms = MultiScalePatchDiscriminator(num_d=3, num_layers_d=1, spatial_dims=2, num_channels=4, in_channels=1, pooling_method="avg", minimum_size_im=32)
    keys = list(ms.state_dict())
    assert "discriminator_0.initial_conv.conv.weight" in keys and "discriminator_1.1.0.adn.N.running_var" in keys and "discriminator_2.2.final_conv.conv.bias" in keys
    deep = MultiScalePatchDiscriminator(num_d=2, num_layers_d=1, spatial_dims=3, num_channels=4, in_channels=1, minimum_size_im=32)
    assert deep.num_layers_d == [1, 2] and "discriminator_1.1.conv.weight" in deep.state_dict()
    assert not any(".adn.N." in k for k in PatchDiscriminator(2, 8, 1, norm="INSTANCE").state_dict())


def test_constructor_errors():
    with pytest.raises(AssertionError, match="image size is too small"):
        MultiScalePatchDiscriminator(num_d=2, num_layers_d=6, spatial_dims=2, num_channels=4, in_channels=1, minimum_size_im=32)
    with pytest.raises(AssertionError, match="must match the number of num_layers_d"):
        MultiScalePatchDiscriminator(num_d=2, num_layers_d=[1, 2, 3], spatial_dims=2, num_channels=4, in_channels=1)
    for kw, word in ((dict(norm="GROUP"), "GROUP"), (dict(norm=("BATCH", {"eps": 1e-3})), "eps"), (dict(activation="PRELU"), "PRELU"),
                     (dict(activation=("LEAKYRELU", {"negative_slope": -0.1})), "-0.1"), (dict(dropout=0.1), "0.1"), (dict(spatial_dims=1), "spatial_dims=1")):
        args = dict(spatial_dims=2, num_channels=4, in_channels=1)
        args.update(kw)
        with pytest.raises(NotImplementedError, match=word):
            PatchDiscriminator(**args)
    with pytest.raises(NotImplementedError, match="max"):
        MultiScalePatchDiscriminator(num_d=2, num_layers_d=1, spatial_dims=2, num_channels=4, in_channels=1, pooling_method="max", minimum_size_im=32)
    PatchDiscriminator(3, 4, 1, activation="RELU", norm="instance")  # served spellings


def test_initialisation_distributions():
    torch.manual_seed(3)
    m = PatchDiscriminator(2, 64, 3, num_layers_d=3)
    w = m[2].conv.weight.detach()  # 256 x 128 x 4 x 4
    assert abs(w.mean().item()) < 2e-4 and abs(w.std().item() - 0.02) < 2e-4
    g = torch.cat([m[i].adn.N.weight.detach() for i in (1, 2, 3)])
    assert abs(g.mean().item() - 1.0) < 3e-3 and abs(g.std().item() - 0.02) < 3e-3
    assert all(bool((m[i].adn.N.bias == 0).all()) for i in (1, 2, 3))
    assert bool((m[1].adn.N.running_mean == 0).all()) and bool((m[1].adn.N.running_var == 1).all()) and int(m[1].adn.N.num_batches_tracked) == 0


def test_distributed_batchnorm_warning(monkeypatch):
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    with pytest.warns(UserWarning, match="SyncBatchNorm"):
        PatchDiscriminator(2, 4, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        PatchDiscriminator(2, 4, 1, norm="INSTANCE")


def test_install_as_generative_serves_the_reference_paths():
    import sys

    def aliases():
        return [k for k in sys.modules if k == "generative" or k.startswith("generative.")]
    saved = {k: sys.modules[k] for k in aliases()}
    try:
        gm.install_as_generative(force=True)
        from generative.losses import PatchAdversarialLoss as L1
        from generative.losses.adversarial_loss import AdversarialCriterions as C2
        from generative.losses.adversarial_loss import PatchAdversarialLoss as L2
        from generative.networks.nets import MultiScalePatchDiscriminator as M1
        from generative.networks.nets.patchgan_discriminator import MultiScalePatchDiscriminator as M2
        from generative.networks.nets.patchgan_discriminator import PatchDiscriminator as D2
        assert L1 is L2 is PatchAdversarialLoss and C2 is AdversarialCriterions and M1 is M2 is MultiScalePatchDiscriminator and D2 is PatchDiscriminator
    finally:  # later tests see the modules they saw before
        for k in aliases():
            del sys.modules[k]
        sys.modules.update(saved)
    assert "batch_norm_act" in A.__all__ and "patch_adv_loss" in A.__all__ and "avg_pool" in A.__all__


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        PatchDiscriminator(2, 4, 1)(torch.zeros(2, 1, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        MultiScalePatchDiscriminator(num_d=2, num_layers_d=1, spatial_dims=2, num_channels=4, in_channels=1, pooling_method="avg", minimum_size_im=32)(
            torch.zeros(2, 1, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        PatchAdversarialLoss()(torch.zeros(2, 1, 6, 6), True, True)
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        A.batch_norm_act(torch.zeros(2, 4, 4, 8), None, None, torch.zeros(8), torch.ones(8), True, 0.1, 1e-5, 0.2)


# ---- average pooling as tap tables ---------------------------------------------------------------------------------------------------------------
def _apply(plan, x):
    """The plan's tables applied with numpy to a channels-first tensor (N, C, *spatial), axis by axis."""
    y = x.double().numpy()
    for a, tab in enumerate(plan.tables):
        m = np.zeros((len(tab.start) - 1, plan.in_spatial[a]))
        for o in range(len(tab.start) - 1):
            for t in range(tab.start[o], tab.start[o + 1]):
                m[o, tab.index[t]] += np.float64(tab.weight[t])
        y = np.moveaxis(np.tensordot(m, y, axes=(1, 2 + a)), 0, 2 + a)
    return torch.from_numpy(y)


@pytest.mark.parametrize("include_pad", [True, False])
@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("spatial", [(8, 9), (7, 12), (6, 7, 9), (8, 8, 5)])
def test_avg_pool_tables_reproduce_torch(spatial, k, include_pad):
    pad = (k - 1) // 2
    x = torch.randn((2, 3, *spatial), generator=torch.Generator().manual_seed(sum(spatial) + k), dtype=torch.float64)
    pool = F.avg_pool2d if len(spatial) == 2 else F.avg_pool3d
    want = pool(x, k, 2, pad, count_include_pad=include_pad)
    plan = avg_pool_plan(spatial, k, 2, pad, include_pad)
    assert plan.out_spatial == tuple(want.shape[2:]) and plan.max_taps == k ** len(spatial)
    assert (_apply(plan, x) - want).abs().max().item() <= 1e-7  # (the weights are fp32: 1 / 3 is not exact)
    back = ResizePlan.from_taps("t", plan.out_spatial, [[[(int(i), w) for i, w in zip(t.index[t.start[o]:t.start[o + 1]], t.weight[t.start[o]:t.start[o + 1]])]
                                                          for o in range(len(t.start) - 1)] for t in plan.transposed])
    gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    pool(xr, k, 2, pad, count_include_pad=include_pad).backward(gy)
    assert (_apply(back, gy) - xr.grad).abs().max().item() <= 1e-7  # the gradient runs on the transposed tables
    assert avg_pool_plan(spatial, k, 2, pad, include_pad) is plan


def test_avg_pool_and_explicit_tables_argument_errors():
    with pytest.raises(ValueError, match="too short"):
        avg_pool_taps(2, 4, 2, 0)
    with pytest.raises(ValueError, match="padding"):
        avg_pool_taps(8, 3, 2, 2)
    with pytest.raises(ValueError, match="tap tables"):
        ResizePlan.from_taps("t", (4, 4), [[[(0, 1.0)]]])
    with pytest.raises(ValueError, match="inside its axis"):
        ResizePlan.from_taps("t", (4,), [[[(4, 1.0)]]])


# ---- the loss -----------------------------------------------------------------------------------------------------------------------------------------
def test_loss_argument_errors_and_members():
    assert [m.value for m in AdversarialCriterions] == ["bce", "hinge", "least_squares"]
    with pytest.raises(ValueError, match="Unrecognised criterion"):
        PatchAdversarialLoss(criterion="wasserstein")
    with pytest.raises(ValueError):
        PatchAdversarialLoss(reduction="average")
    loss = PatchAdversarialLoss(criterion="hinge")
    assert (loss.real_label, loss.fake_label, loss.criterion, loss.reduction) == (1.0, -1.0, "hinge", "mean")
    assert PatchAdversarialLoss().fake_label == 0.0 and PatchAdversarialLoss().activation and not PatchAdversarialLoss(no_activation_leastsq=True).activation
    assert PatchAdversarialLoss(criterion="bce", no_activation_leastsq=True).activation


def test_generator_side_warning_comes_before_the_device_check():
    with pytest.warns(UserWarning, match="target_is_real must be set to True"):
        with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
            PatchAdversarialLoss()(torch.zeros(2, 1, 6, 6), False, False)


@pytest.mark.parametrize("criterion", P.DSTEP_CRITERIA)
def test_fp64_restatement_of_the_criteria_gives_the_fixtures_losses(fx, criterion):
    """The formulas the kernel implements, in plain fp64 torch, against what the reference returned for the two logit maps of the discriminator step."""
    rec = fx["dstep"]["criteria"][criterion]
    got = 0.5 * (P.criterion_value(rec["logits_fake"], criterion, False, True) + P.criterion_value(rec["logits_real"], criterion, True, True))
    assert abs(got.item() - rec["loss"]) <= 1e-12 * max(1.0, abs(rec["loss"]))
    assert tuple(rec["logits_fake"].shape) == (2, 1, 6, 6)
    assert {int(v) for k, v in rec["buffers_after"].items() if k.endswith("num_batches_tracked")} == {5}
