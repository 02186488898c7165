"""CPU (-m "not gpu"): DiffusionModelEncoder's constructor, state_dict layout and argument checks against tests/golden/encoder.pt
(tools/make_golden_encoder.py), the mirrored import path, and the host side of the head kernels.  No compute call is made -- there is no GPU here."""
import sys

import pytest
import torch

import _encoder_cases as E
import generativemodels_amd as gm
from _util import load_fixture
from generativemodels_amd import autograd as A
from generativemodels_amd import ops
from generativemodels_amd.inferers import classifier_guidance_gradient
from generativemodels_amd.networks.nets import DiffusionModelEncoder

NAMES = sorted(E.CASES)


@pytest.fixture(scope="module")
def fx():
    return load_fixture("encoder")


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_keys_order_and_shapes(fx, name):
    m = DiffusionModelEncoder(**E.CASES[name]["cfg"])
    want = fx["cases"][name]["shapes"]
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want)  # keys AND order
    assert got == want
    m.load_state_dict(E.make_state_dict(want, E.CASES[name]["seed"]), strict=True)
    assert isinstance(m.out[2], torch.nn.Dropout) and m.out[2].p == 0.1
    assert tuple(m.out[0].weight.shape) == (512, 4096) and tuple(m.out[3].weight.shape) == (E.CASES[name]["cfg"]["out_channels"], 512)
    assert m.supports_training()


def test_defaults_are_the_references():
    m = DiffusionModelEncoder(spatial_dims=2, in_channels=1, out_channels=3)
    assert m.block_out_channels == (32, 64, 64, 64) and m.attention_levels == (False, False, True, True) and m.num_res_blocks == (2, 2, 2, 2)
    assert len(m.down_blocks) == 4 and all(hasattr(st, "downsampler") for st in m.down_blocks)  # every level downsamples, the last included
    assert not hasattr(m, "middle_block")


def test_int_num_res_blocks_is_accepted():
    m = DiffusionModelEncoder(spatial_dims=2, in_channels=1, out_channels=2, num_res_blocks=2, num_channels=(8, 16), attention_levels=(False, False),
                              norm_num_groups=8)
    assert [len(st.resnets) for st in m.down_blocks] == [2, 2]


def test_constructor_errors():
    kw = dict(spatial_dims=2, in_channels=1, out_channels=2)
    with pytest.raises(ValueError, match=r"DiffusionModelEncoder expects dimension of the cross-attention conditioning \(cross_attention_dim\) when using with_conditioning\."):
        DiffusionModelEncoder(**kw, with_conditioning=True)
    with pytest.raises(ValueError, match=r"DiffusionModelEncoder expects with_conditioning=True when specifying the cross_attention_dim\."):
        DiffusionModelEncoder(**kw, cross_attention_dim=8)
    with pytest.raises(ValueError, match="DiffusionModelEncoder expects all num_channels being multiple of norm_num_groups"):
        DiffusionModelEncoder(**kw, num_channels=(32, 48), attention_levels=(False, False))
    with pytest.raises(ValueError, match="DiffusionModelEncoder expects num_channels being same size of attention_levels"):
        DiffusionModelEncoder(**kw, num_channels=(32, 64), attention_levels=(False, False, True))
    with pytest.raises(ValueError, match="num_head_channels should have the same length as attention_levels"):
        DiffusionModelEncoder(**kw, num_channels=(32, 64), attention_levels=(False, False), num_head_channels=(8, 8, 8))


def _small(**extra):
    return DiffusionModelEncoder(**dict(E.CASES["a2d"]["cfg"], **extra))


def test_forward_errors_come_before_any_launch():
    """CPU tensors: a check that let the call through would end in the no-fallback error instead of the ValueError."""
    x, t = torch.zeros(E.CASES["a2d"]["input"]), torch.zeros(4)
    with pytest.raises(ValueError, match="model should have with_conditioning = True if context is provided"):
        _small()(x, t, context=torch.zeros(4, 1, 16))
    with pytest.raises(ValueError, match="class_labels should be provided when num_class_embeds > 0"):
        _small(num_class_embeds=3)(x, t)
    with pytest.raises(ValueError, match="2048 features"):
        _small()(torch.zeros(4, 1, 32, 64), t)
    with pytest.raises(ValueError, match="2048 features"):
        _small()._encode(torch.zeros(4, 1, 32, 64), t)
    with pytest.raises(ValueError, match="2048 features"):
        classifier_guidance_gradient(_small(), torch.zeros(4, 1, 32, 64), t, torch.zeros(4, dtype=torch.long))


def test_cpu_tensors_raise_the_no_fallback_error():
    m = _small()
    x, t = torch.zeros(E.CASES["a2d"]["input"]), torch.zeros(4)
    def no_grad_eval():
        with torch.no_grad():
            m.eval()(x, t)

    for call in (no_grad_eval, lambda: m.train()(x, t), lambda: m.eval()(x.requires_grad_(True), t),
                 lambda: ops.classifier_head(torch.zeros(1, 256, 16), torch.zeros(512, 4096), None, torch.zeros(2, 512), None),
                 lambda: ops.classifier_head_backward(torch.zeros(1, 256, 16), torch.zeros(1, 512), None, torch.zeros(512, 4096), torch.zeros(2, 512), g=torch.zeros(1, 2))):
        with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
            call()


def test_feature_shape_follows_the_resampler():
    assert _small()._feature_shape((32, 128)) == (8, 32)
    assert _small()._feature_shape((31, 127)) == (8, 32)  # strided convolution, padding 1: (n - 1) // 2 + 1
    assert _small(resblock_updown=True)._feature_shape((32, 128)) == (8, 32)


def test_install_as_generative_resolves_the_tutorials_import():
    keep = {k: v for k, v in sys.modules.items() if k == "generative" or k.startswith("generative.")}
    try:
        gm.install_as_generative(force=True)
        from generative.networks.nets.diffusion_model_unet import DiffusionModelEncoder as Enc2
        from generative.networks.nets.diffusion_model_unet import DiffusionModelUNet as UNet2
        from generative.networks.nets import DiffusionModelEncoder as Enc3

        import generativemodels_amd.networks.nets.diffusion_model_unet as mod

        assert Enc2 is DiffusionModelEncoder is Enc3 is mod.DiffusionModelEncoder
        assert UNet2 is mod.DiffusionModelUNet is gm.networks.nets.DiffusionModelUNet
        assert sys.modules["generative.networks.nets.diffusion_model_unet"] is mod  # not a second copy of the module
    finally:
        for k in [k for k in sys.modules if k == "generative" or k.startswith("generative.")]:
            del sys.modules[k]
        sys.modules.update(keep)


def test_public_names():
    assert "classifier_head" in A.__all__ and callable(A.classifier_head)
    assert "classifier_guidance_gradient" in gm.inferers.__all__
    assert "DiffusionModelEncoder" in gm.networks.nets.__all__


def test_head_chunk_is_a_host_entry():
    assert ops.classifier_head_chunk(torch.float32) == 4 and ops.classifier_head_chunk(torch.bfloat16) == 8
    with pytest.raises(TypeError):
        ops.classifier_head_chunk(torch.float16)
    for dtype in (torch.float32, torch.bfloat16):  # a chunk of 4096-feature samples fits the 64 KiB a launch stages in LDS
        assert ops.classifier_head_chunk(dtype) * 4096 * torch.empty((), dtype=dtype).element_size() <= 65536


def test_fixture_is_sound(fx):
    assert sorted(fx["cases"]) == NAMES
    for name in NAMES:
        rec = fx["cases"][name]
        assert float(E.case_input(name).double().sum()) == rec["input_sum"], "the seeded generator drew other numbers than the fixture's: regenerate it"
        assert rec["fp32_err"]["values"] <= 0.1 * E.FP32_BAR and rec["fp32_err"]["grads"] <= 0.1 * E.GRAD_BAR
        feat = rec["features"]["shape"]
        assert feat[1] * torch.Size(feat[2:]).numel() == 4096 and (name == "tut" or len(set(rec["input_shape"][2:])) > 1)  # 4096 features; no square / cubic input
        # (but the tutorial's own 64 x 64)
        assert all(k in rec["grads"] for k in ("input", "out.0.weight", "out.0.bias", "out.3.weight", "out.3.bias"))
    ch = fx["chain"]
    bar = E.FP32_BAR * E.CHAIN_FACTOR * max(1.0, ch["guided"].abs().max().item())
    assert ch["fp32_err"] <= 0.1 * bar and (ch["guided"] - ch["unguided"]).abs().max().item() >= 100 * bar
